"""Device-side tower engine: packed ViT weights resident in HBM + the composed HIP forward (visrep_vit_forward).

PyTorch is used for device memory and streams only; every FLOP of the forward runs in libvisrep_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import torch

from . import _lib
from .vit_weights import ViTSpec, prefix_table


def _round_up(v: int, a: int) -> int:
    return (v + a - 1) // a * a


def head_pad_for(head_dim: int) -> int:
    """Width a head occupies in the bf16 engine's buffers: 64, 96 (true widths 65 .. 96: attn_fwd96) or 128 (97 .. 128: attn_fwd<2>)."""
    if head_dim < 64 or head_dim > 128:
        raise ValueError("HIP attention kernel supports head_dim 64 .. 128 only (narrower and wider heads: the fp32 engine)")
    return 64 if head_dim == 64 else 96 if head_dim <= 96 else 128


def pad_tower_weights(spec: ViTSpec, layer: dict, dp: int, mp: int) -> dict:
    """One layer's matrices with every head zero-padded from d / heads to `dp` lanes and the MLP from spec.mlp to `mp` units (host, fp32).
    wqkv [3d, d] -> [3 heads dp, d] (the q, k and v rows of head h at h dp inside their block), bqkv likewise, wo [d, d] -> [d, heads dp]
    (columns), w1 / b1 rows and w2 columns -> mp.  All padding is zeros, so nothing changes in exact arithmetic: a padded Q or K lane adds
    0 * 0 to every score, a padded V lane is an output lane that meets a zero wo column, a padded MLP unit has zero weight and bias
    (every activation here maps 0 to 0) and meets a zero w2 column."""
    H, d, m = spec.heads, spec.d, spec.mlp
    dh = d // H
    L = dict(layer)
    if dp != dh:
        def rows(t):                                   # [3 d, ...] -> [3 H dp, ...]
            t = t.detach().float()
            out = torch.zeros((3, H, dp) + tuple(t.shape[1:]))
            out[:, :, :dh] = t.reshape((3, H, dh) + tuple(t.shape[1:]))
            return out.reshape((3 * H * dp,) + tuple(t.shape[1:]))
        L["wqkv"] = rows(L["wqkv"])
        if L.get("bqkv") is not None:
            L["bqkv"] = rows(L["bqkv"])
        wo = torch.zeros(d, H, dp)
        wo[:, :, :dh] = L["wo"].detach().float().reshape(d, H, dh)
        L["wo"] = wo.reshape(d, H * dp)
    if mp != m:
        halves = 2 if spec.act == "swiglu" else 1          # swiglu: the gate half and the value half are padded each (silu(0) * 0 = 0)
        w1 = torch.zeros(halves, mp, d)
        w1[:, :m] = L["w1"].detach().float().reshape(halves, m, d)
        w2 = torch.zeros(d, mp)
        w2[:, :m] = L["w2"].detach().float()
        L["w1"], L["w2"] = w1.reshape(halves * mp, d), w2
        if L.get("b1") is not None:
            b1 = torch.zeros(halves, mp)
            b1[:, :m] = L["b1"].detach().float().reshape(halves, m)
            L["b1"] = b1.reshape(halves * mp)
    return L


def pad_qk_gain(spec: ViTSpec, g: Optional[torch.Tensor], dp: int) -> torch.Tensor:
    """A QK-norm weight [d] (None = ones) with every head zero-padded to `dp` lanes -> [heads dp] (fp32): the padded Q / K columns are zero
    before the norm (pad_tower_weights) and, with a zero gain, stay zero behind it.  visrep_qk_rmsnorm divides the sum of squares by the TRUE width d."""
    H, dh = spec.heads, spec.d // spec.heads
    out = torch.zeros(H, dp)
    out[:, :dh] = 1.0 if g is None else g.detach().float().reshape(H, dh)
    return out.reshape(H * dp)


def swiglu_interleave_index(mp: int) -> torch.Tensor:
    """Row order of the gated GEMM (visrep_gemm_bf16_gated) in terms of HF chunk order [gate 0 .. mp | value 0 .. mp]: GEMM row 32 t + r is the
    gate row of hidden unit 16 t + r, row 32 t + 16 + r its value row (r < 16).  `x[idx]` interleaves, `out[idx] = y` undoes it."""
    if mp % 16:
        raise ValueError("swiglu interleave: the (padded) hidden width must be a multiple of 16")
    unit = torch.arange(mp).reshape(mp // 16, 1, 16)
    return torch.cat([unit, unit + mp], dim=1).reshape(2 * mp)


_SCRATCH = {}


def ensure_scratch(device, nbytes: int = 64 << 20) -> None:
    """One split-K scratch PER DEVICE for visrep_gemm_bf16 (visrep_set_scratch registers it for the current device): few-tile
    problems - the 128x128 tail launches of the ViT GEMMs, the low-resolution convolutions of the diffusion towers - split their K
    loop over idle CUs.  S * M * N * 4 bytes <= 33.6 MB by construction of the split rule (S * tiles <= 2 * 256 block slots,
    128x128 tiles).  The planes are not keyed by stream: one stream per device runs GEMMs at a time (every engine here does)."""
    device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _SCRATCH:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        with torch.cuda.device(idx):
            _lib.check(_lib.require_gpu().visrep_set_scratch(_lib.ptr(buf), nbytes), "visrep_set_scratch")
        _SCRATCH[idx] = buf


class _TowerEngine:
    """What every tower engine does on the host side of the library: it resolves the device, keeps the tensors whose raw pointers the tables
    hold, checks and converts a pixel batch, range-checks the state index and caches workspaces per batch size; an engine with a workspace
    supplies _workspace_bytes(B)."""

    WS_KEEP = 5                                            # unpinned workspaces that stay resident beside the one being asked for
    WS_ZERO = True                                         # the forward expects a zero-filled workspace
    PIXEL_DTYPES = (torch.float32, torch.bfloat16)         # what the forward reads as it is; every other pixel dtype is cast to fp32

    def __init__(self, lib, spec, device):
        self.lib = lib
        self.spec = spec
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self._keep = []                      # tensors referenced by raw pointers, in packing order (sweep.tower_fingerprint hashes them in it)
        self._ws: Dict[int, torch.Tensor] = {}
        self._pinned = set()                 # batch sizes whose workspace a captured HIP graph refers to

    def _hold(self, t, dtype=None):
        """`t` on the engine's device (as `dtype`, if given), contiguous and kept alive; None stays None."""
        if t is None:
            return None
        x = t.detach().to(device=self.device, dtype=dtype).contiguous()
        self._keep.append(x)
        return x

    def _pixels(self, pixels: torch.Tensor) -> torch.Tensor:
        side = self.spec.image_size
        if pixels.dim() != 4 or pixels.shape[1] != 3 or pixels.shape[2] != side or pixels.shape[3] != side:
            raise ValueError(f"Input image size {tuple(pixels.shape)} doesn't match tower ({side}*{side}).")
        px = pixels.to(self.device)
        if px.dtype not in self.PIXEL_DTYPES:
            px = px.float()
        return px.contiguous()

    def _state(self, n: Optional[int], message: str) -> int:
        """The hidden-state index a forward stops at: None = the last one, anything outside 0 .. n_layers is `message`."""
        n = self.n_layers if n is None else n
        if not 0 <= n <= self.n_layers:
            raise ValueError(message)
        return n

    def _allocate(self, nbytes: int) -> torch.Tensor:
        return (torch.zeros if self.WS_ZERO else torch.empty)(nbytes, dtype=torch.uint8, device=self.device)

    def workspace(self, B: int) -> torch.Tensor:
        """The workspace of batch size B.  WS_KEEP unpinned ones stay resident beside it, oldest dropped first (before the new one is allocated:
        with WS_KEEP = 0 two never coexist).  One that a HIP graph captured (the image-variation featurizer records a forward inside its own
        graph) is PINNED: a replayed graph keeps using the pointer it saw, so it is never dropped."""
        ws = self._ws.get(B)
        if ws is None:
            nbytes = self._workspace_bytes(B)
            unpinned = [b for b in self._ws if b not in self._pinned]
            for old in unpinned[: max(0, len(unpinned) - self.WS_KEEP)]:
                self._ws.pop(old)
            ws = self._ws[B] = self._allocate(nbytes)
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            self._pinned.add(B)
        return ws


def _addr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


_VIT_MATRICES = ("wqkv", "wo", "w1", "w2")
_VIT_VECTORS = ("ln1_g", "ln1_b", "bqkv", "bo", "ls1", "ln2_g", "ln2_b", "b1", "b2", "ls2", "sqkv", "s1")


def _vit_vector_table(spec: ViTSpec, weights: dict) -> dict:
    """The tower-level vectors of VitWeights; cls = [d], or [1 + registers, d]: the class token, then the register tokens."""
    return {**{k: weights.get(k) for k in ("patch_b", "pos", "pre_ln_g", "pre_ln_b")}, "cls": prefix_table(spec, weights)}


def _fill_vit_tables(eng: _TowerEngine, patch_w: torch.Tensor, vecs: dict, layers, mat_dtype=torch.float32) -> list:
    """Upload a ViT tower and fill what visrep_vit_forward* read: eng._w (VitWeights), eng._layers (the VitLayer array, eng.n_layers long) and
    eng._vecs.  Tensors enter eng._keep as patch matrix, vector table, then per layer the four matrices (as `mat_dtype`), the fp32 vectors,
    sqkv / s1 and - QK-norm towers - the two gains.  `layers`: one dict per layer, absent or None entries = null pointers; a generator keeps
    one prepared layer on the host at a time.  Returns, per layer, name -> the tensor held."""
    eng._patch_w = eng._hold(patch_w, mat_dtype)
    eng._vecs = {k: eng._hold(v, torch.float32) for k, v in vecs.items()}
    eng._layers = (_lib.VitLayer * max(eng.n_layers, 1))()
    names = _VIT_MATRICES + _VIT_VECTORS + (("qn_g", "kn_g") if eng.spec.qk_norm else ())
    held = []
    for ent, L in zip(eng._layers, layers):
        held.append({k: eng._hold(L.get(k), mat_dtype if k in _VIT_MATRICES else torch.float32) for k in names})
        for k, v in held[-1].items():
            setattr(ent, k, _addr(v))
    eng._w = _lib.VitWeights(patch_w=eng._patch_w.data_ptr(), layers=C.cast(eng._layers, C.POINTER(_lib.VitLayer)))
    for k, v in eng._vecs.items():
        setattr(eng._w, k, _addr(v))
    return held


def _raw_vit_layers(spec: ViTSpec, weights: dict):
    """The packed layers as the fp32 engines take them: untouched, absent QK gains = ones."""
    for L in weights["layers"]:
        if spec.qk_norm:
            L = {**L, **{k: torch.ones(spec.d) for k in ("qn_g", "kn_g") if L.get(k) is None}}
        yield L


def _plain_vit_config(spec: ViTSpec, n: int, kpad: int):
    return _lib.VitConfig(spec.image_size, spec.patch, spec.d, spec.heads, spec.mlp, n, spec.tokens, int(spec.has_cls), int(spec.pre_ln),
                          _lib.ACT[spec.act], kpad, float(spec.eps), registers=spec.registers, norm=_lib.NORM[spec.norm], qk_norm=int(spec.qk_norm))


class VitEngine(_TowerEngine):
    """One ViT tower on one GPU.

    forward(pixels, n_layers) returns hidden_states[n_layers] as a bf16 tensor [B, tokens, d]
    (index 0 = embeddings (+pre-LN for CLIP), index i = output of encoder layer i — the HF
    `output_hidden_states=True` convention the reference towers index with `select_layer`).
    """

    def __init__(self, spec: ViTSpec, weights: dict, device: Optional[torch.device] = None, fuse_ln: Optional[bool] = None,
                 head_pad: Optional[int] = None, fuse_gate: Optional[bool] = None):
        """head_pad: lanes per head in the device buffers, None = head_pad_for(d / heads) (64 -> 64, 65 .. 96 -> 96, 97 .. 128 -> 128);
        128 for a head of 65 .. 96 is the route attn_fwd96 replaced (attn_fwd<2> on heads padded to 128), kept reachable for A/B runs.
        The MLP width is padded to a multiple of 128 alike (pad_tower_weights).
        RMSNorm towers (spec.norm == "rmsnorm") take the same two routes with visrep_rmsnorm_stats / visrep_rmsnorm; QK-norm towers
        (spec.qk_norm) carry qn_g / kn_g padded per head, the pre-scaled-Q constant on qn_g instead of on the Q rows.
        fuse_ln (default on; VISREP_FUSE_LN=0 turns it off): fold every block's LayerNorm into the GEMMs that consume it -
        gamma into the weight rows, beta into the bias, the per-row mean / rstd into the GEMM epilogue (ln_rt / ln_s) - so the
        normalised activations are never written to HBM, and take the row statistics from the epilogue of the residual GEMM that
        produced the rows (visrep_gemm_bf16_resid_stats) - so LayerNorm never reads the residual stream either; only layer 0's
        first LayerNorm runs the read-only statistics pass.  Measured on ViT-L/14-336, batch 256: the two LayerNorm passes per
        layer (19.7 ms of kernel time per 4 forwards) are replaced by 15.2 ms of heavier epilogues + partial-sum reduction:
        +0.8 % kernel time, +1.4 % on the bench line (profiles/round1_fold_stats.md)."""
        super().__init__(_lib.require_gpu(), spec, device)
        self.fuse_ln = (os.environ.get("VISREP_FUSE_LN", "1") != "0") if fuse_ln is None else bool(fuse_ln)
        # SwiGLU towers (DINOv2-giant): fc1 with the gate in the GEMM epilogue (default; w1 / b1 / s1 in the 16-row interleave) or, with
        # fuse_gate=False / VISREP_FUSE_GATE=0, as a plain GEMM + the element-wise visrep_swiglu pass (A/B baseline, profiles/swiglu.md)
        self.fuse_gate = (os.environ.get("VISREP_FUSE_GATE", "1") != "0") if fuse_gate is None else bool(fuse_gate)
        if spec.d % spec.heads:
            raise ValueError("d must be a multiple of heads")
        self.head_dim = spec.d // spec.heads
        self.head_pad = head_pad_for(self.head_dim) if head_pad is None else int(head_pad)
        if self.head_pad not in (64, 96, 128) or self.head_pad < self.head_dim or (self.head_dim == 64) != (self.head_pad == 64):
            raise ValueError(f"head_pad must be 96 or 128 and >= the head width {self.head_dim} (64-wide heads are not padded)")
        if spec.d % 128:
            raise ValueError("d must be a multiple of 128")
        self.mlp_pad = _round_up(spec.mlp, 128)
        da = spec.heads * self.head_pad
        ensure_scratch(self.device)
        self.kpad = _round_up(3 * spec.patch * spec.patch, 64)
        pw = torch.zeros(spec.d, self.kpad, dtype=torch.float32)
        pw[:, : 3 * spec.patch * spec.patch] = weights["patch_w"].float()
        if weights["pos"].shape[0] != spec.tokens:
            raise ValueError(f"position embedding has {weights['pos'].shape[0]} rows, spec wants {spec.tokens}")
        self.n_layers = n = len(weights["layers"])
        # softmax scale in the exponent's base, folded into the Q rows of the Q|K|V projection (attn_fwd PS): q' = c * q with
        # c = head_dim^-0.5 * log2(e), so that 2^(q'.k) = e^(q.k / sqrt(head_dim)).  VISREP_Q_PRESCALE=0 keeps the scale in the kernel.
        # VISREP_Q_PRESCALE=2 (default) additionally lets towers with a CLS token and 64 n patches run the image-aligned attention kernel.
        # Padded heads (head_pad 96 / 128) keep the scale in the kernel: the pre-scaled variant of the flash kernel is built for width 64 only.
        self._q_mode = int(os.environ.get("VISREP_Q_PRESCALE", "2")) if self.head_pad == 64 else 0
        self.q_prescaled = self._q_mode != 0
        # QK-norm towers (InternViT-6B): a norm behind the projection would undo a constant folded into the Q rows, so it goes into qn_g instead
        qc = torch.ones(3 * da)
        q_const = self.head_dim ** -0.5 * 1.4426950408889634
        if self.q_prescaled and not spec.qk_norm:
            qc[: da] = q_const

        def fold(Wm, bias, g, b, rowscale=None):
            """Linear(LayerNorm(x)) = rstd * (x (g o W)^T - mean * s) + (W b + bias): (g o W in bf16, s over the ROUNDED rows, b').
            rowscale (the Q rows' softmax scale) multiplies the fp32 product before its single rounding to bf16."""
            Wb = Wm.detach().float().to(torch.bfloat16).float()               # the weights the unfused path multiplies with
            rs = torch.ones(Wb.shape[0]) if rowscale is None else rowscale
            Wf = (Wb * g.detach().float()[None] * rs[:, None]).to(torch.bfloat16)
            shift = Wb @ b.detach().float()                                  # beta pushed through the linear map
            return Wf, Wf.float().sum(1), (shift if bias is None else shift + bias.detach().float()) * rs

        def device_layer(L):
            L = pad_tower_weights(spec, L, self.head_pad, self.mlp_pad)       # before the fold: it sees the padded matrices (zero rows: s = 0, b' = 0)
            L["sqkv"] = L["s1"] = None
            if self.fuse_ln:                                                   # RMSNorm blocks: gamma only, no beta term (sqkv / s1 stay finite and meet a zero factor)
                nb = torch.zeros(spec.d) if spec.norm == "rmsnorm" else None
                L["wqkv"], L["sqkv"], L["bqkv"] = fold(L["wqkv"], L.get("bqkv"), L["ln1_g"], L["ln1_b"] if nb is None else nb, qc)
                L["w1"], L["s1"], L["b1"] = fold(L["w1"], L.get("b1"), L["ln2_g"], L["ln2_b"] if nb is None else nb)
            elif self.q_prescaled and not spec.qk_norm:                        # unfused path: scale the (bf16-rounded) rows, round once more
                L["wqkv"] = L["wqkv"].detach().float().to(torch.bfloat16).float() * qc[:, None]
                if L.get("bqkv") is not None:
                    L["bqkv"] = L["bqkv"].detach().float() * qc
            if spec.act == "swiglu" and self.fuse_gate:                        # after the fold (per row): w1, b1 and s1 move together
                idx = swiglu_interleave_index(self.mlp_pad)
                for k in ("w1", "b1", "s1"):
                    if L.get(k) is not None:
                        L[k] = L[k][idx]
            if spec.qk_norm:                                                   # fp32 gains, padded per head; the pre-scaled-Q constant rides on qn_g
                L["qn_g"] = pad_qk_gain(spec, L.get("qn_g"), self.head_pad) * (q_const if self.q_prescaled else 1.0)
                L["kn_g"] = pad_qk_gain(spec, L.get("kn_g"), self.head_pad)
            return L

        _fill_vit_tables(self, pw, _vit_vector_table(spec, weights), map(device_layer, weights["layers"]), torch.bfloat16)
        self._cfg = _lib.VitConfig(spec.image_size, spec.patch, spec.d, spec.heads, self.mlp_pad, n, spec.tokens,
                                   int(spec.has_cls), int(spec.pre_ln), _lib.ACT[spec.act], self.kpad, float(spec.eps), self._q_mode,
                                   self.head_dim, self.head_pad, spec.registers, _lib.NORM[spec.norm], int(spec.qk_norm))

    def _workspace_bytes(self, B: int) -> int:
        old_knob = self.lib.visrep_set_fuse_gate(int(self.fuse_gate))              # the unfused SwiGLU route keeps a wider MLP buffer
        nbytes = self.lib.visrep_vit_workspace_bytes(C.byref(self._cfg), B)
        self.lib.visrep_set_fuse_gate(old_knob)
        return nbytes

    @torch.no_grad()
    def forward(self, pixels: torch.Tensor, n_layers: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        s = self.spec
        px = self._pixels(pixels)
        n_layers = self._state(n_layers, "n_layers out of range")
        B = px.shape[0]
        if out is None:
            out = torch.empty(B, s.tokens, s.d, dtype=torch.bfloat16, device=self.device)
        ws = self.workspace(B)
        with torch.cuda.device(self.device):
            old_knob = self.lib.visrep_set_fuse_gate(int(self.fuse_gate))          # per-thread, host side: which fc1 route this engine's weights are packed for
            rc = self.lib.visrep_vit_forward(C.byref(self._cfg), C.byref(self._w), _lib.ptr(px),
                                             _lib.F32 if px.dtype == torch.float32 else _lib.BF16,
                                             _lib.ptr(out), B, n_layers, _lib.ptr(ws), _lib.stream_ptr())
            self.lib.visrep_set_fuse_gate(old_knob)
        _lib.check(rc, "visrep_vit_forward")
        return out


class VitEngineF32(_TowerEngine):
    """The same tower in reference precision: fp32 weights, activations and accumulation (csrc/f32ops.hip, visrep_vit_forward_f32).

    The reference's C-score CLIP / OpenCLIP / DINOv2 towers run in fp32 (C_score/extract_feature.py:36-45,49-50: no dtype cast,
    fp32 pixels); this engine is what makes images -> tower -> A / C score comparable with that chain at the 1e-4 bar.  About
    1/6 of the bf16 engine's throughput on the split-bf16 route (1/10 on the exact-fp32 MFMA route, which takes any head width that is a
    multiple of 4).
    forward() returns fp32 [B, tokens, d]; images are processed in chunks so that the fp32 score matrices stay below `max_ws_bytes`."""

    WS_ZERO = False
    PIXEL_DTYPES = (torch.float32,)

    def __init__(self, spec: ViTSpec, weights: dict, device: Optional[torch.device] = None, max_ws_bytes: int = 8 << 30, gemm: str = "auto",
                 products: Optional[int] = None):
        """gemm: 'split' = projections and attention as split-bf16 products on the bf16 matrix pipe (fp32 values as bf16 planes, fp32
        accumulation, visrep_vit_forward_f32_split); 'native' = exact-fp32 MFMA (visrep_vit_forward_f32); 'auto' = split where the tower's
        shapes allow it (d, mlp % 256 == 0, head width 64), VISREP_F32_GEMM in the environment overrides.
        products (split route): 6 = three planes, every plane pair >= 2^-24 of the result (fp32-equivalent, ~1e-7 per product sum);
        4 / 3 = two planes (16 significand bits), all four pairs / without (mid, mid): ~4e-6 per product sum at half the matrix work.
        None = DEFAULT_SPLIT_PRODUCTS = 6, the fp32-equivalent set (3 holds A <= 1e-4 and exact PCK hits on the full-size SYNTHETIC towers,
        profiles/round4_precision.md, and is the sweep's explicit opt-in); VISREP_F32_PRODUCTS in the environment overrides."""
        super().__init__(_lib.require_gpu(), spec, device)
        if spec.d % spec.heads or (spec.d // spec.heads) % 4 or spec.mlp % 4:
            raise ValueError("fp32 engine: d / heads and mlp must be multiples of 4")
        self.kpad = _round_up(3 * spec.patch * spec.patch, 4)
        self.max_ws_bytes = int(max_ws_bytes)
        pw = torch.zeros(spec.d, self.kpad, dtype=torch.float32)
        pw[:, : 3 * spec.patch * spec.patch] = weights["patch_w"].float()
        if weights["pos"].shape[0] != spec.tokens:
            raise ValueError(f"position embedding has {weights['pos'].shape[0]} rows, spec wants {spec.tokens}")
        self.n_layers = n = len(weights["layers"])
        held = _fill_vit_tables(self, pw, _vit_vector_table(spec, weights), _raw_vit_layers(spec, weights))
        self._cfg = _plain_vit_config(spec, n, self.kpad)
        gemm = os.environ.get("VISREP_F32_GEMM", gemm)
        if gemm not in ("auto", "split", "native"):
            raise ValueError(f"gemm must be 'auto', 'split' or 'native', got {gemm!r}")
        can = bool(self.lib.visrep_vit_f32_split_supported(C.byref(self._cfg)))
        if gemm == "split" and not can:
            raise ValueError("split-bf16 route needs d and mlp to be multiples of 256, head width 64 and LayerNorm blocks without QK norm")
        self.gemm = "split" if (gemm != "native" and can) else "native"
        products = int(os.environ.get("VISREP_F32_PRODUCTS", products if products is not None else DEFAULT_SPLIT_PRODUCTS))
        if products not in (3, 4, 6):
            raise ValueError(f"products must be 3, 4 or 6, got {products}")
        self.products = products if self.gemm == "split" else None
        self._wsplit = None
        if self.gemm == "split":
            npl = split_planes(products)
            # the four projection matrices of every layer as bf16 planes [N, npl K] (hi | mid [| lo]), split on the device once
            self._split_layers = (_lib.VitLayer * max(n, 1))()
            with torch.cuda.device(self.device):
                for i in range(n):
                    for k in ("wqkv", "wo", "w1", "w2"):
                        wf = held[i][k]
                        planes = torch.empty(wf.shape[0], npl * wf.shape[1], dtype=torch.bfloat16, device=self.device)
                        _lib.check(self.lib.visrep_split_bf16_planes(_lib.ptr(wf), wf.stride(0), wf.shape[0], wf.shape[1], npl, _lib.ptr(planes),
                                                                     _lib.stream_ptr()), "visrep_split_bf16_planes")
                        self._keep.append(planes)
                        setattr(self._split_layers[i], k, planes.data_ptr())
            self._wsplit = _lib.VitWeights()
            self._wsplit.layers = C.cast(self._split_layers, C.POINTER(_lib.VitLayer))

    def chunk(self) -> int:
        """Images per library call.  Bounded by the workspace budget, then picked for the GEMMs' tile rounds (best_chunk): the persistent
        256 x 256 kernel runs floor(tiles / CUs) rounds + a tail launch for a remainder of up to CUs / 4 tiles (else one more round), and the
        N = d projections have the fewest tiles per row block - 64 images of a 577-token tower are 2.25 rounds of them (3 run), 113 images
        3.98 (4 run)."""
        per = self.lib.visrep_vit_f32_workspace_bytes(C.byref(self._cfg), 1)
        cap = max(1, min(128, self.max_ws_bytes // max(per, 1)))
        forced = int(os.environ.get("VISREP_F32_CHUNK", "0"))              # A/B knob (tools/)
        return min(forced, cap) if forced > 0 else best_chunk(self.spec.tokens, self.spec.d, cap)

    def _workspace_bytes(self, B: int) -> int:
        return self.lib.visrep_vit_f32_workspace_bytes(C.byref(self._cfg), B)

    @torch.no_grad()
    def forward(self, pixels: torch.Tensor, n_layers: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        s = self.spec
        px = self._pixels(pixels)
        n_layers = self._state(n_layers, "n_layers out of range")
        B = px.shape[0]
        if out is None:
            out = torch.empty(B, s.tokens, s.d, dtype=torch.float32, device=self.device)
        step = self.chunk()
        with torch.cuda.device(self.device):
            for b0 in range(0, B, step):
                nb = min(step, B - b0)
                ws = self.workspace(nb)
                if self.gemm == "split":
                    rc = self.lib.visrep_vit_forward_f32_split(C.byref(self._cfg), C.byref(self._w), C.byref(self._wsplit), self.products,
                                                               _lib.ptr(px[b0:b0 + nb]), _lib.ptr(out[b0:b0 + nb]), nb, n_layers, _lib.ptr(ws),
                                                               _lib.stream_ptr())
                else:
                    rc = self.lib.visrep_vit_forward_f32(C.byref(self._cfg), C.byref(self._w), _lib.ptr(px[b0:b0 + nb]), _lib.ptr(out[b0:b0 + nb]),
                                                         nb, n_layers, _lib.ptr(ws), _lib.stream_ptr())
                _lib.check(rc, "visrep_vit_forward_f32")
        return out


def best_chunk(tokens: int, d: int, cap: int, cus: Optional[int] = None) -> int:
    """Images per launch (<= cap, >= cap / 2) for which a [count * tokens, d] GEMM wastes the least of the persistent 256 x 256 kernel's tile
    rounds.  The cost model is the GEMM dispatcher's own rule (csrc/gemm_bf16.hip, visrep_gemm_dispatch): T tiles on `cus` CUs run as
    floor(T / cus) full rounds; a remainder goes to the 128 x 128 tail launch when 0 < 4 * rem <= cus and the full rounds end on a row
    boundary - priced here at 0.45 of a round plus twice its share of one (profiles/round4_gemm.md section 5: a tail pair of launches is
    14-18 us beside a 31-us K = 1024 round, and that kernel runs at about half the rate) - and costs a whole extra round otherwise.
    Returns the LARGEST count whose efficiency (tiles / (cus * rounds paid)) is within 1 % of the best in the range.
    cus = None asks the library for the current device's CU count (visrep_device_cu_count; 256 when no device is visible).  On MI355X:
    best_chunk(577, 1024, 128) = 113 (3.98 rounds, 4 paid), best_chunk(257, 1024, 128) = 127 (exactly 2 rounds, no tail launch)."""
    if cus is None:
        cus = 256                                               # no device visible (host-side planning / tests): the MI355X count
        if torch.cuda.is_available():
            cus = int(_lib.load().visrep_device_cu_count())
    ntn = max(1, d // 256)

    def eff(c):
        tiles = -(-c * tokens // 256) * ntn
        rounds, rem = divmod(tiles, cus)
        if rem == 0:
            paid = rounds
        elif rounds >= 1 and rem * 4 <= cus and (rounds * cus) % ntn == 0:
            paid = rounds + 0.45 + 2.0 * rem / cus
        else:
            paid = rounds + 1
        return tiles / (cus * paid)
    lo = max(cap // 2, 1)
    effs = {c: eff(c) for c in range(lo, cap + 1)}
    top = max(effs.values())
    return max(c for c, e in effs.items() if e >= top - 0.01)


class VitEngineCPU(_TowerEngine):
    """The same tower on HOST cores (visrep_vit_forward_cpu, csrc/host_twins.hip): plain C++ fp32 on host threads.  BASELINE configs[0]
    ("vision_tower feature-extract on 32 COCO images, CPU float32 - plumbing, no GPU") and SURVEY §8b's `*_cpu` twins.  Built ONLY when the
    caller asks for device "cpu" explicitly (make_engine(..., device="cpu"); a tower config with device="cpu") - the GPU engines never fall
    back to it.  forward() takes and returns CPU fp32 tensors."""

    PIXEL_DTYPES = (torch.float32,)

    def __init__(self, spec: ViTSpec, weights: dict, threads: Optional[int] = None):
        super().__init__(_lib.load(), spec, "cpu")
        self.threads = int(threads) if threads else 0
        if weights["pos"].shape[0] != spec.tokens:
            raise ValueError(f"position embedding has {weights['pos'].shape[0]} rows, spec wants {spec.tokens}")
        self.kpad = 3 * spec.patch * spec.patch
        self.n_layers = n = len(weights["layers"])
        _fill_vit_tables(self, weights["patch_w"].reshape(spec.d, -1)[:, : self.kpad], _vit_vector_table(spec, weights), _raw_vit_layers(spec, weights))
        self._cfg = _plain_vit_config(spec, n, self.kpad)

    @torch.no_grad()
    def forward(self, pixels: torch.Tensor, n_layers: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        s = self.spec
        px = self._pixels(pixels)
        n_layers = self._state(n_layers, "n_layers out of range")
        B = px.shape[0]
        if out is None:
            out = torch.empty(B, s.tokens, s.d, dtype=torch.float32)
        rc = self.lib.visrep_vit_forward_cpu(C.byref(self._cfg), C.byref(self._w), _lib.ptr(px), _lib.ptr(out), B, n_layers, self.threads)
        _lib.check(rc, "visrep_vit_forward_cpu")
        return out


def make_engine(spec: ViTSpec, weights: dict, device=None, precision: str = "bf16", products: Optional[int] = None):
    """precision 'bf16' = the MFMA throughput engine; 'fp32' = the reference-precision engine (products: its split-bf16 product set,
    None = DEFAULT_SPLIT_PRODUCTS).  device "cpu" - and only an explicit "cpu" - builds the host twin (fp32, whatever `precision` says)."""
    if device is not None and torch.device(device).type == "cpu":
        return VitEngineCPU(spec, weights)
    if precision in ("bf16", torch.bfloat16):
        return VitEngine(spec, weights, device)
    if precision in ("fp32", "float32", torch.float32):
        return VitEngineF32(spec, weights, device, products=products)
    raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")


# Plane-pair products of the split-bf16 route (VitEngineF32; see its __init__).  The DEFAULT is the fp32-EQUIVALENT set: six products over
# three-plane operands (24 significand bits per operand, every dropped term < 2^-24 of the result) - what a drop-in for the reference's fp32
# towers (C_score/extract_feature.py:36-45) has to be on checkpoints nobody has validated a cheaper set on.  3 = (hi,hi) (hi,mid) (mid,hi)
# over two-plane operands (16 significand bits, the mid x mid term dropped) is an explicit OPT-IN for throughput runs (the sweep passes
# tower_products=3 and says so in its dtype field): measured at full size on SYNTHETIC N(0, 0.02) weights (profiles/round4_precision.md) -
# CLIP-L/14-336 features 8.6e-6 rel-L2 of the fp32 oracle (six products: 2.5e-6, the bf16 engine: 1.2e-2), A score 1e-7 relative, 0 of 2,400
# PCK hits flipped - at 1.8x the six-product tower's rate; real checkpoints with massive-activation outlier channels were never available
# offline, which is why it is not the default.
DEFAULT_SPLIT_PRODUCTS = 6
THROUGHPUT_SPLIT_PRODUCTS = 3


def split_planes(products: int) -> int:
    """bf16 planes per fp32 value a product set reads: three for the six-product (fp32-equivalent) set, two for 3 / 4 products."""
    return 3 if products == 6 else 2


def split_bf16_planes(x: torch.Tensor, nplanes: int = 3) -> torch.Tensor:
    """fp32 [rows, K] -> bf16 planes [rows, nplanes K] = hi | mid [| lo] (x = hi + mid + lo to 24 bits; hi + mid to 16): the operand format
    of gemm_f32_split."""
    lib = _lib.require_gpu()
    rows, K = x.shape
    planes = torch.empty(rows, nplanes * K, dtype=torch.bfloat16, device=x.device)
    _lib.check(lib.visrep_split_bf16_planes(_lib.ptr(x), x.stride(0), rows, K, nplanes, _lib.ptr(planes), _lib.stream_ptr()), "visrep_split_bf16_planes")
    return planes


def split_bf16x3(x: torch.Tensor) -> torch.Tensor:
    return split_bf16_planes(x, 3)


def gemm_f32_split(a_planes: torch.Tensor, w_planes: torch.Tensor, bias: Optional[torch.Tensor] = None, act: str = "none",
                   resid: Optional[torch.Tensor] = None, ls: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                   planes_out: bool = False, products: int = 6):
    """fp32 act(A W^T + bias) (+ LayerScale, residual) on the bf16 matrix pipe from bf16 planes (split_bf16_planes with
    split_planes(products) planes); returns the fp32 result, or its own planes [M, npl N] when planes_out."""
    lib = _lib.require_gpu()
    npl = split_planes(products)
    M, Kp = a_planes.shape
    N, K = w_planes.shape[0], Kp // npl
    if w_planes.shape[1] != Kp or Kp % npl:
        raise ValueError("gemm_f32_split: operand plane widths differ")
    po = torch.empty(M, npl * N, dtype=torch.bfloat16, device=a_planes.device) if planes_out else None
    if out is None and not planes_out:
        out = torch.empty(M, N, dtype=torch.float32, device=a_planes.device)
    rc = lib.visrep_gemm_f32_split(_lib.ptr(a_planes), _lib.ptr(w_planes), M, N, K, products, _lib.ptr(bias), _lib.ACT[act], _lib.ptr(resid),
                                   _lib.ptr(ls), _lib.ptr(out), out.stride(0) if out is not None else N, _lib.ptr(po), _lib.stream_ptr())
    _lib.check(rc, "visrep_gemm_f32_split")
    return po if planes_out else out


def gemm_f32(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = _lib.EPI_BIAS, act: str = "none",
             resid: Optional[torch.Tensor] = None, ls: Optional[torch.Tensor] = None, w_kn: bool = False, alpha: float = 1.0,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 C = epilogue(alpha * A @ W^T + bias) (w_kn: A @ W) on the exact-fp32 MFMA path."""
    lib = _lib.require_gpu()
    M, K = a.shape
    N = w.shape[1] if w_kn else w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    rc = lib.visrep_gemm_f32(_lib.ptr(a), a.stride(0), _lib.ptr(w), w.stride(0), int(w_kn), _lib.ptr(bias), _lib.ptr(out), out.stride(0), M, N, K,
                             epilogue, _lib.ACT[act], _lib.ptr(resid), _lib.ptr(ls), float(alpha), 1, 1, None, _lib.stream_ptr())
    _lib.check(rc, "visrep_gemm_f32")
    return out


# ------------------------------------------------------------------------------------------------ thin op wrappers
def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = _lib.EPI_BIAS,
         act: str = "none", resid: Optional[torch.Tensor] = None, ls: Optional[torch.Tensor] = None,
         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C = epilogue(A @ W^T): A [M,K] bf16, W [N,K] bf16 (nn.Linear layout), fp32 bias/ls.  EPI_VT is exposed via linear_vt()."""
    lib = _lib.require_gpu()
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32 if epilogue == _lib.EPI_F32 else torch.bfloat16, device=a.device)
    rc = lib.visrep_gemm_bf16(_lib.ptr(a), a.stride(0), _lib.ptr(w), w.stride(0), _lib.ptr(bias), _lib.ptr(out), out.stride(0),
                              M, N, K, epilogue, _lib.ACT[act], _lib.ptr(resid), _lib.ptr(ls), _lib.stream_ptr())
    _lib.check(rc, "visrep_gemm_bf16")
    return out


def gemm_gated(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, ln_rt: Optional[torch.Tensor] = None,
               ln_s: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SwiGLU GEMM (visrep_gemm_bf16_gated): a [M, K] bf16, w [2 mp, K] bf16 with gate / value rows interleaved in blocks of 16
    (swiglu_interleave_index), bias / ln_s [2 mp] in the same order -> [M, mp] bf16 = silu(gate) * value.  `out` may be a column window."""
    lib = _lib.require_gpu()
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N // 2, dtype=torch.bfloat16, device=a.device)
    rc = lib.visrep_gemm_bf16_gated(_lib.ptr(a), a.stride(0), _lib.ptr(w), w.stride(0), _lib.ptr(bias), _lib.ptr(ln_rt), _lib.ptr(ln_s),
                                    _lib.ptr(out), out.stride(0), M, N, K, _lib.stream_ptr())
    _lib.check(rc, "visrep_gemm_bf16_gated")
    return out


def swiglu(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """silu(x[:, :F]) * x[:, F:] (HF chunk order) for bf16 or fp32 x [M, 2 F] (visrep_swiglu / visrep_swiglu_f32)."""
    lib = _lib.require_gpu()
    M, F = x.shape[0], x.shape[1] // 2
    if out is None:
        out = torch.empty(M, F, dtype=x.dtype, device=x.device)
    fn = lib.visrep_swiglu_f32 if x.dtype == torch.float32 else lib.visrep_swiglu
    _lib.check(fn(_lib.ptr(x), x.stride(0), _lib.ptr(out), out.stride(0), M, F, _lib.stream_ptr()), "visrep_swiglu")
    return out


def linear_vt(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: Optional[torch.Tensor] = None,
              col_offset: int = 0) -> torch.Tensor:
    """V projection in the attention kernel's V^T layout: returns [N, ldvt] bf16 (see csrc/attention.hip).

    out / col_offset: write the tokens of `a` as columns [col_offset, col_offset + M) of an existing (zero-initialised) V^T
    buffer - how a joint key sequence is assembled from several token groups (SD3: image tokens, then prompt tokens);
    col_offset must be a multiple of 16 (the perm16 granule)."""
    lib = _lib.require_gpu()
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        ldvt = _round_up(M, 64) + 64
        out = torch.zeros(N, ldvt, dtype=torch.bfloat16, device=a.device)
    if col_offset % 16 or col_offset + M > out.shape[1]:
        raise ValueError("linear_vt: col_offset must be a multiple of 16 and fit the buffer")
    rc = lib.visrep_gemm_bf16(_lib.ptr(a), a.stride(0), _lib.ptr(w), w.stride(0), _lib.ptr(bias), C.c_void_p(out.data_ptr() + 2 * col_offset),
                              out.stride(0), M, N, K, _lib.EPI_VT, 0, None, None, _lib.stream_ptr())
    _lib.check(rc, "visrep_gemm_bf16(VT)")
    return out


def gemm_rows(a: torch.Tensor, period: int, stride: int, first: int, rows: int, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
              epilogue: int = _lib.EPI_BIAS, act: str = "none", ln_rt: Optional[torch.Tensor] = None, ln_s: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GEMM over a periodic subset of a's rows (visrep_gemm_bf16_rows): logical row r = physical (r // period) * stride + r % period + first.
    EPI_VT returns / fills a V^T buffer [N, ld] (columns = logical rows, perm16), the others [rows, N]."""
    lib = _lib.require_gpu()
    N, K = w.shape[0], a.shape[1]
    if (rows - 1) // period * stride + (rows - 1) % period + first >= a.shape[0]:
        raise ValueError("gemm_rows: the row map reaches past a")
    if out is None:
        if epilogue == _lib.EPI_VT:
            out = torch.zeros(N, _round_up(rows, 64) + 64, dtype=torch.bfloat16, device=a.device)
        else:
            out = torch.empty(rows, N, dtype=torch.float32 if epilogue == _lib.EPI_F32 else torch.bfloat16, device=a.device)
    rc = lib.visrep_gemm_bf16_rows(_lib.ptr(a), a.stride(0), period, stride, first, _lib.ptr(w), w.stride(0), _lib.ptr(bias), _lib.ptr(ln_rt),
                                   _lib.ptr(ln_s), _lib.ptr(out), out.stride(0), rows, N, K, epilogue, _lib.ACT[act], _lib.stream_ptr())
    _lib.check(rc, "visrep_gemm_bf16_rows")
    return out


def layernorm(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float) -> torch.Tensor:
    lib = _lib.require_gpu()
    y = torch.empty_like(x)
    rc = lib.visrep_layernorm(_lib.ptr(x), x.stride(0), _lib.ptr(g), _lib.ptr(b), _lib.ptr(y), y.stride(0), x.shape[0], x.shape[1],
                              eps, _lib.stream_ptr())
    _lib.check(rc, "visrep_layernorm")
    return y


def mhsa(qk: torch.Tensor, vt: torch.Tensor, B: int, T: int, H: int, scale: float, head_dim: int = 64) -> torch.Tensor:
    """qk [B T, 2 H head_dim] (Q | K), vt [H head_dim, ldvt]; head_dim = the padded width of the buffers (64, 96 or 128)."""
    lib = _lib.require_gpu()
    out = torch.empty(B * T, H * head_dim, dtype=torch.bfloat16, device=qk.device)
    rc = lib.visrep_mhsa_fwd(_lib.ptr(qk), qk.stride(0), _lib.ptr(vt), vt.stride(0), _lib.ptr(out), out.stride(0), B, T, H, head_dim,
                             scale, _lib.stream_ptr())
    _lib.check(rc, "visrep_mhsa_fwd")
    return out


def mhsa_cls_supported(T: int) -> bool:
    return bool(_lib.load().visrep_mhsa_cls_supported(int(T)))


def mhsa_cls(qk: torch.Tensor, vt: torch.Tensor, vcls: torch.Tensor, B: int, T: int, H: int) -> torch.Tensor:
    """Image-aligned self-attention (visrep_mhsa_cls_fwd): qk [B T, 2 H 64] with pre-scaled Q; vt = V^T of the patch tokens (column
    b (T - 1) + t - 1, as linear_vt over the patch rows writes it); vcls = V rows of the CLS tokens [B, H 64]."""
    lib = _lib.require_gpu()
    out = torch.empty(B * T, H * 64, dtype=torch.bfloat16, device=qk.device)
    rc = lib.visrep_mhsa_cls_fwd(_lib.ptr(qk), qk.stride(0), _lib.ptr(vt), vt.stride(0), _lib.ptr(vcls), vcls.stride(0), _lib.ptr(out),
                                 out.stride(0), B, T, H, 64, _lib.stream_ptr())
    _lib.check(rc, "visrep_mhsa_cls_fwd")
    return out


def mhsa_prefix_supported(T: int, prefix: int) -> bool:
    return bool(_lib.load().visrep_mhsa_prefix_supported(int(T), int(prefix)))


def mhsa_prefix(qk: torch.Tensor, vt: torch.Tensor, vpre: torch.Tensor, B: int, T: int, prefix: int, H: int) -> torch.Tensor:
    """Image-aligned self-attention with `prefix` side keys per image (visrep_mhsa_prefix_fwd): qk [B T, 2 H 64] with pre-scaled Q; vt = V^T of
    the patch tokens (column b (T - prefix) + t - prefix); vpre = V rows of the prefix tokens [B prefix, H 64]."""
    lib = _lib.require_gpu()
    out = torch.empty(B * T, H * 64, dtype=torch.bfloat16, device=qk.device)
    rc = lib.visrep_mhsa_prefix_fwd(_lib.ptr(qk), qk.stride(0), _lib.ptr(vt), vt.stride(0), _lib.ptr(vpre), vpre.stride(0), _lib.ptr(out),
                                    out.stride(0), B, T, prefix, H, 64, _lib.stream_ptr())
    _lib.check(rc, "visrep_mhsa_prefix_fwd")
    return out


# ------------------------------------------------------------------------------------------------ ConvNeXt
class ConvNextEngine(_TowerEngine):
    """One ConvNeXt tower on one GPU (visrep_convnext_forward): forward(pixels, n_stages) returns hidden_states[n_stages] of HF ConvNextModel as
    bf16 token rows [B, H_s W_s, C_s] - index 0 = the stem output, 1 .. 4 = the stage outputs.  bf16 on the GPU only: there is no fp32 and no
    host ConvNeXt engine, and asking for one is an error, never a fallback."""

    def __init__(self, spec, weights: dict, device: Optional[torch.device] = None):
        from . import convnext_weights as CW
        if device is not None and torch.device(device).type == "cpu":
            raise ValueError("ConvNeXt towers have no host engine (device='cpu'): only the bf16 HIP engine exists")
        super().__init__(_lib.require_gpu(), spec, device)
        self.n_layers = 4                                  # the tower protocol's name for "last hidden-state index"
        ensure_scratch(self.device)

        def dev(t):
            return _addr(self._hold(t))

        D = CW.device_layout(spec, weights)
        nblk = sum(spec.depths)
        self._blocks = (_lib.ConvNextBlock * nblk)()
        self._w = _lib.ConvNextWeights()
        for k in ("stem_w", "stem_b", "stem_ln_g", "stem_ln_b"):
            setattr(self._w, k, dev(D[k]))
        i = 0
        for st, stage in enumerate(D["stages"]):
            if len(stage["blocks"]) != spec.depths[st]:
                raise ValueError(f"stage {st} has {len(stage['blocks'])} blocks, spec wants {spec.depths[st]}")
            for k in ("ds_ln_g", "ds_ln_b", "ds_w", "ds_b"):
                getattr(self._w, k)[st] = dev(stage[k])
            for L in stage["blocks"]:
                for k in ("dw_w", "dw_b", "w1", "b1", "s1", "w2", "b2", "ls"):
                    setattr(self._blocks[i], k, dev(L[k]))
                i += 1
        self._w.blocks = C.cast(self._blocks, C.POINTER(_lib.ConvNextBlock))
        self._cfg = _lib.ConvNextConfig(spec.image_size, 64, (C.c_int * 4)(*spec.depths), (C.c_int * 4)(*spec.hidden_sizes), float(spec.eps))

    def _workspace_bytes(self, B: int) -> int:
        nbytes = self.lib.visrep_convnext_workspace_bytes(C.byref(self._cfg), B)
        if nbytes == 0:
            raise RuntimeError(f"visrep_convnext_workspace_bytes refused the tower: {_lib.last_error()}")
        return nbytes

    @torch.no_grad()
    def forward(self, pixels: torch.Tensor, n_stages: Optional[int] = None, out: Optional[torch.Tensor] = None, n_layers: Optional[int] = None) -> torch.Tensor:
        s = self.spec
        px = self._pixels(pixels)
        n_stages = self._state(n_layers if n_stages is None else n_stages, "n_stages out of range (0 = stem output, 1 .. 4 = stage outputs)")
        B = px.shape[0]
        if out is None:
            out = torch.empty(B, s.grid(n_stages) ** 2, s.width(n_stages), dtype=torch.bfloat16, device=self.device)
        ws = self.workspace(B)
        with torch.cuda.device(self.device):
            rc = self.lib.visrep_convnext_forward(C.byref(self._cfg), C.byref(self._w), _lib.ptr(px), _lib.F32 if px.dtype == torch.float32 else _lib.BF16,
                                                  _lib.ptr(out), B, n_stages, _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, "visrep_convnext_forward")
        return out


def make_convnext_engine(spec, weights: dict, device=None, precision: str = "bf16") -> ConvNextEngine:
    """make_engine for ConvNeXt towers: bf16 on the GPU, and a ValueError that says so for anything else."""
    if precision not in ("bf16", "bfloat16"):
        raise ValueError(f"ConvNeXt towers run in bf16 only: there is no {precision} ConvNeXt engine (a full fp32 engine is out of scope)")
    return ConvNextEngine(spec, weights, device)


def dwconv7x7_stats(x: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor, C: Optional[int] = None, eps: float = 1e-6):
    """x [B, H, W, ldx] bf16 (the first C columns are the channels) -> (y [B, H, W, C] bf16, rt [B H W, 2] fp32) - visrep_dwconv7x7_stats."""
    lib = _lib.require_gpu()
    B, H, W, ldx = x.shape
    C = ldx if C is None else C
    rows = B * H * W
    y = torch.empty(B, H, W, C, dtype=torch.bfloat16, device=x.device)
    part = torch.empty(max(rows, 1) * max(C // 64, 1), 2, dtype=torch.float32, device=x.device)
    rt = torch.zeros(_round_up(rows, 128) + 8, 2, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.visrep_dwconv7x7_stats(_lib.ptr(x), ldx, _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(y), C, _lib.ptr(part), _lib.ptr(rt), B, H, W, C,
                                              float(eps), _lib.stream_ptr()), "visrep_dwconv7x7_stats")
    return y, rt[:rows]


def ln_space_to_depth2(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, C: Optional[int] = None, eps: float = 1e-6) -> torch.Tensor:
    """x [B, H, W, ldx] bf16 -> [B (H/2) (W/2), 4 C] bf16 - visrep_ln_space_to_depth2."""
    lib = _lib.require_gpu()
    B, H, W, ldx = x.shape
    C = ldx if C is None else C
    out = torch.empty(B * (H // 2) * (W // 2), 4 * C, dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.visrep_ln_space_to_depth2(_lib.ptr(x), ldx, _lib.ptr(g), _lib.ptr(b), _lib.ptr(out), 4 * C, B, H, W, C, float(eps),
                                                 _lib.stream_ptr()), "visrep_ln_space_to_depth2")
    return out


def dwconv7x7_stats_cpu(x: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor, C: Optional[int] = None, eps: float = 1e-6, threads: int = 0):
    """Host twin of dwconv7x7_stats (HOST bf16 tensors; no GPU needed)."""
    lib = _lib.load()
    B, H, W, ldx = x.shape
    C = ldx if C is None else C
    x, wt, bias = x.contiguous(), wt.float().contiguous(), bias.float().contiguous()
    y = torch.empty(B, H, W, C, dtype=torch.bfloat16)
    rt = torch.zeros(B * H * W, 2, dtype=torch.float32)
    _lib.check(lib.visrep_dwconv7x7_stats_cpu(_lib.ptr(x), ldx, _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(y), C, _lib.ptr(rt), B, H, W, C, float(eps), threads),
               "visrep_dwconv7x7_stats_cpu")
    return y, rt


def ln_space_to_depth2_cpu(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, C: Optional[int] = None, eps: float = 1e-6, threads: int = 0) -> torch.Tensor:
    lib = _lib.load()
    B, H, W, ldx = x.shape
    C = ldx if C is None else C
    x, g, b = x.contiguous(), g.float().contiguous(), b.float().contiguous()
    out = torch.empty(B * (H // 2) * (W // 2), 4 * C, dtype=torch.bfloat16)
    _lib.check(lib.visrep_ln_space_to_depth2_cpu(_lib.ptr(x), ldx, _lib.ptr(g), _lib.ptr(b), _lib.ptr(out), 4 * C, B, H, W, C, float(eps), threads),
               "visrep_ln_space_to_depth2_cpu")
    return out


# ------------------------------------------------------------------------------------------------ SAM ViT
class SamEngine(_TowerEngine):
    """One SAM ViT tower on one GPU (visrep_sam_forward): forward(pixels, n_state) returns state n_state of HF SamVisionModel as bf16 token
    rows - 0 = patch embedding + positions, 1 .. L = the block outputs [B, g g, d], L + 1 = the neck output [B, g g, out_channels] - and stops
    after it.  bf16 on the GPU only: there is no fp32 and no host SAM engine, and asking for one is an error, never a fallback."""

    WS_KEEP = 0                                            # the workspaces are the large ones: one unpinned batch size at a time

    def __init__(self, spec, weights: dict, device: Optional[torch.device] = None):
        from . import sam_weights as SW
        if device is not None and torch.device(device).type == "cpu":
            raise ValueError("SAM towers have no host engine (device='cpu'): only the bf16 HIP engine exists")
        super().__init__(_lib.require_gpu(), spec, device)
        self.n_layers = spec.layers + 1                    # the tower protocol's name for "last hidden-state index"
        self.kpad = _round_up(3 * spec.patch * spec.patch, 64)
        ensure_scratch(self.device)

        def dev(t):
            return _addr(self._hold(t))

        if len(weights["layers"]) != spec.layers:
            raise ValueError(f"weights have {len(weights['layers'])} layers, spec wants {spec.layers}")
        D = SW.device_layout(spec, weights, self.kpad)
        self._layers = (_lib.SamLayer * spec.layers)()
        for i, L in enumerate(D["layers"]):
            for k, _ in _lib.SamLayer._fields_:
                setattr(self._layers[i], k, dev(L[k]))
        self._w = _lib.SamWeights()
        for k, _ in _lib.SamWeights._fields_[:-1]:
            setattr(self._w, k, dev(D[k]))
        self._w.layers = C.cast(self._layers, C.POINTER(_lib.SamLayer))
        mask = 0
        for i in spec.global_attn_indexes:
            mask |= 1 << i
        self._cfg = _lib.SamConfig(spec.image_size, spec.patch, spec.d, spec.layers, spec.heads, spec.mlp, spec.window, spec.out_channels, self.kpad,
                                   mask, float(spec.eps), 1e-6)

    def _workspace_bytes(self, B: int) -> int:
        nbytes = self.lib.visrep_sam_workspace_bytes(C.byref(self._cfg), B)
        if nbytes == 0:
            raise RuntimeError(f"visrep_sam_workspace_bytes refused the tower: {_lib.last_error()}")
        return nbytes

    @torch.no_grad()
    def forward(self, pixels: torch.Tensor, n_state: Optional[int] = None, out: Optional[torch.Tensor] = None, n_layers: Optional[int] = None) -> torch.Tensor:
        s = self.spec
        px = self._pixels(pixels)
        n_state = self._state(n_layers if n_state is None else n_state,
                              f"n_state out of range (0 = embeddings, 1 .. {s.layers} = blocks, {s.layers + 1} = the neck)")
        B = px.shape[0]
        if out is None:
            out = torch.empty(B, s.grid ** 2, s.width(n_state), dtype=torch.bfloat16, device=self.device)
        ws = self.workspace(B)
        with torch.cuda.device(self.device):
            rc = self.lib.visrep_sam_forward(C.byref(self._cfg), C.byref(self._w), _lib.ptr(px), _lib.F32 if px.dtype == torch.float32 else _lib.BF16,
                                             _lib.ptr(out), B, n_state, _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, "visrep_sam_forward")
        return out


def make_sam_engine(spec, weights: dict, device=None, precision: str = "bf16") -> SamEngine:
    """make_engine for SAM towers: bf16 on the GPU, and a ValueError that says so for anything else."""
    if precision not in ("bf16", "bfloat16"):
        raise ValueError(f"SAM towers run in bf16 only: there is no {precision} SAM engine (a full fp32 engine is out of scope)")
    return SamEngine(spec, weights, device)


def relpos_tables(qk: torch.Tensor, Rh: torch.Tensor, Rw: torch.Tensor, NB: int, S: int, H: int, out=None):
    """qk [NB S S, ldqk] bf16 (Q in the first H 64 columns), Rh / Rw [2 S - 1, 64] fp32 -> (rel_h, rel_w) fp32 [NB, H, S S, S] - visrep_relpos_tables
    on the GPU, its host twin for host tensors.  out: a (rel_h, rel_w) pair to write into instead of allocating."""
    T = S * S
    if out is not None:
        rel_h, rel_w = out
    else:
        rel_h = torch.empty(NB, H, T, S, dtype=torch.float32, device=qk.device)
        rel_w = torch.empty_like(rel_h)
    if qk.device.type == "cpu":
        _lib.check(_lib.load().visrep_relpos_tables_cpu(_lib.ptr(qk), qk.stride(0), _lib.ptr(Rh), _lib.ptr(Rw), _lib.ptr(rel_h), _lib.ptr(rel_w), NB, S, H,
                                                        64, 0), "visrep_relpos_tables_cpu")
        return rel_h, rel_w
    lib = _lib.require_gpu()
    with torch.cuda.device(qk.device):
        _lib.check(lib.visrep_relpos_tables(_lib.ptr(qk), qk.stride(0), _lib.ptr(Rh), _lib.ptr(Rw), _lib.ptr(rel_h), _lib.ptr(rel_w), NB, S, H, 64,
                                            _lib.stream_ptr()), "visrep_relpos_tables")
    return rel_h, rel_w


def mhsa_relpos(qk: torch.Tensor, vt: torch.Tensor, rel_h: torch.Tensor, rel_w: torch.Tensor, NB: int, S: int, H: int, scale: float = 0.125) -> torch.Tensor:
    """visrep_mhsa_relpos_fwd: qk [NB S S, ldqk] bf16, vt [H 64, ldvt] bf16 (VISREP_EPI_VT layout), tables fp32 [NB, H, S S, S] -> [NB S S, H 64] bf16."""
    lib = _lib.require_gpu()
    out = torch.empty(NB * S * S, H * 64, dtype=torch.bfloat16, device=qk.device)
    with torch.cuda.device(qk.device):
        _lib.check(lib.visrep_mhsa_relpos_fwd(_lib.ptr(qk), qk.stride(0), _lib.ptr(vt), vt.stride(0), _lib.ptr(rel_h), _lib.ptr(rel_w), _lib.ptr(out),
                                              out.stride(0), NB, S, H, 64, float(scale), _lib.stream_ptr()), "visrep_mhsa_relpos_fwd")
    return out
