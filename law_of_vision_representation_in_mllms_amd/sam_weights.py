"""SAM ViT tower specs and weight packing (host side, torch-CPU only), beside vit_weights.py and convnext_weights.py.

The tower is HF `SamVisionModel` (the Segment Anything image encoder, a ViTDet-style ViT): patch embedding + an absolute position table
[1, g, g, d], no class token; blocks x + attn(LN1(x)), x + lin2(GELU(lin1(LN2(x)))) whose attention adds the decomposed relative-position
term q.Rh[qh - kh] + q.Rw[qw - kw] (the UNSCALED query) to the logits and runs over 14 x 14 windows of the zero-padded map except in the
layers of `global_attn_indexes`; then the neck conv1x1 -> LayerNorm -> conv3x3 -> LayerNorm (channel norms, eps 1e-6, no conv bias).

Packed layout (fp32 torch tensors on CPU; matrices in nn.Linear [out, in] form):
  patch_w [d, 3 p p] (k = c p p + i p + j)  patch_b [d]  pos [g g, d]
  layers[l]: ln1_g / ln1_b, wqkv [3 d, d] (rows q heads | k heads | v heads), bqkv [3 d], rel_h / rel_w [2 S - 1, 64] (S = window, or g in a
             global layer), wo [d, d], bo, ln2_g / ln2_b, w1 [mlp, d], b1, w2 [d, mlp], b2
  neck_w1 [C, d]  neck_ln1_g / _b [C]  neck_w2 [C, 9 C] (k = (ky 3 + kx) C + c)  neck_ln2_g / _b [C]
`device_layout` turns that into what visrep_sam_forward reads (LayerNorms folded into the Q|K|V and fc1 GEMMs, the raw qkv bias kept for
the pad rows of the windows)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np
import torch

EPS = 1e-6
SAM_MEAN = (0.485, 0.456, 0.406)           # SAM's published pixel statistics (SamImageProcessor defaults: the ImageNet ones)
SAM_STD = (0.229, 0.224, 0.225)


@dataclass(frozen=True)
class SamSpec:
    name: str
    image_size: int
    patch: int
    d: int
    layers: int
    heads: int
    mlp: int
    window: int
    global_attn_indexes: Tuple[int, ...]
    out_channels: int = 256
    eps: float = EPS
    family: str = "sam"

    def __post_init__(self):
        object.__setattr__(self, "global_attn_indexes", tuple(sorted(int(v) for v in self.global_attn_indexes)))
        if self.heads <= 0 or self.d % self.heads or self.d // self.heads != 64:
            raise ValueError(f"SAM towers need heads 64 wide, got d {self.d} / {self.heads} heads = {self.d / max(self.heads, 1):g} "
                             "(sam-vit-huge, 1280 / 16 = 80, is not supported: the relative-position attention kernel is built for width 64)")
        if self.image_size <= 0 or self.patch <= 0 or self.image_size % self.patch:
            raise ValueError(f"SAM input side {self.image_size} must be a positive multiple of the patch {self.patch}")
        if not 2 <= self.grid <= 64:
            raise ValueError(f"SAM patch grid side must be 2 .. 64, got {self.grid} (global attention over at most 4096 tokens)")
        if not 2 <= self.window <= 64:
            raise ValueError(f"SAM window must be 2 .. 64, got {self.window}")
        if self.d % 128 or self.mlp % 128 or self.out_channels % 64:
            raise ValueError("SAM towers need d and mlp multiples of 128 and output channels a multiple of 64")
        if self.layers < 1 or self.layers > 64 or any(not 0 <= i < self.layers for i in self.global_attn_indexes):
            raise ValueError("SAM towers need 1 .. 64 layers and global_attn_indexes inside them")

    @property
    def grid(self) -> int:
        return self.image_size // self.patch

    @property
    def n_states(self) -> int:
        return self.layers + 2

    def width(self, state: int) -> int:
        return self.out_channels if state == self.layers + 1 else self.d

    def side(self, layer: int) -> int:
        """Side of the grids layer `layer` attends over."""
        return self.grid if layer in self.global_attn_indexes else self.window


# Shapes of the public configs (a local config.json always wins).
SPECS: Dict[str, SamSpec] = {
    "facebook/sam-vit-base": SamSpec("facebook/sam-vit-base", 1024, 16, 768, 12, 12, 3072, 14, (2, 5, 8, 11)),
    "facebook/sam-vit-large": SamSpec("facebook/sam-vit-large", 1024, 16, 1024, 24, 16, 4096, 14, (5, 11, 17, 23)),
}


def spec_from_hf_config(cfg, name: str = "", vit_img_size=None) -> SamSpec:
    """HF SamVisionConfig, or a SamConfig (its vision_config is taken) -> spec."""
    cfg = getattr(cfg, "vision_config", cfg)
    if isinstance(cfg, dict):
        from transformers import SamVisionConfig
        cfg = SamVisionConfig(**cfg)
    mt = getattr(cfg, "model_type", "")
    if mt != "sam_vision_model":
        raise ValueError(f"unsupported HF model_type {mt!r} (expected 'sam_vision_model', or a 'sam' config with a vision_config)")
    if not getattr(cfg, "use_rel_pos", True):
        raise ValueError("SAM: use_rel_pos=False is not supported (the tower's attention is the relative-position kernel)")
    if not getattr(cfg, "use_abs_pos", True):
        raise ValueError("SAM: use_abs_pos=False is not supported")
    if not getattr(cfg, "qkv_bias", True):
        raise ValueError("SAM: qkv_bias=False is not supported")
    if getattr(cfg, "hidden_act", "gelu") != "gelu" or getattr(cfg, "num_channels", 3) != 3:
        raise ValueError("SAM: only hidden_act 'gelu' and 3 input channels are supported")
    if vit_img_size and int(vit_img_size) != int(cfg.image_size):
        raise ValueError(f"SAM: vit_img_size {vit_img_size} differs from the checkpoint's image_size {cfg.image_size}: the input side cannot be "
                         "re-targeted (the reference module cannot either: its position table and global relative-position tables are fixed)")
    mlp = int(getattr(cfg, "mlp_dim", None) or cfg.hidden_size * cfg.mlp_ratio)
    return SamSpec(name, int(cfg.image_size), int(cfg.patch_size), int(cfg.hidden_size), int(cfg.num_hidden_layers), int(cfg.num_attention_heads),
                   mlp, int(cfg.window_size), tuple(cfg.global_attn_indexes), int(cfg.output_channels), float(cfg.layer_norm_eps))


def hf_config(spec: SamSpec):
    """The HF config of a spec (tests and the oracle build SamVisionModel from it)."""
    from transformers import SamVisionConfig
    return SamVisionConfig(hidden_size=spec.d, output_channels=spec.out_channels, num_hidden_layers=spec.layers, num_attention_heads=spec.heads,
                           num_channels=3, image_size=spec.image_size, patch_size=spec.patch, hidden_act="gelu", layer_norm_eps=spec.eps,
                           qkv_bias=True, use_abs_pos=True, use_rel_pos=True, window_size=spec.window,
                           global_attn_indexes=list(spec.global_attn_indexes), mlp_dim=spec.mlp)


def _bare(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Either key layout -> bare SamVisionEncoder names: `vision_encoder.*` of SamVisionModel / SamModel (prompt encoder, mask decoder and
    shared embedding keys are dropped), or the bare encoder."""
    out = {}
    pre = "vision_encoder."
    has = any(k.startswith(pre) for k in sd)
    for k, v in sd.items():
        if has:
            if not k.startswith(pre):
                continue
            k = k[len(pre):]
        elif not k.startswith(("patch_embed.", "pos_embed", "layers.", "neck.")):
            continue
        out[k] = v.detach().float().cpu()
    return out


def _rel_table(t: torch.Tensor, S: int, layer: int, name: str) -> torch.Tensor:
    """A layer's rel_pos table must be [2 S - 1, 64]: the reference would interpolate another length (get_rel_pos), this packer refuses it."""
    if tuple(t.shape) != (2 * S - 1, 64):
        raise ValueError(f"SAM: layer {layer} {name} is {tuple(t.shape)}, the tower needs [{2 * S - 1}, 64] (grid side {S}): relative-position "
                         "tables of another length are not supported (they would have to be interpolated)")
    return t


def pack_hf_state_dict(sd: Dict[str, torch.Tensor], spec: SamSpec) -> dict:
    s = _bare(sd)
    d, g, C = spec.d, spec.grid, spec.out_channels
    pos = s["pos_embed"]
    if tuple(pos.shape[1:3]) != (g, g):
        raise ValueError(f"SAM: the checkpoint's position table is {tuple(pos.shape[1:3])}, the spec's grid is {g} x {g}: the input side cannot be re-targeted")
    w = {"patch_w": s["patch_embed.projection.weight"].reshape(d, -1), "patch_b": s["patch_embed.projection.bias"], "pos": pos.reshape(g * g, d),
         "layers": []}
    for l in range(spec.layers):
        p, S = f"layers.{l}.", spec.side(l)
        w["layers"].append({
            "ln1_g": s[p + "layer_norm1.weight"], "ln1_b": s[p + "layer_norm1.bias"], "wqkv": s[p + "attn.qkv.weight"], "bqkv": s[p + "attn.qkv.bias"],
            "rel_h": _rel_table(s[p + "attn.rel_pos_h"], S, l, "rel_pos_h"), "rel_w": _rel_table(s[p + "attn.rel_pos_w"], S, l, "rel_pos_w"),
            "wo": s[p + "attn.proj.weight"], "bo": s[p + "attn.proj.bias"], "ln2_g": s[p + "layer_norm2.weight"], "ln2_b": s[p + "layer_norm2.bias"],
            "w1": s[p + "mlp.lin1.weight"], "b1": s[p + "mlp.lin1.bias"], "w2": s[p + "mlp.lin2.weight"], "b2": s[p + "mlp.lin2.bias"]})
    w.update(neck_w1=s["neck.conv1.weight"].reshape(C, d), neck_ln1_g=s["neck.layer_norm1.weight"], neck_ln1_b=s["neck.layer_norm1.bias"],
             neck_w2=s["neck.conv2.weight"].permute(0, 2, 3, 1).reshape(C, 9 * C).contiguous(),
             neck_ln2_g=s["neck.layer_norm2.weight"], neck_ln2_b=s["neck.layer_norm2.bias"])
    return w


def to_hf_state_dict(spec: SamSpec, w: dict, prefix: str = "vision_encoder.") -> Dict[str, torch.Tensor]:
    """The inverse of pack_hf_state_dict (SamVisionModel names by default; prefix='' = the bare encoder): what the tests load the oracle with."""
    d, g, C, p = spec.d, spec.grid, spec.out_channels, spec.patch
    sd = {"patch_embed.projection.weight": w["patch_w"].reshape(d, 3, p, p), "patch_embed.projection.bias": w["patch_b"],
          "pos_embed": w["pos"].reshape(1, g, g, d)}
    for l, L in enumerate(w["layers"]):
        q = f"layers.{l}."
        sd.update({q + "layer_norm1.weight": L["ln1_g"], q + "layer_norm1.bias": L["ln1_b"], q + "attn.qkv.weight": L["wqkv"], q + "attn.qkv.bias": L["bqkv"],
                   q + "attn.rel_pos_h": L["rel_h"], q + "attn.rel_pos_w": L["rel_w"], q + "attn.proj.weight": L["wo"], q + "attn.proj.bias": L["bo"],
                   q + "layer_norm2.weight": L["ln2_g"], q + "layer_norm2.bias": L["ln2_b"], q + "mlp.lin1.weight": L["w1"], q + "mlp.lin1.bias": L["b1"],
                   q + "mlp.lin2.weight": L["w2"], q + "mlp.lin2.bias": L["b2"]})
    sd.update({"neck.conv1.weight": w["neck_w1"].reshape(C, d, 1, 1), "neck.layer_norm1.weight": w["neck_ln1_g"], "neck.layer_norm1.bias": w["neck_ln1_b"],
               "neck.conv2.weight": w["neck_w2"].reshape(C, 3, 3, C).permute(0, 3, 1, 2).contiguous(),
               "neck.layer_norm2.weight": w["neck_ln2_g"], "neck.layer_norm2.bias": w["neck_ln2_b"]})
    return {prefix + k: v.detach().float().clone() for k, v in sd.items()}


def synthetic_weights(spec: SamSpec, seed: int = 1) -> dict:
    """Deterministic random-init weights (numpy RandomState): fan-in scaled matrices, LayerNorm gains around 1, and NON-ZERO rel_pos_*, pos and
    qkv bias (a freshly constructed HF module has all three at zero: every bias path would go untested)."""
    rs = np.random.RandomState(seed)

    def rn(*shape, std=0.02, mean=0.0):
        return torch.from_numpy((rs.standard_normal(shape) * std + mean).astype(np.float32))

    d, g, C, m = spec.d, spec.grid, spec.out_channels, spec.mlp
    kp = 3 * spec.patch * spec.patch
    w = {"patch_w": rn(d, kp, std=kp ** -0.5), "patch_b": rn(d, std=0.1), "pos": rn(g * g, d, std=0.5), "layers": []}
    for l in range(spec.layers):
        S = spec.side(l)
        w["layers"].append({
            "ln1_g": rn(d, std=0.1, mean=1.0), "ln1_b": rn(d, std=0.1), "wqkv": rn(3 * d, d, std=1.5 * d ** -0.5), "bqkv": rn(3 * d, std=0.3),
            "rel_h": rn(2 * S - 1, 64, std=0.15), "rel_w": rn(2 * S - 1, 64, std=0.15), "wo": rn(d, d, std=d ** -0.5), "bo": rn(d, std=0.02),
            "ln2_g": rn(d, std=0.1, mean=1.0), "ln2_b": rn(d, std=0.1), "w1": rn(m, d, std=d ** -0.5), "b1": rn(m, std=0.02),
            "w2": rn(d, m, std=m ** -0.5), "b2": rn(d, std=0.02)})
    w.update(neck_w1=rn(C, d, std=d ** -0.5), neck_ln1_g=rn(C, std=0.1, mean=1.0), neck_ln1_b=rn(C, std=0.1),
             neck_w2=rn(C, 9 * C, std=(9 * C) ** -0.5), neck_ln2_g=rn(C, std=0.1, mean=1.0), neck_ln2_b=rn(C, std=0.1))
    return w


def hostile_weights(spec: SamSpec, seed: int = 1, n_outlier: int = 3, outlier=(30.0, 100.0), rel_scale: float = 6.0, qkv_bias: float = 4.0) -> dict:
    """`synthetic_weights` with, deterministically per seed:
    * the relative-position tables of the first windowed and the first global layer multiplied by `rel_scale`: with |q| of a few units over 64
      channels the position term reaches tens of units in some heads and dominates scale q.k;
    * a qkv bias of +-`qkv_bias` (several units) on a quarter of the Q, K and V columns of every layer: a pad row of a window that is not the
      raw bias - the folded bias b + W beta, zeros, or a masked key - changes the windows' outputs visibly;
    * `n_outlier` massive-activation channels: rows of the first layer's lin2 scaled by a log-uniform factor in `outlier` with a bias of the
      same size, and LayerNorm gains of the later layers at 0.05 / 2 for them."""
    w = synthetic_weights(spec, seed=seed)
    rs = np.random.RandomState(seed + 7919)
    d = spec.d
    wl = [l for l in range(spec.layers) if l not in spec.global_attn_indexes][:1] + list(spec.global_attn_indexes[:1])
    for l in wl:
        w["layers"][l]["rel_h"] = w["layers"][l]["rel_h"] * rel_scale
        w["layers"][l]["rel_w"] = w["layers"][l]["rel_w"] * rel_scale
    for L in w["layers"]:
        cols = torch.from_numpy(np.sort(rs.choice(3 * d, 3 * d // 4, replace=False)[: 3 * d // 4: 3]))
        b = L["bqkv"].clone()
        b[cols] = torch.from_numpy(np.where(rs.rand(len(cols)) < 0.5, -qkv_bias, qkv_bias).astype(np.float32))
        L["bqkv"] = b
    ch = torch.from_numpy(np.sort(rs.choice(d, n_outlier, replace=False)))
    fac = torch.from_numpy(np.exp(rs.uniform(np.log(outlier[0]), np.log(outlier[1]), n_outlier)).astype(np.float32))
    sgn = torch.from_numpy(np.where(rs.rand(n_outlier) < 0.5, -1.0, 1.0).astype(np.float32))
    L0 = w["layers"][0]
    L0["w2"], L0["b2"] = L0["w2"].clone(), L0["b2"].clone()
    L0["w2"][ch] *= fac[:, None]
    L0["b2"][ch] = sgn * fac
    for L in w["layers"][1:]:
        for k in ("ln1_g", "ln2_g"):
            L[k] = L[k].clone()
            L[k][ch[0::2]] = 0.05
            L[k][ch[1::2]] = 2.0
    w["hostile"] = {"channels": ch.tolist(), "rel_layers": wl}
    return w


def device_layout(spec: SamSpec, w: dict, kpad: int) -> dict:
    """Packed fp32 weights -> the arrays visrep_sam_forward reads (host tensors; matrices bf16, vectors fp32).  LayerNorm folded as the ViT
    engine folds it: Linear(LN(x)) = rstd (x (g o W)^T - mean s) + (W b + bias), g o W rounded once to bf16, s the row sums of the ROUNDED
    matrix, W b with the bf16 W.  bqkv_raw is the unfolded qkv bias: what the projection of a zero (pad) token is."""
    bf = torch.bfloat16

    def fold(Wm, bias, g, b):
        Wb = Wm.detach().float().to(bf).float()
        Wf = (Wb * g.detach().float()[None]).to(bf)
        return Wf, Wf.float().sum(1), Wb @ b.detach().float() + bias.detach().float()

    pw = torch.zeros(spec.d, kpad)
    pw[:, : w["patch_w"].shape[1]] = w["patch_w"].float()
    out = {"patch_w": pw.to(bf), "patch_b": w["patch_b"].float(), "pos": w["pos"].float().contiguous(), "layers": []}
    for l, L in enumerate(w["layers"]):
        S = spec.side(l)
        if tuple(L["rel_h"].shape) != (2 * S - 1, 64) or tuple(L["rel_w"].shape) != (2 * S - 1, 64):
            raise ValueError(f"layer {l}: rel_pos tables must be [{2 * S - 1}, 64], got {tuple(L['rel_h'].shape)} / {tuple(L['rel_w'].shape)}")
        wqkv, sqkv, bqkv = fold(L["wqkv"], L["bqkv"], L["ln1_g"], L["ln1_b"])
        w1, s1, b1 = fold(L["w1"], L["b1"], L["ln2_g"], L["ln2_b"])
        out["layers"].append({"wqkv": wqkv, "bqkv": bqkv, "sqkv": sqkv, "bqkv_raw": L["bqkv"].float().contiguous(),
                              "rel_h": L["rel_h"].float().contiguous(), "rel_w": L["rel_w"].float().contiguous(),
                              "wo": L["wo"].float().to(bf), "bo": L["bo"].float(), "w1": w1, "b1": b1, "s1": s1,
                              "w2": L["w2"].float().to(bf), "b2": L["b2"].float()})
    for k in ("neck_w1", "neck_w2"):
        out[k] = w[k].float().to(bf).contiguous()
    for k in ("neck_ln1_g", "neck_ln1_b", "neck_ln2_g", "neck_ln2_b"):
        out[k] = w[k].float().contiguous()
    return out
