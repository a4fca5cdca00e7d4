"""Shared pieces of the register-token tests (tests/test_host_registers.py, tests/test_gpu_registers.py): DINOv2 with registers
(HF Dinov2WithRegisters) and the prefix-key image-aligned attention kernel attn_fwd_prefix (visrep_mhsa_prefix_fwd).

Tower.  Token rows: CLS, R registers, the patches.  HF adds the position embedding to [CLS | patches] and only then inserts the registers
(Dinov2WithRegistersEmbeddings.forward), so the registers carry no position term; the position table is resized from the native grid with an
ANTIALIASED bicubic (plain DINOv2: not antialiased).  `hidden_states` restates the tower in torch from the packed weights; the host test pins
it - and through it the packer - to transformers' own Dinov2WithRegistersModel.

Kernel cases.  Inputs, oracle, bound and packers are tests/_attention_cases.py's (an image-aligned case is carried as its "cls" route: pre-scaled
Q, head width 64); what is new here is the prefix of NP side keys, their V rows `vpre` [B NP, ldvp] and the constructed kinds:
  sink   one prefix key 40 above every patch score: the reference never moves, patch p sits near 2^-40
  stair  patch maxima climb past the prefix maximum by param[0] per tile (7.5: the move is just not taken on the first tile; 8.5: taken)
  apart  prefix scores 200 apart: all but the largest p_i underflow to exactly 0 in fp32
  ones / qzero  as in _attention_cases
`rounding_model` restates the prefix scheme with the roundings the kernel is allowed - fp32 scores, fp32 prefix p, bf16-rounded patch p, fp32
sums, one bf16 rounding of the output - and the host test holds it to the existing bound on every case."""
import math
import os
import sys
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _attention_cases as AC  # noqa: E402

from law_of_vision_representation_in_mllms_amd import vit_weights as VW  # noqa: E402


# ------------------------------------------------------------------------------------------------ tower
def register_tiny_spec(act="gelu", image_size=112, registers=4, layers=3):
    """d 128, 2 heads of 64, patch 14: grid 8 at 112 px (T = 1 + 4 + 64 = 69: the prefix kernel), grid 4 at 56 px (T = 21: the general one)."""
    mlp = VW.swiglu_hidden(128, 4) if act == "swiglu" else 512
    return VW.tiny_spec("dinov2", act=act, image_size=image_size, patch=14, d=128, heads=2, mlp=mlp, layers=layers, registers=registers)


def hidden_states(spec, w, pixels, n_layers=None, dtype=torch.float64):
    """[h0 .. hn] of a DINOv2(-with-registers) tower from packed weights in `dtype`; w["pos"] is in token-row order (zero rows for registers)."""
    p, d, heads, eps = spec.patch, spec.d, spec.heads, spec.eps
    c = lambda t: None if t is None else t.to(dtype)
    x = pixels.to(dtype)
    B = x.shape[0]
    t = F.conv2d(x, c(w["patch_w"]).view(d, 3, p, p), c(w.get("patch_b")), stride=p).flatten(2).transpose(1, 2)
    pre = [c(w["cls"]).view(1, 1, d).expand(B, 1, d)]
    if spec.registers:
        pre.append(c(w["reg"]).view(1, spec.registers, d).expand(B, spec.registers, d))
    t = torch.cat(pre + [t], dim=1) + c(w["pos"]).unsqueeze(0)
    hs = [t]
    dh = d // heads
    for L in (w["layers"] if n_layers is None else w["layers"][:n_layers]):
        h = F.layer_norm(t, (d,), c(L["ln1_g"]), c(L["ln1_b"]), eps)
        q, k, v = F.linear(h, c(L["wqkv"]), c(L["bqkv"])).split(d, dim=-1)
        T = q.shape[1]
        q, k, v = (z.view(B, T, heads, dh).transpose(1, 2) for z in (q, k, v))
        a = torch.softmax(((q @ k.transpose(-1, -2)) / math.sqrt(dh)).to(torch.float64 if dtype == torch.float64 else torch.float32), dim=-1).to(dtype)
        o = F.linear((a @ v).transpose(1, 2).reshape(B, T, d), c(L["wo"]), c(L["bo"]))
        t = t + o * c(L["ls1"])
        h = F.layer_norm(t, (d,), c(L["ln2_g"]), c(L["ln2_b"]), eps)
        if spec.act == "swiglu":
            x1, x2 = F.linear(h, c(L["w1"]), c(L["b1"])).chunk(2, dim=-1)
            h = F.linear(F.silu(x1) * x2, c(L["w2"]), c(L["b2"]))
        else:
            assert spec.act == "gelu"
            h = F.linear(F.gelu(F.linear(h, c(L["w1"]), c(L["b1"]))), c(L["w2"]), c(L["b2"]))
        t = t + h * c(L["ls2"])
        hs.append(t)
    return hs


def select(hidden, registers, feature):
    """The feature-selection rule: 'patch' drops CLS and registers, 'cls_patch' keeps the CLS row and drops the registers."""
    if feature == "patch":
        return hidden[:, 1 + registers:]
    return torch.cat([hidden[:, :1], hidden[:, 1 + registers:]], dim=1)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def hf_register_model(swiglu=False, seed=0, registers=4):
    """A tiny random-init transformers.Dinov2WithRegistersModel: d 128, 2 heads, 3 layers, patch 14, native grid 5 (image_size 70)."""
    import transformers
    torch.manual_seed(seed)
    cfg = transformers.Dinov2WithRegistersConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, mlp_ratio=4, patch_size=14, image_size=70,
                                                 num_register_tokens=registers, use_swiglu_ffn=swiglu, layerscale_value=1.0)
    model = transformers.Dinov2WithRegistersModel(cfg).eval()
    with torch.no_grad():                                        # random init leaves cls / registers / LayerScale at constants: give them values
        g = torch.Generator().manual_seed(seed + 1)
        model.embeddings.cls_token.copy_(torch.randn(model.embeddings.cls_token.shape, generator=g) * 0.5)
        model.embeddings.register_tokens.copy_(torch.randn(model.embeddings.register_tokens.shape, generator=g) * 0.5)
        model.embeddings.position_embeddings.copy_(torch.randn(model.embeddings.position_embeddings.shape, generator=g) * 0.5)
        for layer in model.encoder.layer:
            layer.layer_scale1.lambda1.copy_(torch.rand(128, generator=g) + 0.5)
            layer.layer_scale2.lambda1.copy_(torch.rand(128, generator=g) + 0.5)
            for n, prm in layer.named_parameters():
                if n.endswith("bias"):
                    prm.copy_(torch.randn(prm.shape, generator=g) * 0.1)
    return model


def save_checkpoint(model, path, crop):
    """save_pretrained + a preprocessor_config.json that names the crop the tower is built at."""
    import json
    model.save_pretrained(path)
    with open(os.path.join(path, "preprocessor_config.json"), "w") as f:
        json.dump({"crop_size": {"height": crop, "width": crop}, "size": {"shortest_edge": crop}}, f)


def hf_hidden(model, pixels, layer=-2):
    with torch.no_grad():
        return model(pixels, output_hidden_states=True).hidden_states[layer]


# ------------------------------------------------------------------------------------------------ kernel cases
class PCase(NamedTuple):
    NP: int
    T: int
    B: int
    H: int
    kind: str = "rand"                    # rand | sink | stair | apart | ones | qzero
    param: tuple = ()
    seed: int = 0

    @property
    def id(self):
        s = f"np{self.NP}-T{self.T}-B{self.B}-H{self.H}"
        return s + (f"-{self.kind}{'_'.join(str(p) for p in self.param)}" if self.kind != "rand" else "")

    @property
    def carrier(self):
        """The _attention_cases.Case that carries oracle / bound / exponents: pre-scaled Q, head width 64, Tq = Tk = T."""
        return AC.Case("cls", self.B, self.T, self.T, self.H, seed=self.seed)


SHAPES = ((2, 66, 2, 2), (5, 69, 2, 2), (8, 72, 2, 2),          # one tile, one query block
          (5, 133, 3, 2),                                          # two query blocks (the second: 5 live rows, three empty waves), batch / head strides
          (5, 197, 70, 1))                                         # 140 workgroups: more than one round of the XCD remap
KINDS = (("rand", ()), ("sink", ()), ("stair", (7.5,)), ("stair", (8.5,)), ("apart", ()), ("ones", ()), ("qzero", ()))
KERNEL_CASES = tuple(PCase(NP, T, B, H, kind, param, seed=1100 + 10 * si + ki)
                     for si, (NP, T, B, H) in enumerate(SHAPES) for ki, (kind, param) in enumerate(KINDS))
C0, C1 = AC.C0, AC.C1


def make_inputs(pc):
    """{"q", "k", "v": bf16-exact float64 [B, T, H, 64], "scale": 0.0}; the exponent of 2 is the raw q.k (pre-scaled Q)."""
    rs = np.random.RandomState(2000 + pc.seed)
    B, T, H, NP = pc.B, pc.T, pc.H, pc.NP
    quiet = pc.kind in ("sink", "stair", "apart")                # background scores of a few hundredths: the constructed keys decide
    amp = 0.05 if quiet else 1.0
    q = rs.standard_normal((B, T, H, 64)) * (amp if quiet else 0.125 * AC.LOG2E)
    k = rs.standard_normal((B, T, H, 64)) * amp
    v = rs.standard_normal((B, T, H, 64))
    if pc.kind == "ones":
        v[:] = 1.0
    elif pc.kind == "qzero":
        q[:] = 0.0
    elif quiet:
        q[..., C0] = 0.0; q[..., C1] = 0.0; k[..., C0] = 0.0; k[..., C1] = 0.0
        if pc.kind == "sink":
            q[..., C1] = 1.0
            k[:, min(2, NP - 1), :, C1] = 40.0
        elif pc.kind == "stair":
            q[..., C0] = 1.0
            for t in range((T - NP) // 64):
                k[:, NP + 64 * t + 11, :, C0] = (t + 1) * pc.param[0]
        elif pc.kind == "apart":
            q[..., C1] = 1.0
            for i in range(NP):
                k[:, i, :, C1] = -200.0 * ((i + 1) % NP)         # the largest prefix score is not the first key's
    elif pc.kind != "rand":
        raise ValueError(pc.kind)
    return {"q": AC.bf16_round(q), "k": AC.bf16_round(k), "v": AC.bf16_round(v), "scale": 0.0}


def oracle(inp, pc):
    return AC.oracle(inp, pc.carrier)


def figures(inp, pc):
    """What the constructed kinds claim, in float64 (image 0, head 0): prefix maximum, per-tile patch maxima, prefix scores."""
    E = AC.exponents(inp, pc.carrier, 0)[0]
    pre = E[:, :pc.NP]
    tiles = np.stack([E[:, pc.NP + 64 * t: pc.NP + 64 * (t + 1)].max(1) for t in range((pc.T - pc.NP) // 64)], 1)
    return {"pre": pre, "pre_max": pre.max(1), "tile_max": tiles}


def rounding_model(inp, pc):
    """The prefix scheme with the roundings the kernel is allowed and no other: fp32 scores; m = max of the prefix scores; prefix p_i =
    fp32 exp2(s_i - m), NOT rounded to bf16; l and O from them in fp32; then whole 64-key tiles as attn_fwd_cls: the reference moves when a
    tile's maximum exceeds it by more than 8, p = fp32 exp2, the row sum over the fp32 p, P.V over the bf16-rounded p; one bf16 rounding of O / l."""
    f32 = AC._f32
    out = np.empty_like(inp["q"])
    case, NP = pc.carrier, pc.NP
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for b in range(pc.B):
            E = f32(AC.exponents(inp, case, b))
            vh = inp["v"][b].transpose(1, 0, 2)
            for h in range(pc.H):
                Eh, V = E[h], vh[h]
                m = Eh[:, :NP].max(1)
                pp = f32(np.exp2(f32(Eh[:, :NP] - m[:, None])))
                l = np.zeros(pc.T); o = np.zeros((pc.T, 64))
                for i in range(NP):
                    l = f32(l + pp[:, i])
                    o = f32(o + pp[:, i:i + 1] * V[i][None, :])
                for t in range((pc.T - NP) // 64):
                    sl = slice(NP + 64 * t, NP + 64 * (t + 1))
                    mloc = Eh[:, sl].max(1)
                    m_new = np.where(mloc - m > 8.0, mloc, m)
                    alpha = np.where(m_new == m, 1.0, f32(np.exp2(f32(m - m_new))))
                    p = f32(np.exp2(f32(Eh[:, sl] - m_new[:, None])))
                    l = f32(l * alpha + f32(p.sum(1)))
                    o = f32(o * alpha[:, None] + AC.bf16_round(p) @ V[sl])
                    m = m_new
                out[b, :, h] = AC.bf16_round(o / l[:, None])
    return out


# ------------------------------------------------------------------------------------------------ packers
LAYOUTS = ("tight", "window")


def layout_dims(layout, pc):
    HD = pc.H * 64
    kcols = pc.B * (pc.T - pc.NP)
    d = {"ldq": 2 * HD, "qoff": 0, "ldvt": kcols, "ldo": HD, "oshift": 0, "ldvp": HD, "vpoff": 0}
    if layout == "window":
        d.update(ldq=2 * HD + 72, qoff=40, ldvt=kcols + 192, ldo=HD + 8, ldvp=HD + 12, vpoff=4)
    elif layout == "narrow_a":
        d.update(ldo=HD + 4)
    elif layout == "narrow_b":
        d.update(ldo=HD + 8, oshift=8)
    else:
        assert layout == "tight", layout
    return d


def pack(inp, pc, layout, hostile=True):
    """As _attention_cases.pack for the image-aligned layout: Q | K one NaN-framed buffer (three NaN rows behind it), V^T of the patch keys
    image-aligned with hostile pad columns, the prefix V rows a window in a NaN buffer (row b NP + i), the output a window in a NaN pattern."""
    d = layout_dims(layout, pc)
    B, T, H, NP = pc.B, pc.T, pc.H, pc.NP
    HD, M = H * 64, B * T
    q2, k2, v2 = (inp[n].reshape(-1, HD) for n in ("q", "k", "v"))
    patch = np.arange(M) % T >= NP
    bufs = {"q": (AC._window(np.concatenate([q2, k2], 1), d["ldq"], d["qoff"], 3 if hostile else 0), d["qoff"]),
            "vt": (AC.pack_vt(v2[patch], d["ldvt"], hostile), 0),
            "vpre": (AC._window(v2[~patch], d["ldvp"], d["vpoff"], 0, align=4), d["vpoff"])}
    lead = AC.OUT_LEAD + d["oshift"] // 2
    bufs["out"] = (np.full(lead + M * d["ldo"] + 64, AC.NAN_BITS, dtype=np.uint16), lead)
    return {"bufs": bufs, "dims": d, "M": M, "HD": HD}


# ------------------------------------------------------------------------------------------------ refusals
PREFIX_BASE = dict(qk=0, ldqk=256, vt=0, ldvt=128, vpre=0, ldvp=128, out=0, ldo=128, B=2, T=69, NP=5, H=2, head_dim=64)
PREFIX_POINTERS = ("qk", "vt", "vpre", "out")
REFUSALS = tuple(
    [(f"NP {n}", {"NP": n, "T": 64 + n}, AC.ERR_SHAPE, "prefix must be 1 .. 8") for n in (0, 9)]
    + [("T - NP not a multiple of 64", {"T": 70}, AC.ERR_SHAPE, "multiple of 64"), ("T - NP below 64", {"T": 5}, AC.ERR_SHAPE, "multiple of 64"),
       ("head_dim 128", {"head_dim": 128}, AC.ERR_SHAPE, "head_dim 64")]
    + [(f"null {p}", {p: None}, AC.ERR_ARG, "null pointer") for p in PREFIX_POINTERS]
    + [(f"{p} + 8 bytes", {p: 8}, AC.ERR_ARG, "16-byte aligned") for p in ("qk", "vt")]
    + [(f"{p} + 4 bytes", {p: 4}, AC.ERR_ARG, "8-byte aligned") for p in ("vpre", "out")]
    + [("ldvt short", {"ldvt": 64}, AC.ERR_SHAPE, "ldvt must cover"), ("ldvp short", {"ldvp": 64}, AC.ERR_SHAPE, "ldvp must cover")])


def refusal_args(overrides, base_ptr):
    a = dict(PREFIX_BASE)
    for n in PREFIX_POINTERS:
        a[n] = base_ptr
    for n, v in overrides.items():
        a[n] = (None if v is None else base_ptr + v) if n in PREFIX_POINTERS else v
    return list(a.values())
