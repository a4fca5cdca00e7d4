"""ConvNeXt tower specs and weight packing (host side, torch-CPU only), beside vit_weights.py: a hierarchical convolutional tower shares
nothing with ViTSpec but the packing conventions.

The tower is HF `ConvNextModel` (and, through a key rename, the timm ConvNeXt trunk of OpenCLIP's `convnext_*` models): a 4x4 stride-4 stem
convolution + LayerNorm, then four stages of blocks  x + ls * pwconv2(GELU(pwconv1(LayerNorm(dwconv7x7(x))))), stages 2 .. 4 behind a
LayerNorm + 2x2 stride-2 convolution.  Every LayerNorm of the hidden states uses eps 1e-6 (HF hard-codes it; `layer_norm_eps` is the pooler's).

Packed layout (fp32 torch tensors on CPU; matrices in nn.Linear [out, in] form):
  stem_w [C0, 48] (k = c 16 + i 4 + j)  stem_b [C0]  stem_ln_g / stem_ln_b [C0]
  stages[s]: ds_ln_g / ds_ln_b [C_(s-1)], ds_w [C_s, 4 C_(s-1)] (k = (i 2 + j) C_(s-1) + c), ds_b [C_s]   (None for s = 0)
             blocks[i]: dw_w [49, C] (tap-major, tap = ky 7 + kx)  dw_b [C]  ln_g / ln_b [C]  w1 [4C, C]  b1 [4C]  w2 [C, 4C]  b2 [C]  ls [C]|None
`device_layout` turns that into what visrep_convnext_forward reads: the block LayerNorm folded into pwconv1 and GEMM output widths zero-padded
to a multiple of 128.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Dict, Optional, Tuple

import numpy as np
import torch

EPS = 1e-6


@dataclass(frozen=True)
class ConvNextSpec:
    name: str
    image_size: int
    depths: Tuple[int, int, int, int]
    hidden_sizes: Tuple[int, int, int, int]
    eps: float = EPS
    layerscale: bool = True
    family: str = "convnext"

    def __post_init__(self):
        object.__setattr__(self, "depths", tuple(int(v) for v in self.depths))
        object.__setattr__(self, "hidden_sizes", tuple(int(v) for v in self.hidden_sizes))
        if len(self.depths) != 4 or len(self.hidden_sizes) != 4:
            raise ValueError("ConvNeXt towers have four stages (depths and hidden_sizes of length 4)")
        if any(c % 64 for c in self.hidden_sizes):
            raise ValueError(f"ConvNeXt stage widths must be multiples of 64, got {list(self.hidden_sizes)}: convnext-tiny / convnext-small "
                             "(96 .. 768) are not supported (the depthwise kernel works on slabs of 64 channels)")
        if any(d < 1 for d in self.depths):
            raise ValueError("every ConvNeXt stage needs at least one block")
        if self.image_size <= 0 or self.image_size % 32:
            raise ValueError(f"ConvNeXt input side must be a multiple of 32 (stride 4, then three 2x2 downsamplings), got {self.image_size}")

    @property
    def n_states(self) -> int:
        return 5

    def grid(self, state: int) -> int:
        """Map side of hidden state `state` (0 = stem, 1 .. 4 = stage outputs)."""
        return self.image_size // (4 << max(state - 1, 0))

    def width(self, state: int) -> int:
        return self.hidden_sizes[max(state - 1, 0)]

    def at_resolution(self, image_size: int) -> "ConvNextSpec":
        return replace(self, image_size=image_size)


# Shapes as recalled from the public configs (they could not be read offline); a local config.json always wins.
SPECS: Dict[str, ConvNextSpec] = {
    "facebook/convnext-base-224": ConvNextSpec("facebook/convnext-base-224", 224, (3, 3, 27, 3), (128, 256, 512, 1024)),
    "laion/CLIP-convnext_large_d_320.laion2B-s29B-b131K-ft-soup":
        ConvNextSpec("laion/CLIP-convnext_large_d_320.laion2B-s29B-b131K-ft-soup", 320, (3, 3, 27, 3), (192, 384, 768, 1536)),
    "laion/CLIP-convnext_xxlarge-laion2B-s34B-b82K-augreg-soup":
        ConvNextSpec("laion/CLIP-convnext_xxlarge-laion2B-s34B-b82K-augreg-soup", 256, (3, 4, 30, 3), (384, 768, 1536, 3072)),
}


def tiny_spec(image_size: int = 64, depths=(1, 1, 2, 1), hidden_sizes=(64, 128, 192, 256), layerscale: bool = True) -> ConvNextSpec:
    return ConvNextSpec("tiny-convnext", image_size, tuple(depths), tuple(hidden_sizes), layerscale=layerscale)


def spec_from_hf_config(cfg, name: str = "", crop_size: Optional[int] = None) -> ConvNextSpec:
    """HF ConvNextConfig (model_type 'convnext') -> spec.  crop_size: the processor's, when the checkpoint has one; else cfg.image_size."""
    mt = getattr(cfg, "model_type", "")
    if mt != "convnext":
        raise ValueError(f"unsupported HF model_type {mt!r} (expected 'convnext')")
    if getattr(cfg, "num_channels", 3) != 3 or getattr(cfg, "patch_size", 4) != 4 or getattr(cfg, "num_stages", 4) != 4:
        raise ValueError("ConvNeXt: only 3 input channels, a 4x4 stem and four stages are supported")
    if getattr(cfg, "hidden_act", "gelu") != "gelu":
        raise ValueError(f"ConvNeXt: unsupported hidden_act {cfg.hidden_act!r}")
    return ConvNextSpec(name, int(crop_size or getattr(cfg, "image_size", 224)), tuple(cfg.depths), tuple(cfg.hidden_sizes),
                        layerscale=float(getattr(cfg, "layer_scale_init_value", 1e-6)) > 0)


def hf_config(spec: ConvNextSpec):
    """The HF config of a spec (tests and the oracle build ConvNextModel from it)."""
    from transformers import ConvNextConfig
    return ConvNextConfig(num_channels=3, patch_size=4, num_stages=4, hidden_sizes=list(spec.hidden_sizes), depths=list(spec.depths),
                          hidden_act="gelu", layer_scale_init_value=1e-6 if spec.layerscale else 0.0, image_size=spec.image_size)


_TIMM_RENAMES = (("stem.0.", "embeddings.patch_embeddings."), ("stem.1.", "embeddings.layernorm."), (".downsample.", ".downsampling_layer."),
                 (".blocks.", ".layers."), (".conv_dw.", ".dwconv."), (".norm.", ".layernorm."), (".mlp.fc1.", ".pwconv1."),
                 (".mlp.fc2.", ".pwconv2."))


def _to_hf_keys(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Either key layout -> bare HF ConvNextModel names.  timm / OpenCLIP: `visual.trunk.` prefix, stem.{0,1}, stages.N.downsample.{0,1},
    stages.N.blocks.M.{conv_dw, norm, mlp.fc1, mlp.fc2, gamma}; head / norm_pre / text tower keys are dropped."""
    out = {}
    timm = any(k.startswith(("visual.trunk.", "trunk.", "stem.0.")) for k in sd)
    for k, v in sd.items():
        if timm:
            for p in ("visual.trunk.", "trunk."):
                if k.startswith(p):
                    k = k[len(p):]
                    break
            else:
                if not k.startswith(("stem.", "stages.")):
                    continue                                   # the text tower, logit_scale, visual.head ...
            if not k.startswith(("stem.", "stages.")):
                continue                                       # head.*, norm_pre.*
            for a, b in _TIMM_RENAMES:
                k = k.replace(a, b)
            if k.endswith(".gamma"):
                k = k[:-len("gamma")] + "layer_scale_parameter"
            if k.startswith("stages."):
                k = "encoder." + k
        else:
            for p in ("convnext.", "vision_model.", "model."):
                if k.startswith(p):
                    k = k[len(p):]
                    break
        out[k] = v.detach().float().cpu()
    return out


def pack_hf_state_dict(sd: Dict[str, torch.Tensor], spec: ConvNextSpec) -> dict:
    s = _to_hf_keys(sd)
    C0 = spec.hidden_sizes[0]
    w = {"stem_w": s["embeddings.patch_embeddings.weight"].reshape(C0, 48), "stem_b": s["embeddings.patch_embeddings.bias"],
         "stem_ln_g": s["embeddings.layernorm.weight"], "stem_ln_b": s["embeddings.layernorm.bias"], "stages": []}
    for st in range(4):
        C = spec.hidden_sizes[st]
        pre = f"encoder.stages.{st}."
        stage = {"ds_ln_g": None, "ds_ln_b": None, "ds_w": None, "ds_b": None, "blocks": []}
        if st > 0:
            Ci = spec.hidden_sizes[st - 1]
            cw = s[pre + "downsampling_layer.1.weight"]                      # [C, Ci, 2, 2] -> k = (i 2 + j) Ci + c
            stage.update(ds_ln_g=s[pre + "downsampling_layer.0.weight"], ds_ln_b=s[pre + "downsampling_layer.0.bias"],
                         ds_w=cw.permute(0, 2, 3, 1).reshape(C, 4 * Ci).contiguous(), ds_b=s[pre + "downsampling_layer.1.bias"])
        for i in range(spec.depths[st]):
            b = f"{pre}layers.{i}."
            stage["blocks"].append({
                "dw_w": s[b + "dwconv.weight"].reshape(C, 49).t().contiguous(), "dw_b": s[b + "dwconv.bias"],
                "ln_g": s[b + "layernorm.weight"], "ln_b": s[b + "layernorm.bias"],
                "w1": s[b + "pwconv1.weight"].reshape(4 * C, C), "b1": s[b + "pwconv1.bias"],      # timm conv_mlp trunks keep [4C, C, 1, 1]
                "w2": s[b + "pwconv2.weight"].reshape(C, 4 * C), "b2": s[b + "pwconv2.bias"],
                "ls": s[b + "layer_scale_parameter"].reshape(C) if spec.layerscale else None,
            })
        w["stages"].append(stage)
    return w


def to_hf_state_dict(spec: ConvNextSpec, w: dict) -> Dict[str, torch.Tensor]:
    """The inverse of pack_hf_state_dict (bare ConvNextModel names, without the pooler LayerNorm): what the tests load the oracle module with."""
    C0 = spec.hidden_sizes[0]
    sd = {"embeddings.patch_embeddings.weight": w["stem_w"].reshape(C0, 3, 4, 4), "embeddings.patch_embeddings.bias": w["stem_b"],
          "embeddings.layernorm.weight": w["stem_ln_g"], "embeddings.layernorm.bias": w["stem_ln_b"]}
    for st, stage in enumerate(w["stages"]):
        C = spec.hidden_sizes[st]
        pre = f"encoder.stages.{st}."
        if st > 0:
            Ci = spec.hidden_sizes[st - 1]
            sd[pre + "downsampling_layer.0.weight"], sd[pre + "downsampling_layer.0.bias"] = stage["ds_ln_g"], stage["ds_ln_b"]
            sd[pre + "downsampling_layer.1.weight"] = stage["ds_w"].reshape(C, 2, 2, Ci).permute(0, 3, 1, 2).contiguous()
            sd[pre + "downsampling_layer.1.bias"] = stage["ds_b"]
        for i, L in enumerate(stage["blocks"]):
            b = f"{pre}layers.{i}."
            sd[b + "dwconv.weight"] = L["dw_w"].t().reshape(C, 1, 7, 7).contiguous()
            sd[b + "dwconv.bias"] = L["dw_b"]
            sd[b + "layernorm.weight"], sd[b + "layernorm.bias"] = L["ln_g"], L["ln_b"]
            sd[b + "pwconv1.weight"], sd[b + "pwconv1.bias"] = L["w1"], L["b1"]
            sd[b + "pwconv2.weight"], sd[b + "pwconv2.bias"] = L["w2"], L["b2"]
            if L["ls"] is not None:
                sd[b + "layer_scale_parameter"] = L["ls"]
    return {k: v.detach().float().clone() for k, v in sd.items()}


def synthetic_weights(spec: ConvNextSpec, seed: int = 1) -> dict:
    """Deterministic random-init weights (numpy RandomState).  Fan-in scaled matrices, LayerNorm gains around 1, LayerScale around 0.3: the
    hidden states stay O(1) and every block changes them visibly."""
    rs = np.random.RandomState(seed)

    def rn(*shape, std=0.02, mean=0.0):
        return torch.from_numpy((rs.standard_normal(shape) * std + mean).astype(np.float32))

    C0 = spec.hidden_sizes[0]
    w = {"stem_w": rn(C0, 48, std=48 ** -0.5), "stem_b": rn(C0), "stem_ln_g": rn(C0, std=0.1, mean=1.0), "stem_ln_b": rn(C0, std=0.1), "stages": []}
    for st in range(4):
        C = spec.hidden_sizes[st]
        stage = {"ds_ln_g": None, "ds_ln_b": None, "ds_w": None, "ds_b": None, "blocks": []}
        if st > 0:
            Ci = spec.hidden_sizes[st - 1]
            stage.update(ds_ln_g=rn(Ci, std=0.1, mean=1.0), ds_ln_b=rn(Ci, std=0.1), ds_w=rn(C, 4 * Ci, std=(4 * Ci) ** -0.5), ds_b=rn(C))
        for _ in range(spec.depths[st]):
            stage["blocks"].append({
                "dw_w": rn(49, C, std=1.0 / 7), "dw_b": rn(C, std=0.1), "ln_g": rn(C, std=0.1, mean=1.0), "ln_b": rn(C, std=0.1),
                "w1": rn(4 * C, C, std=C ** -0.5), "b1": rn(4 * C), "w2": rn(C, 4 * C, std=(4 * C) ** -0.5), "b2": rn(C),
                "ls": rn(C, std=0.05, mean=0.3) if spec.layerscale else None,
            })
        w["stages"].append(stage)
    return w


def hostile_weights(spec: ConvNextSpec, seed: int = 1, profile: str = "outlier", n_outlier: int = 4, outlier=(50.0, 200.0), ls_range=(1e-5, 1.0),
                    const_value: float = 25.0) -> dict:
    """The profiles vit_weights.hostile_weights plants, on a ConvNeXt: starts from `synthetic_weights` and plants, deterministically per seed,
    "outlier" (and "all"): `n_outlier` channels of stage 1 and of stage 3 whose writer - the rows of the stage's first pwconv2 - is scaled by a
      log-uniform factor in `outlier` with a bias of +-(50 .. 200); the LayerNorm gains of the stage's LATER blocks, and of the downsampling
      LayerNorm behind it, are 0.02 for half of those channels and 3 for the other half (a squashed and an amplified outlier column in the
      folded pwconv1).  Those channels keep LayerScale 0.5 so that the planted activations survive.
    "const" (and "all"): `const_value` (25) added to every channel of the first depthwise bias of each stage: every row of that convolution's
      output sits at |mean| ~ 25 std - the case var = E[x^2] - mean^2 from partial sums is worst at (a ConvNeXt has no position table: the
      near-constant position of the ViT profile is every position here).
    every profile: LayerScale spread log-uniformly over `ls_range` (1e-5 .. 1) with random signs."""
    if profile not in ("outlier", "const", "all"):
        raise ValueError(f"profile must be 'outlier', 'const' or 'all', got {profile!r}")
    w = synthetic_weights(spec, seed=seed)
    rs = np.random.RandomState(seed + 7919)
    plant = profile in ("outlier", "all")
    info = {"profile": profile, "channels": {}}
    for st, stage in enumerate(w["stages"]):
        C = spec.hidden_sizes[st]
        ch = None
        if plant and st in (0, 2):
            ch = np.sort(rs.choice(C, n_outlier, replace=False))
            fac = np.exp(rs.uniform(np.log(outlier[0]), np.log(outlier[1]), n_outlier)).astype(np.float32)
            sgn = np.where(rs.rand(n_outlier) < 0.5, -1.0, 1.0).astype(np.float32)
            L = stage["blocks"][0]
            L["w2"], L["b2"] = L["w2"].clone(), L["b2"].clone()
            L["w2"][torch.from_numpy(ch)] *= torch.from_numpy(fac)[:, None]
            L["b2"][torch.from_numpy(ch)] = torch.from_numpy(sgn * fac / 0.5)
            gains = [b for b in stage["blocks"][1:]]
            for L2 in gains:
                L2["ln_g"] = L2["ln_g"].clone()
                L2["ln_g"][torch.from_numpy(ch[0::2])] = 0.02
                L2["ln_g"][torch.from_numpy(ch[1::2])] = 3.0
            if st + 1 < 4:
                nxt = w["stages"][st + 1]
                nxt["ds_ln_g"] = nxt["ds_ln_g"].clone()
                nxt["ds_ln_g"][torch.from_numpy(ch[0::2])] = 3.0
                nxt["ds_ln_g"][torch.from_numpy(ch[1::2])] = 0.02
            info["channels"][st] = ch.tolist()
        for i, L in enumerate(stage["blocks"]):
            if spec.layerscale:
                mag = np.exp(rs.uniform(np.log(ls_range[0]), np.log(ls_range[1]), C)).astype(np.float32)
                sg = np.where(rs.rand(C) < 0.5, -1.0, 1.0).astype(np.float32)
                v = torch.from_numpy(mag * sg)
                if ch is not None:
                    v[torch.from_numpy(ch)] = 0.5
                L["ls"] = v
            if profile in ("const", "all") and i == 0:
                L["dw_b"] = L["dw_b"] + const_value
    w["hostile"] = info
    return w


def torch_forward(spec: ConvNextSpec, w: dict, pixels: torch.Tensor, dtype=torch.float32):
    """Engine-free restatement of the packed weights in torch (channels-last token rows, the GEMMs the engine runs): the five hidden states as
    [B, H_s W_s, C_s].  Tests hold it against transformers' ConvNextModel - what pins the packer's layouts."""
    F = torch.nn.functional
    B, S = pixels.shape[0], spec.image_size // 4
    cast = lambda t: t.to(dtype)
    cols = pixels.to(dtype).reshape(B, 3, S, 4, S, 4).permute(0, 2, 4, 1, 3, 5).reshape(B * S * S, 48)       # k = c 16 + i 4 + j
    C = spec.hidden_sizes[0]
    x = F.layer_norm(cols @ cast(w["stem_w"]).t() + cast(w["stem_b"]), (C,), cast(w["stem_ln_g"]), cast(w["stem_ln_b"]), spec.eps)
    states = [x.reshape(B, S * S, C)]
    for st, stage in enumerate(w["stages"]):
        if st > 0:
            n = F.layer_norm(x, (C,), cast(stage["ds_ln_g"]), cast(stage["ds_ln_b"]), spec.eps)
            n = n.reshape(B, S // 2, 2, S // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * (S // 2) ** 2, 4 * C)  # k = (i 2 + j) C + c
            S, C = S // 2, spec.hidden_sizes[st]
            x = n @ cast(stage["ds_w"]).t() + cast(stage["ds_b"])
        for L in stage["blocks"]:
            m = x.reshape(B, S, S, C).permute(0, 3, 1, 2)
            y = F.conv2d(m, cast(L["dw_w"]).t().reshape(C, 1, 7, 7), cast(L["dw_b"]), padding=3, groups=C).permute(0, 2, 3, 1).reshape(-1, C)
            hdn = F.gelu(F.layer_norm(y, (C,), cast(L["ln_g"]), cast(L["ln_b"]), spec.eps) @ cast(L["w1"]).t() + cast(L["b1"]))
            o = hdn @ cast(L["w2"]).t() + cast(L["b2"])
            x = x + (o * cast(L["ls"]) if L["ls"] is not None else o)
        states.append(x.reshape(B, S * S, C))
    return states


def _pad_rows(t: torch.Tensor, n: int) -> torch.Tensor:
    out = torch.zeros((n,) + tuple(t.shape[1:]), dtype=torch.float32)
    out[: t.shape[0]] = t.detach().float()
    return out


def pad128(c: int) -> int:
    return (c + 127) // 128 * 128


def device_layout(spec: ConvNextSpec, w: dict) -> dict:
    """Packed fp32 weights -> the arrays visrep_convnext_forward reads (host tensors; matrices bf16, vectors fp32).
    The block LayerNorm is folded into pwconv1 as the ViT engine folds its norms: Linear(LN(y)) = rstd (y (g o W)^T - mean s) + (W b + bias)
    with g o W rounded once to bf16, s[n] the row sums of the ROUNDED matrix, W b taken with the bf16 W the unfused path would multiply with.
    GEMM OUTPUT widths are zero-padded to a multiple of 128 (192 -> 256): rows of stem_w / ds_w / w2 and entries of their biases and of ls;
    the residual stream's padded columns are then zero in every stage, and no GEMM reads them (K is always a true width)."""
    bf = torch.bfloat16
    C0 = spec.hidden_sizes[0]
    stem = torch.zeros(pad128(C0), 64)
    stem[:C0, :48] = w["stem_w"].float()
    out = {"stem_w": stem.to(bf), "stem_b": _pad_rows(w["stem_b"], pad128(C0)), "stem_ln_g": w["stem_ln_g"].float(), "stem_ln_b": w["stem_ln_b"].float(),
           "stages": []}
    for st, stage in enumerate(w["stages"]):
        C = spec.hidden_sizes[st]
        Cp = pad128(C)
        o = {"ds_ln_g": None, "ds_ln_b": None, "ds_w": None, "ds_b": None, "blocks": []}
        if st > 0:
            o.update(ds_ln_g=stage["ds_ln_g"].float(), ds_ln_b=stage["ds_ln_b"].float(), ds_w=_pad_rows(stage["ds_w"], Cp).to(bf),
                     ds_b=_pad_rows(stage["ds_b"], Cp))
        for L in stage["blocks"]:
            Wb = L["w1"].detach().float().to(bf).float()
            Wf = (Wb * L["ln_g"].detach().float()[None]).to(bf)
            o["blocks"].append({
                "dw_w": L["dw_w"].detach().float().contiguous(), "dw_b": L["dw_b"].detach().float(),
                "w1": Wf, "s1": Wf.float().sum(1), "b1": Wb @ L["ln_b"].detach().float() + L["b1"].detach().float(),
                "w2": _pad_rows(L["w2"], Cp).to(bf), "b2": _pad_rows(L["b2"], Cp),
                "ls": None if L["ls"] is None else _pad_rows(L["ls"], Cp),
            })
        out["stages"].append(o)
    return out
