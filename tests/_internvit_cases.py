"""Shared pieces of the InternViT tests (tests/test_host_internvit.py, tests/test_gpu_internvit.py): RMSNorm blocks and the RMSNorm over the
whole embedding width behind q_proj / k_proj (HF InternVLVisionModel, the vision tower of the InternVL family).

Oracle.  The real transformers module on random weights: `hf_model` builds one per cell of the matrix norm_type x use_qk_norm x
attention_bias x head geometry and gives every parameter that random init leaves at a constant (cls, position table, lambda_*, norm weights,
biases) a value; `hf_from_packed` loads a packed dict (synthetic_weights / hostile_weights) into the module, so that towers without a
checkpoint are checked against the same code.

Bounds (stated as formulas, u = 2^-24, the unit roundoff of fp32):
  * one wave sums the d squares of a row as n_l = 8 * ceil(d / 512) sequential FMAs per lane, six shuffle-adds, then mean, + eps, sqrt and a
    reciprocal: the sum of non-negative terms carries at most (n_l + 6) u relative error, the square root halves it, the four scalar operations
    add u each - RSTD_REL(d) = ((n_l + 6) / 2 + 4) u bounds rstd's relative error;
  * an output element is x * rstd * g (two more roundings) and then ONE rounding to bf16.  bf16 keeps 8 significant bits (7 stored), so
    round-to-nearest moves a value by at most half an ulp = 2^-8 of it (the unit roundoff of the format; 2^-9 would be that of a 9-bit one):
    OUT_REL(d) = 2^-8 + (RSTD_REL(d) + 2 u) (1 + 2^-8);
  * two fp32 sums of the same N non-negative terms in different orders differ by at most 2 (N - 1) u relative, their rsqrt by half of it plus
    the scalar operations of both sides: ORDER_REL(N) = (N + 7) u.
"""
import math
import os
import sys
from dataclasses import replace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(__file__))

from law_of_vision_representation_in_mllms_amd import vit_weights as VW  # noqa: E402

U = 2.0 ** -24


def lane_terms(d):
    return 8 * math.ceil(d / 512)


def rstd_rel(d):
    return ((lane_terms(d) + 6) / 2 + 4) * U


def out_rel(d):
    return 2.0 ** -8 + (rstd_rel(d) + 2 * U) * (1 + 2.0 ** -8)


def order_rel(n):
    return (n + 7) * U


def bf16_round(a):
    """float64 / float32 array -> the nearest bf16 values (round to nearest even), as float64."""
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def bf16_bits(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().copy()


def from_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).double().numpy()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------------------------ RMSNorm row cases
RMS_DS = (64, 1024, 2056, 3200, 4096)        # first partial 64-lane chunk, the old LayerNorm kernels' range, past 2048, InternViT-6B, the widest
RMS_ROWS = (1, 5, 130)
EPS = 1e-6


def rms_rows_input(rows, d, seed):
    """bf16-exact rows: N(0, 1); row 1 (when there is one) carries one channel at 200 x the rest, the last row of a multi-row case is all zero."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((rows, d))
    if rows > 1:
        x[1, (7 * d) // 13] *= 200.0
        x[-1] = 0.0
    g = rs.standard_normal(d) * 0.5 + 1.0
    return bf16_round(x), g.astype(np.float32)


def rms_oracle(x, g, eps=EPS, d_true=None):
    """float64: (rstd [rows], y [rows, d])."""
    d_true = x.shape[1] if d_true is None else d_true
    rstd = 1.0 / np.sqrt((x * x).sum(1) / d_true + eps)
    return rstd, x * rstd[:, None] * g.astype(np.float64)[None]


# ------------------------------------------------------------------------------------------------ QK-norm cases
QK_GEOMETRIES = ((2, 64, 64), (2, 72, 96), (25, 128, 128), (3, 80, 96))   # (heads, head_dim, head_pad)
QK_ROWS = (1, 67)


def qk_input(rows, heads, hd, hp, seed):
    """{"qk": bf16-exact [rows, 2, heads, hp] with zero pad lanes, "qg" / "kg": fp32 [heads, hp] with zero pad lanes (0.02 .. 3, random signs)}"""
    rs = np.random.RandomState(seed)
    qk = np.zeros((rows, 2, heads, hp))
    qk[..., :hd] = rs.standard_normal((rows, 2, heads, hd)) * np.array([0.3, 2.0])[None, :, None, None]
    gains = []
    for _ in range(2):
        g = np.zeros((heads, hp), dtype=np.float32)
        g[:, :hd] = np.exp(rs.uniform(np.log(0.02), np.log(3.0), (heads, hd))) * np.where(rs.rand(heads, hd) < 0.5, -1.0, 1.0)
        gains.append(g)
    return {"qk": bf16_round(qk), "qg": gains[0], "kg": gains[1]}


def qk_oracle(inp, hd, eps=EPS):
    """float64 [rows, 2, heads, hp]: each half of each row normalised over ALL its columns with the mean over the true width heads * hd."""
    qk = inp["qk"]
    rows, _, heads, hp = qk.shape
    g = np.stack([inp["qg"], inp["kg"]]).astype(np.float64)
    rstd = 1.0 / np.sqrt((qk * qk).sum((2, 3)) / (heads * hd) + eps)
    return qk * rstd[:, :, None, None] * g[None]


QK_BASE = dict(qk=0, ldqk=256 + 8, width=128, d_true=128, qn_g=0, kn_g=0, rows=4, eps=EPS)
QK_POINTERS = ("qk", "qn_g", "kn_g")
ERR_ARG, ERR_SHAPE = -1, -2
QK_REFUSALS = tuple(
    [(f"null {p}", {p: None}, ERR_ARG, "null pointer") for p in QK_POINTERS]
    + [(f"{p} + 8 bytes", {p: 8}, ERR_ARG, "16-byte aligned") for p in QK_POINTERS]
    + [("width 4104", {"width": 4104, "ldqk": 8208, "d_true": 4104}, ERR_SHAPE, "at most 4096"), ("width 132", {"width": 132}, ERR_SHAPE, "multiple of 8"),
       ("ldqk % 8", {"ldqk": 260}, ERR_SHAPE, "ldqk % 8"), ("ldqk short", {"ldqk": 248}, ERR_SHAPE, "ldqk >= 2 * width"),
       ("d_true 0", {"d_true": 0}, ERR_SHAPE, "d_true"), ("d_true above width", {"d_true": 136}, ERR_SHAPE, "d_true")])


def qk_refusal_args(overrides, base_ptr):
    a = dict(QK_BASE)
    for n in QK_POINTERS:
        a[n] = base_ptr
    for n, v in overrides.items():
        a[n] = (None if v is None else base_ptr + v) if n in QK_POINTERS else v
    return list(a.values())


# ------------------------------------------------------------------------------------------------ towers
NORMS = ("layer_norm", "rms_norm")
HOST_MATRIX = tuple((n, q, b, h) for n in NORMS for q in (False, True) for b in (False, True) for h in ((2, 64), (2, 72)))


def matrix_id(cell):
    n, q, b, (H, dh) = cell
    return f"{n}-{'qk' if q else 'noqk'}-{'bias' if b else 'nobias'}-{H}x{dh}"


def hf_config(norm_type="rms_norm", qk=True, bias=False, heads=(2, 64), layers=3, image=28, patch=7, mlp=256, eps=1e-6, **kw):
    import transformers
    return transformers.InternVLVisionConfig(hidden_size=heads[0] * heads[1], num_hidden_layers=layers, num_attention_heads=heads[0],
                                             intermediate_size=mlp, image_size=[image, image], patch_size=[patch, patch], norm_type=norm_type,
                                             use_qk_norm=qk, attention_bias=bias, layer_norm_eps=eps, **kw)


def hf_model(seed=0, **kw):
    """A tiny random-init transformers.InternVLVisionModel with non-trivial lambda_*, q_norm / k_norm / block-norm weights, cls, positions, biases."""
    import transformers
    torch.manual_seed(seed)
    model = transformers.InternVLVisionModel(hf_config(**kw)).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "lambda_" in n or (("norm" in n) and n.endswith("weight")):
                p.copy_((torch.rand(p.shape, generator=g) + 0.5) * torch.where(torch.rand(p.shape, generator=g) < 0.25, -1.0, 1.0))
            elif "cls_token" in n or "position_embeddings" in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            elif n.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return model


def hf_hidden(model, pixels, k, dtype=torch.float32):
    """hidden_states[k] of the module run in `dtype` (a copy is cast: the caller's fp32 weights are never rounded)."""
    import copy
    m = model if dtype == torch.float32 else copy.deepcopy(model).to(dtype)
    with torch.no_grad():
        return m(pixels.to(dtype), output_hidden_states=True).hidden_states[k].float()


def internvit_tiny_spec(norm="rmsnorm", qk=True, heads=(2, 64), image=28, patch=7, mlp=256, layers=3):
    return replace(VW.tiny_spec("internvl", image_size=image, patch=patch, d=heads[0] * heads[1], heads=heads[0], mlp=mlp, layers=layers),
                   norm=norm, qk_norm=qk)


def hf_from_packed(spec, w):
    """transformers.InternVLVisionModel carrying a packed dict (the inverse of vit_weights.pack_hf_state_dict): the oracle of towers built from
    synthetic_weights / hostile_weights."""
    import transformers
    d, p = spec.d, spec.patch
    cfg = hf_config({"layernorm": "layer_norm", "rmsnorm": "rms_norm"}[spec.norm], spec.qk_norm, True, (spec.heads, d // spec.heads), len(w["layers"]),
                    spec.image_size, p, spec.mlp, spec.eps)
    model = transformers.InternVLVisionModel(cfg).eval()
    sd = {"embeddings.cls_token": w["cls"].reshape(1, 1, d), "embeddings.position_embeddings": w["pos"].reshape(1, -1, d),
          "embeddings.patch_embeddings.projection.weight": w["patch_w"].reshape(d, 3, p, p), "embeddings.patch_embeddings.projection.bias": w["patch_b"]}
    for i, L in enumerate(w["layers"]):
        pre = f"encoder.layer.{i}."
        for j, c in enumerate("qkv"):
            sd[pre + f"attention.{c}_proj.weight"] = L["wqkv"][j * d:(j + 1) * d]
            sd[pre + f"attention.{c}_proj.bias"] = L["bqkv"][j * d:(j + 1) * d]
        sd.update({pre + "attention.projection_layer.weight": L["wo"], pre + "attention.projection_layer.bias": L["bo"],
                   pre + "lambda_1": L["ls1"], pre + "lambda_2": L["ls2"], pre + "layernorm_before.weight": L["ln1_g"],
                   pre + "layernorm_after.weight": L["ln2_g"], pre + "mlp.fc1.weight": L["w1"], pre + "mlp.fc1.bias": L["b1"],
                   pre + "mlp.fc2.weight": L["w2"], pre + "mlp.fc2.bias": L["b2"]})
        if spec.norm == "layernorm":
            sd.update({pre + "layernorm_before.bias": L["ln1_b"], pre + "layernorm_after.bias": L["ln2_b"]})
        if spec.qk_norm:                                          # absent in a packed dict = ones, the module's own initial value
            sd.update({pre + f"attention.{c}_norm.weight": L[f"{c}n_g"] if L.get(f"{c}n_g") is not None else torch.ones(d) for c in "qk"})
    model.load_state_dict({k: v.detach().float().clone() for k, v in sd.items()}, strict=True)
    return model


def save_checkpoint(model, path, wrap=False, prefix="model.", extra=None):
    """save_pretrained of the bare vision model; wrap=True writes the InternVL layout instead: config.json with the tower as `vision_config`
    and the weights under `model.vision_tower.` (prefix="": the older `vision_tower.` layout); `extra`: further tensors of the checkpoint
    (language model, projector) that the tower loader must leave alone."""
    import json
    if not wrap:
        model.save_pretrained(path)
        return
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    import transformers
    cfg = transformers.InternVLConfig(vision_config=model.config.to_dict())
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg.to_dict(), f)
    sd = {prefix + "vision_tower." + k: v.contiguous() for k, v in model.state_dict().items()}
    sd.update(extra or {})
    save_file(sd, os.path.join(path, "model.safetensors"))
