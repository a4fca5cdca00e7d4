"""Shared inputs, oracles and bounds of the ConvNeXt tests (tests/test_host_convnext.py, tests/test_gpu_convnext.py).

The tower oracle is transformers.ConvNextModel on the CPU, built from the packed weights.  The kernel oracle is float64 numpy.

Bound of the row statistics.  rt = (rstd, -mean rstd) comes from fp32 sums of n = C values v (the bf16-rounded outputs) and of their squares:
s1 and s2 are summed in some order of n terms, so |s1 - S1| <= g sum|v| and |s2 - S2| <= g S2 with g = n u / (1 - n u), u = 2^-24 (the
standard bound of recursive summation, any order; the squares add one rounding each: n + 1).  With m = S1 / n, q = S2 / n, a = sum|v| / n:
  |dmean| <= g a + u |m|,   |dvar| <= g' q + 2 |m| |dmean| + dmean^2 + 2 u (q + m^2),   g' = (n + 1) u / (1 - (n + 1) u)
(the last term: the roundings of s2 / n, mean^2 and their difference).  rstd = (var + eps)^-1/2 moves by at most |dvar| / (2 (var_lo + eps)^1.5)
+ 2 u rstd with var_lo = max(var - |dvar|, 0), and -mean rstd by |dmean| rstd + |m| drstd + u |m| rstd.  The host twin sums in double and only
rounds the results: it sits inside the same bound.  Nothing here is taken from what the kernels return."""
from __future__ import annotations

import copy

import numpy as np
import torch

from law_of_vision_representation_in_mllms_amd import convnext_weights as CW

U = 2.0 ** -24
EPS = 1e-6

# (B, H, W, C) of the issue, plus one ragged map that takes the 16 x 16 tile (the issue's 20 x 20 map computes fewer padded outputs on 8 x 8 tiles)
DW_CASES = ((3, 2, 2, 64), (2, 5, 9, 64), (1, 16, 16, 192), (2, 20, 20, 128), (1, 8, 8, 3072), (1, 31, 31, 64))
DW_ROUTE = {(3, 2, 2, 64): "dwconv_8", (2, 5, 9, 64): "dwconv_8", (1, 16, 16, 192): "dwconv_16", (2, 20, 20, 128): "dwconv_8",
            (1, 8, 8, 3072): "dwconv_8", (1, 31, 31, 64): "dwconv_16"}
S2D_CASES = ((2, 4, 6, 64), (1, 10, 10, 192))


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def bf16_round(a: np.ndarray) -> np.ndarray:
    """float64 / float32 array -> the nearest bf16 values (ties to even), as float64."""
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).double().numpy()


_INPUTS = {}


def dw_input(case, ld_pad=0):
    """x [B, H, W, C] bf16-exact N(0, 1) with one image shifted to mean 6 and a few large pixels; wt [49, C], bias [C] fp32.  Computed once."""
    key = (case, ld_pad)
    if key not in _INPUTS:
        B, H, W, C = case
        rs = np.random.RandomState(B * 1000 + H * 100 + W * 10 + C)
        x = rs.standard_normal((B, H, W, C))
        x[-1] += 6.0
        x[0, H // 2, W // 2] *= 30.0
        x = torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16)
        wt = torch.from_numpy((rs.standard_normal((49, C)) / 7).astype(np.float32))
        bias = torch.from_numpy((rs.standard_normal(C) * 0.5).astype(np.float32))
        _INPUTS[key] = (x, wt, bias)
    return _INPUTS[key]


_ORACLE = {}


def dw_oracle(case):
    """float64: (exact sums [B, H, W, C], sum of |terms| [B, H, W, C]) of bias + 49 taps, cross-correlation with zero padding 3."""
    if case not in _ORACLE:
        x, wt, bias = dw_input(case)
        B, H, W, C = case
        xp = np.zeros((B, H + 6, W + 6, C))
        xp[:, 3:H + 3, 3:W + 3] = x.double().numpy()
        w = wt.double().numpy()
        acc = np.broadcast_to(bias.double().numpy(), (B, H, W, C)).copy()
        mag = np.abs(acc)
        for ky in range(7):
            for kx in range(7):
                t = xp[:, ky:ky + H, kx:kx + W] * w[ky * 7 + kx]
                acc += t
                mag += np.abs(t)
        _ORACLE[case] = (acc, mag)
    return _ORACLE[case]


def dw_check_output(y: torch.Tensor, case):
    """y equals bf16(float64 result) except where the fp32 chain can land on the other side of a rounding boundary: the chain of 50 terms is
    within s = 50 u sum|terms| of the exact sum (fused multiply-adds: one rounding per term) and rounding is monotonic, so every output lies in
    [bf16(exact - s), bf16(exact + s)] - one value unless a rounding boundary falls inside that interval (a cancelling sum has a wide one)."""
    acc, mag = dw_oracle(case)
    got = y.double().numpy().reshape(acc.shape)
    want = bf16_round(acc)
    slack = 50 * U * mag
    lo, hi = bf16_round(acc - slack), bf16_round(acc + slack)
    exact = got == want
    near = (got >= lo) & (got <= hi)
    assert np.all(exact | near), f"{case}: {(~(exact | near)).sum()} outputs are not the bf16 rounding of the float64 sum"
    assert exact.mean() > 0.98, f"{case}: only {exact.mean():.4f} of the outputs round like the float64 sum"   # a boundary case is rare: 50 u << 2^-9
    return float(1.0 - exact.mean())


def rt_bound(v: np.ndarray, eps: float = EPS):
    """v [rows, n] float64 = the rounded outputs -> (rt_exact [rows, 2], bound [rows, 2]) as derived in the module docstring."""
    n = v.shape[1]
    g, g1 = n * U / (1 - n * U), (n + 1) * U / (1 - (n + 1) * U)
    m, q, a = v.mean(1), (v * v).mean(1), np.abs(v).mean(1)
    var = np.maximum(q - m * m, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    dmean = g * a + U * np.abs(m)
    dvar = g1 * q + 2 * np.abs(m) * dmean + dmean ** 2 + 2 * U * (q + m * m)
    var_lo = np.maximum(var - dvar, 0.0)
    drstd = dvar / (2 * (var_lo + eps) ** 1.5) + 2 * U * rstd
    dshift = dmean * rstd + np.abs(m) * drstd + U * np.abs(m) * rstd
    return np.stack([rstd, -m * rstd], 1), np.stack([drstd, dshift], 1)


def dw_check_rt(rt: torch.Tensor, y: torch.Tensor, case, eps: float = EPS):
    """rt against float64 statistics of the ROUNDED outputs y (whatever y is: the statistics must describe what the GEMM reads)."""
    C = case[3]
    want, bound = rt_bound(y.double().numpy().reshape(-1, C), eps)
    err = np.abs(rt.double().numpy().reshape(-1, 2) - want)
    assert np.all(err <= bound), f"{case}: rt off by up to {(err / bound).max():.2f} x its bound"
    return float((err / bound).max())


def rounded_stats_input():
    """Outputs 256 + x with 0 < x < 0.9 through an identity tap: bf16 keeps steps of 2 above 256, so every ROUNDED output is exactly 256 while
    the fp32 values have a standard deviation of about 0.25."""
    C = 64
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.uniform(0.05, 0.9, (1, 4, 4, C)).astype(np.float32)).to(torch.bfloat16)
    wt = torch.zeros(49, C)
    wt[24] = 1.0
    return x, wt, torch.full((C,), 256.0)


def rounded_stats_check(y, rt):
    """Statistics of the rounded row: var = 0 exactly (64 x 256 and 64 x 65536 are exact in fp32), rstd = eps^-1/2 = 1000, shift = -256000.
    Statistics of the unrounded values would give rstd near 4."""
    assert torch.equal(y.float(), torch.full(y.shape, 256.0))
    r = rt.double().cpu().numpy().reshape(-1, 2)
    assert np.allclose(r[:, 0], 1000.0, rtol=1e-5) and np.allclose(r[:, 1], -256000.0, rtol=1e-5), r[:2]


def s2d_input(case):
    B, H, W, C = case
    rs = np.random.RandomState(H * 100 + W * 10 + C)
    x = rs.standard_normal((B, H, W, C)) * 2.0 + 3.0
    x[0, 0, 0] = 0.0                                            # a constant row: var = 0, rstd = eps^-1/2
    g = torch.from_numpy((1.0 + 0.2 * rs.standard_normal(C)).astype(np.float32))
    b = torch.from_numpy((0.3 * rs.standard_normal(C)).astype(np.float32))
    return torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16), g, b


def s2d_oracle(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float = EPS) -> np.ndarray:
    """float64 LayerNorm + space-to-depth: [B (H/2) (W/2), 4 C], k = (i 2 + j) C + c."""
    B, H, W, C = x.shape
    v = x.double().numpy()
    n = (v - v.mean(-1, keepdims=True)) / np.sqrt(v.var(-1, keepdims=True) + eps) * g.double().numpy() + b.double().numpy()
    return n.reshape(B, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B * (H // 2) * (W // 2), 4 * C)


def s2d_check(out: torch.Tensor, x, g, b):
    """Within one bf16 rounding (2^-9 relative) plus the fp32 evaluation error of (x - mean) rstd g + b: a handful of u on each term's magnitude."""
    want = s2d_oracle(x, g, b)
    B, H, W, C = x.shape
    v = x.double().numpy()
    z = np.abs((v - v.mean(-1, keepdims=True)) / np.sqrt(v.var(-1, keepdims=True) + EPS) * g.double().numpy()) + np.abs(b.double().numpy())
    z = z.reshape(B, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(want.shape)
    bound = 2.0 ** -8 * np.abs(want) + (C + 16) * U * z + 1e-30
    err = np.abs(out.double().numpy() - want)
    assert np.all(err <= bound), f"ln_space_to_depth2: off by up to {(err / bound).max():.2f} x the bound"


# ------------------------------------------------------------------------------------------------ tower oracle
TINY = dict(depths=(1, 1, 2, 1), hidden_sizes=(64, 128, 192, 256))
LARGE_WIDTHS = dict(depths=(1, 1, 1, 1), hidden_sizes=(192, 384, 768, 1536))


def hf_from_packed(spec, w):
    """transformers.ConvNextModel carrying a packed dict (convnext_weights.to_hf_state_dict): the oracle of towers built from packed weights."""
    import transformers
    model = transformers.ConvNextModel(CW.hf_config(spec)).eval()
    missing, unexpected = model.load_state_dict(CW.to_hf_state_dict(spec, w), strict=False)
    assert not unexpected and all(k.startswith("layernorm.") for k in missing), (missing, unexpected)   # only the pooler's LayerNorm is not packed
    return model


def hf_hidden_states(model, pixels, dtype=torch.float32):
    """The five hidden states as token rows [B, H W, C] of the module run in `dtype` (a copy is cast: the caller's weights are never rounded)."""
    m = model if dtype == torch.float32 else copy.deepcopy(model).to(dtype)
    with torch.no_grad():
        hs = m(pixels.to(dtype), output_hidden_states=True).hidden_states
    assert len(hs) == 5
    return [h.float().flatten(2).transpose(1, 2).contiguous() for h in hs]


_PAIRS = {}


def oracle_pair(key, spec, w, px):
    """(the five fp32 hidden states, the module's own bf16 error against each) - computed once per key and shared."""
    if key not in _PAIRS:
        model = hf_from_packed(spec, w)
        want = hf_hidden_states(model, px)
        low = hf_hidden_states(model, px, torch.bfloat16)
        _PAIRS[key] = (want, [rel(a, b) for a, b in zip(low, want)])
    return _PAIRS[key]


def pixels(B, side, seed):
    return torch.randn(B, 3, side, side, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).float()


def timm_state_dict(sd):
    """An HF ConvNextModel state dict renamed to the timm / OpenCLIP layout (timm is not installed: this rename is the second layout's fixture)."""
    out = {}
    for k, v in sd.items():
        if k.startswith("layernorm."):
            k = "visual.trunk.head.norm." + k.split(".", 1)[1]
        else:
            k = k.replace("embeddings.patch_embeddings.", "stem.0.").replace("embeddings.layernorm.", "stem.1.").replace("encoder.stages.", "stages.")
            k = k.replace(".downsampling_layer.", ".downsample.").replace(".layers.", ".blocks.").replace(".dwconv.", ".conv_dw.")
            k = k.replace(".layernorm.", ".norm.").replace(".pwconv1.", ".mlp.fc1.").replace(".pwconv2.", ".mlp.fc2.").replace(".layer_scale_parameter", ".gamma")
            k = "visual.trunk." + k
        out[k] = v
    out["logit_scale"] = torch.tensor(4.6)
    out["text.token_embedding.weight"] = torch.zeros(4, 4)
    return out
