"""Shared pieces of the SwiGLU-FFN tests (tests/test_host_swiglu.py, tests/test_gpu_swiglu.py).

oracle/vit.py cannot express a gated MLP, so the restatement lives here, written from HF modeling_dinov2.py:

    class Dinov2SwiGLUFFN:   hidden = weights_in(x);  x1, x2 = hidden.chunk(2, dim=-1);  return weights_out(silu(x1) * x2)
    hidden width h = (int(int(d * mlp_ratio) * 2 / 3) + 7) // 8 * 8

inside the pre-LN block  x += ls1 * Attn(LN1(x));  x += ls2 * FFN(LN2(x))  of Dinov2Layer.  Weights in the package's packed layout with
w1 [2h, d] / b1 [2h] = weights_in (gate rows, then value rows) and w2 [d, h] = weights_out.

Contract bound of the gated GEMM (`gated_reference`).  The kernel computes, per output element, two fp32 sums of K bf16 products
g and u (exact products, fp32 accumulation in some order), adds the bias, and rounds silu(g) * u to bf16 once:
  * |dg| <= (K + 2) * 2^-24 * sum_k |a_k| |w_k|: K - 1 additions of an fp32 chain each contribute at most 2^-24 of a partial sum that is bounded
    by the sum of magnitudes, the bias addition one more, and one is spare for the accumulator hand-over between MFMA blocks.  Likewise du.
    The bias magnitude joins the sum of magnitudes.
  * y = silu(g) u:  |dy| <= sup|silu'| |u| |dg| + |silu(g)| |du| + second order, sup|silu'| = 1.0998 < 1.1; the second-order term
    1.1 |dg| |du| is below 2^-40 of the magnitudes and is covered by the 0.0002 of slack in 1.1.
  * one bf16 rounding of y: 2^-9 |y| (half an ulp of 8 significant bits), stated as 2^-8 |y| as the issue sets it, and 2^-22 |y| for the fp32
    v_exp / v_rcp / multiplies of silu (each within 1 ulp = 2^-23, and the exponent's argument rounding within the slack of the 2^-8 term).
With the LayerNorm fold the kernel forms g = rstd * acc + (t * s + b) with t = -mean * rstd (two FMAs): the accumulation error is scaled by
|rstd| and the two FMAs add 2^-24 (|rstd acc| + |t s| + |b|) each at most, so
  |dg| <= (K + 2) * 2^-24 * |rstd| * sum_k |a_k| |w_k| + 2 * 2^-24 * (|rstd * acc| + |t * s| + |b|)
and the same for u.  The reference applies the SAME fp32 inputs (rstd, t, s, b as given), in float64.
"""
import hashlib
import math

import torch
import torch.nn.functional as F

from law_of_vision_representation_in_mllms_amd import vit_weights as VW


def swiglu_tiny_spec(d=128, heads=2, mlp=344, layers=3, image_size=42, patch=14):
    """A DINOv2-shaped tower with the gated MLP; mlp = 344 = swiglu_hidden(128, 4) is not a multiple of 16, so both paddings are exercised."""
    return VW.tiny_spec("dinov2", act="swiglu", image_size=image_size, patch=patch, d=d, heads=heads, mlp=mlp, layers=layers)


def swiglu_hidden_states(spec, w, pixels, n_layers=None, dtype=torch.float64):
    """[h0 .. hn] of a swiglu tower in `dtype` (float64 = the reference; bfloat16 = what the reference chain does on a GPU)."""
    p, d, heads, eps = spec.patch, spec.d, spec.heads, spec.eps
    assert spec.act == "swiglu"
    c = lambda t: None if t is None else t.to(dtype)
    x = pixels.to(dtype)
    B = x.shape[0]
    t = F.conv2d(x, c(w["patch_w"]).view(d, 3, p, p), c(w.get("patch_b")), stride=p).flatten(2).transpose(1, 2)
    if w.get("cls") is not None:
        t = torch.cat([c(w["cls"]).view(1, 1, d).expand(B, 1, d), t], dim=1)
    t = t + c(w["pos"]).unsqueeze(0)
    if w.get("pre_ln_g") is not None:
        t = F.layer_norm(t, (d,), c(w["pre_ln_g"]), c(w["pre_ln_b"]), eps)
    hs = [t]
    dh = d // heads
    for L in (w["layers"] if n_layers is None else w["layers"][:n_layers]):
        h = F.layer_norm(t, (d,), c(L["ln1_g"]), c(L["ln1_b"]), eps)
        q, k, v = F.linear(h, c(L["wqkv"]), c(L["bqkv"])).split(d, dim=-1)
        T = q.shape[1]
        q, k, v = (z.view(B, T, heads, dh).transpose(1, 2) for z in (q, k, v))
        a = torch.softmax(((q @ k.transpose(-1, -2)) / math.sqrt(dh)).to(torch.float64 if dtype == torch.float64 else torch.float32), dim=-1).to(dtype)
        o = F.linear((a @ v).transpose(1, 2).reshape(B, T, d), c(L["wo"]), c(L["bo"]))
        t = t + (o * c(L["ls1"]) if L.get("ls1") is not None else o)
        h = F.layer_norm(t, (d,), c(L["ln2_g"]), c(L["ln2_b"]), eps)
        x1, x2 = F.linear(h, c(L["w1"]), c(L["b1"])).chunk(2, dim=-1)          # Dinov2SwiGLUFFN.forward
        h = F.linear(F.silu(x1) * x2, c(L["w2"]), c(L["b2"]))
        t = t + (h * c(L["ls2"]) if L.get("ls2") is not None else h)
        hs.append(t)
    return hs


def interleave(t, mp):
    """HF chunk order [gate | value] (2 mp rows) -> the gated GEMM's row order (engine.swiglu_interleave_index)."""
    from law_of_vision_representation_in_mllms_amd import engine
    return t[engine.swiglu_interleave_index(mp)]


def gated_reference(a, w_hf, b_hf, ln=None):
    """float64 result and per-element bound of the gated GEMM for bf16-valued operands in HF chunk order.
    a [M, K], w_hf [2 mp, K] (fp32 tensors holding bf16 values), b_hf [2 mp] fp32 or None, ln = (rt [M, 2] fp32, s [2 mp] fp32) or None.
    Returns (y [M, mp] float64, bound [M, mp] float64) - see the module docstring for the derivation."""
    A, W = a.double(), w_hf.double()
    K = A.shape[1]
    mp = W.shape[0] // 2
    acc = A @ W.t()                                              # [M, 2 mp]
    mag = A.abs() @ W.abs().t()
    b = torch.zeros(2 * mp, dtype=torch.float64) if b_hf is None else b_hf.double()
    e24 = 2.0 ** -24
    if ln is None:
        z = acc + b
        dz = (K + 2) * e24 * (mag + b.abs())
    else:
        rt, s = ln[0].double(), ln[1].double()
        rstd, tt = rt[:, :1], rt[:, 1:2]
        z = rstd * acc + tt * s + b
        dz = (K + 2) * e24 * rstd.abs() * mag + 2 * e24 * ((rstd * acc).abs() + (tt * s).abs() + b.abs())
    g, u, dg, du = z[:, :mp], z[:, mp:], dz[:, :mp], dz[:, mp:]
    sg = g * torch.sigmoid(g)
    y = sg * u
    bound = 1.1 * u.abs() * dg + sg.abs() * du + (2.0 ** -8 + 2.0 ** -22) * y.abs()
    return y, bound


def weights_digest(w) -> str:
    """sha256 over the flattened packed dict (names and fp32 bytes, sorted by name)."""
    h = hashlib.sha256()
    for k, v in sorted(VW.flatten(w).items()):
        h.update(k.encode() + b"\0" + v.detach().float().contiguous().numpy().tobytes())
    return h.hexdigest()
