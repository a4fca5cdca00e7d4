"""Shared pieces of the GEMM epilogue contract tests (tests/test_host_gemm_cases.py, tests/test_gpu_gemm_contract.py): a float64 oracle with a
derived per-element bound for every epilogue of the bf16 GEMM family, the row-statistics oracle, the sentinel window builder and the case table.

Operation (csrc/gemm_epilogue.h; the split-K reductions of csrc/gemm_bf16.hip restate it).  Operands are bf16 (held in fp32 tensors here),
bias / ls / ln_s / ln_rt are fp32.  acc = sum_k a[m, k] w[n, k] in fp32, then
    z = acc + bias[n]                                   or, LayerNorm folded (ln = (rt, s)):   z = rstd[m] acc + t[m] s[n] + bias[n]
    BIAS  y = bf16(z)           ACT  y = bf16(act(z))           RESID  y = bf16(resid[m, n] + ls[n] z)   (ls = 1 without LayerScale)
    F32   y = z (fp32)          VT   y = bf16(z) stored transposed: vt[n, perm16(m)], perm16 = the 4-token groups of a 16-token block in the
                                     order 0, 2, 1, 3 (csrc/attention.hip; `perm16` / `vt_unpermute` below)
EPI_PATCH is internal to visrep_vit_forward (the ABI refuses it) and stays covered by the tower parity tests; EPI_GATED has its own
oracle in tests/_swiglu_cases.py.

Bound (`gemm_reference`), u = 2^-24 (half an fp32 ulp):
  * products of two bf16 values have 16 significant bits: exact in fp32.  An fp32 sum of K terms in ANY order (MFMA blocks, the hand-over
    between them, split-K slices added in slice order: S - 1 <= K / 256 - 1 more additions) errs by at most (number of additions) * u * (sum of
    magnitudes): |d acc| <= (K + 8) u mag, mag = sum_k |a| |w|.  The bias addition is one more rounding of at most u (mag + |bias|) and is
    counted inside the same factor: |dz| <= (K + 8) u (mag + |bias|).
  * LayerNorm fold: the accumulation error is scaled by |rstd|; the device forms fma(acc, rstd, fma(t, s, bias)) (tile kernels, 2 roundings) or
    t * s, fma(acc, rstd, .), + bias (reductions, 3 roundings), each of at most u (|rstd acc| + |t s| + |bias|):
    |dz| <= (K + 8) u |rstd| mag + 3 u (|rstd acc| + |t s| + |bias|).  The oracle applies the SAME fp32 rstd, t, s, bias, in float64.
  * RESID: the LayerScale product rounds once (u |ls z|), the residual addition once (u (|ls z| + |resid|)), the error of z is scaled by |ls|:
    |dv| <= |ls| |dz| + u (2 |ls z| + |resid|)  (stated with the factor 2 also when there is no LayerScale).
  * ACT: |d act| <= L |dz| + allowance(z); L = sup |act'| = 1.0998 < 1.1 for x sigmoid(c x) (quick_gelu; the same function of u = c x as silu),
    1.1290 < 1.13 for x Phi(x) (at x = sqrt 2) and for its tanh form (checked on a dense grid by the host test); the second-order term
    L'' dz^2 / 2 is below 2^-40 of the magnitudes and lives in the slack of the constants.  allowance = `act_allowance`, see there.
  * one rounding to bf16 (8 significant bits, round to nearest even): half an ulp is 2^-8 of the binade's lower end, so at most 2^-8 |v| of the
    COMPUTED value v, |v| <= |y| + d with d the sum of the terms above: 2^-8 |y| + 2^-8 d, stated as d (1 + 2^-7) + 2^-8 |y|; plus 2^-126, the
    smallest normal, for results flushed towards zero.  F32 outputs have none of this.  The 2^-8 |y| term is attained (a value just above a
    power of two that falls on a rounding tie), so the worst err / bound over a few thousand bf16 outputs is always close to 1 - for the CPU
    emulation as for the device - and says nothing about the arithmetic; `arithmetic_bound` (the bound without the output rounding, for a
    result taken before it) is what the host test holds the unrounded emulation to, with room to spare.
Nothing in the bound depends on anything a GPU produced.

Device activations (`apply_act`, csrc/common.h) and their allowance.  v_rcp_f32 and v_exp_f32 are accurate to 1 ulp = 2^-23 relative.
  quick_gelu  x * rcp(1 + exp2(c x)), c = fp32(-1.702 log2 e): the exponent's argument carries two roundings (the constant's and the
              product's): relative 2 u, absolute 2 u |c x|, i.e. relative ln2 * 2 u |c x| on e = exp2(.), plus the instruction's 2^-23; 1 + e rounds
              (u), rcp 2^-23, the final product u.  d sigma / sigma = e / (1 + e) * de / e = (1 - sigma) de / e.  Total relative error of y <=
              2^-23 (3 + ln2 |c x| (1 - sigma)); stated as 2^-23 (4 + |arg| (1 - sigma)), arg = the exponent's argument.
  gelu_tanh   x * rcp(1 + exp2(-v)), v = 2.3022082 (x + 0.044715 x^3): v carries at most six roundings (two constants, x * x, the product, the fma,
              the scale): relative 6 u = 3 * 2^-23 -> relative 3 ln2 * 2^-23 |v| on e.  Total <= 2^-23 (4 + 3 |arg| (1 - sigma)), which is what both use.
              Beyond |arg| = 126 the device's exp2 overflows to inf (y = -0 where the true value is below 2^-126 |x|) or underflows (sigma = 1
              exactly, relative error 2^-126): covered by the 2^-126 (1 + |x|) guard.
  gelu        x * Phi(x), Phi from Abramowitz-Stegun 7.1.26: erfc(z) = p(t) t exp(-z^2), t = 1 / (1 + 0.3275911 z), |error| <= 1.5e-7 on erf, so
              0.75e-7 on the half.  fp32 evaluation: Horner with five fma on alternating coefficients (sum of |a_i| t^i <= 4.47 where p >= 0.25, so
              at most 2 * 5 u * 4.47 / 0.25 = 180 u relative on p, in practice a few u), t from one fma and one rcp (3 u), the exponent
              -log2e z^2 with three roundings (relative 3 u, i.e. 3 u z^2 on the exponential, plus 2^-23), two more products:
              |d half| <= 0.75e-7 + half * 2^-23 (96 + 2 z^2), z = |x| / sqrt 2, and |dy| <= |x| |d half| + 2^-23 |y| (1 - half and the last product).
The host test evaluates these formulas in fp32 on a dense grid against float64 and requires the error to stay inside the allowance.

Row statistics (`row_stats_reference`): the device sums x and x^2 of the N bf16 values it WROTE in fp32 (partial sums of 64 columns from the
epilogue, or one block per row in the split-K reduction), then mean = s1 / N, var = max(s2 / N - mean^2, 0), rstd = 1 / sqrt(var + eps),
t = -mean rstd.  With E|x|, E[x^2] of the row:  |d mean| <= (N + 4) u E|x|;  |d var| <= (N + 8) u E[x^2] + 2 |mean| |d mean|  (sum of squares
N + 4 roundings, its scaling, the square of the mean and the subtraction four more, all of quantities <= E[x^2]);
|d rstd| <= rstd (0.55 |d var| / (var + eps) + 4 u)  (first order with 10 % for the curvature, valid while |d var| < 0.1 (var + eps); sqrt and
the division round once each);  |d t| <= rstd |d mean| + |mean| |d rstd| + 2 u |t|.
Because E[x^2] = var + mean^2 and E|x| <= sqrt(E[x^2]), |d var| / var <= 3 (N + 8) u (1 + mean^2 / var): the relative bound on rstd grows
LINEARLY in 1 + mean^2 / var - the cancellation of the one-pass formula.  The two-pass read-back (visrep_layernorm_stats, the route of
split-K at N != 1024 and of tail rows) is far inside the same bound.  RMS: rstd = 1 / sqrt(E[x^2] + eps), no cancellation:
|d rstd| <= rstd (0.55 (N + 8) u + 4 u), t = 0 exactly.
OFFSET rows: the residual carries a common offset of 16 against a row std of 1.5 .. 2.5, |mean| / std = 6 .. 11 ("8" nominal; the tests
assert >= 5 on what was written).  At 8 the bound on var is 65 times the plain rows' (1.2 % of var at N = 1024, 0.3 % at N = 256), which is
visible, while a sum that loses four columns (mean = s1' / N) moves var by 2 * 4 / N * 64 = 50 % (N = 1024): forty times the bound, so the
float64 oracle still separates right from wrong; the average of N - 4 columns (mean = s1' / (N - 4)) moves the mean by about 2 std / N only
and var by about 3 %: still outside the bound on most rows.  A CPU fp32 emulation of the one-pass formula (sequential sums, the worst realistic order) stays below a
tenth of the bound (printed by the host test).  A larger ratio buys nothing: at 64 the bound itself passes 10 % of var and stops separating.

V^T padding columns.  The tile kernels store whole 4-token groups: tokens M .. round_up(M, 4) - 1 of the last group get the projection of
the clamped row M - 1 (with a folded LayerNorm and zero statistics past M: the bias) - finite values; `splitk_reduce_vt` writes zeros
there.  The consumer (csrc/attention.hip) masks every key outside [b T, (b + 1) T) of its image before the softmax, so its P is exactly 0 for
those columns and it needs them FINITE only (0 * finite = 0): the two producers differ in a way the consumer cannot observe.  Contract
checked here: the stored columns of the tokens below round_up(M, 4) may be written with finite values, nothing else - in particular not the
other 4-token groups of the last 16-token block, which perm16 interleaves with the written ones (M = 24: columns 16 .. 19 and 24 .. 27 are
written, 20 .. 23 and 28 .. 31 stay untouched).
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
KINDS = ("bias", "act", "resid", "f32", "vt")
ACTS = ("quick_gelu", "gelu", "gelu_tanh")
LIPSCHITZ = {"quick_gelu": 1.1, "gelu": 1.13, "gelu_tanh": 1.13}
QUICK_C = 1.702 * math.log2(math.e)                     # apply_act: 2.4554669595930157
TANH_C = 2.0 * math.sqrt(2.0 / math.pi) * math.log2(math.e)   # 2.302208198


def bf(x):
    return x.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ activations
def act_exact(name, z):
    """float64 definition of the activation (HF QuickGELUActivation, nn.GELU(), nn.GELU('tanh'))."""
    z = z.double()
    if name == "quick_gelu":
        return z * torch.sigmoid(1.702 * z)
    if name == "gelu":
        return 0.5 * z * torch.erfc(-z / math.sqrt(2.0))        # x Phi(x); erfc keeps the lower tail
    if name == "gelu_tanh":
        return z * torch.sigmoid(2.0 * math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3))   # = 0.5 z (1 + tanh u) without the cancellation at u << 0
    raise ValueError(name)


def act_allowance(name, z):
    """|device formula in fp32 - exact activation| at the exact argument z (float64), from the module docstring."""
    z = z.double()
    y = act_exact(name, z).abs()
    guard = TINY * (1.0 + z.abs())
    if name in ("quick_gelu", "gelu_tanh"):
        arg = QUICK_C * z if name == "quick_gelu" else TANH_C * (z + 0.044715 * z ** 3)          # y = z sigma, sigma = 1 / (1 + exp2(-arg))
        return 2.0 ** -23 * (4.0 + 3.0 * arg.abs() * torch.sigmoid(-arg * math.log(2.0))) * y + guard
    if name == "gelu":
        half = 0.5 * torch.erfc(z.abs() / math.sqrt(2.0))
        return z.abs() * (0.75e-7 + half * 2.0 ** -23 * (96.0 + z * z)) + 2.0 ** -23 * y + guard
    raise ValueError(name)


def act_device_formula_fp32(name, x):
    """`apply_act` of csrc/common.h evaluated in fp32 on the CPU (torch fp32 exp2 / reciprocal are within 1 ulp, like v_exp_f32 / v_rcp_f32).
    fma is emulated by a float64 product-sum rounded once (exact for fp32 operands)."""
    x = x.float()
    fma = lambda a, b, c: (a.double() * b.double() + c.double()).float()
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    if name == "quick_gelu":
        return x * torch.reciprocal(1.0 + torch.exp2(f(-2.4554669595930157) * x))
    if name == "gelu_tanh":
        v = f(2.302208198) * fma(f(0.044715) * x * x, x, x)
        return x * torch.reciprocal(1.0 + torch.exp2(-v))
    if name == "gelu":
        z = x.abs() * f(0.70710678118654752)
        t = torch.reciprocal(fma(f(0.3275911), z, f(1.0)))
        p = fma(f(1.061405429), t, f(-1.453152027))
        for c in (1.421413741, -0.284496736, 0.254829592):
            p = fma(p, t, f(c))
        half = f(0.5) * p * t * torch.exp2(f(-1.4426950408889634) * z * z)
        return x * torch.where(x < 0, half, 1.0 - half)
    raise ValueError(name)


# ------------------------------------------------------------------------------------------------ the oracle
def gemm_reference(kind, a, w, bias, *, act=None, resid=None, ls=None, ln=None):
    """float64 result and per-element bound of one GEMM epilogue.  a [M, K], w [N, K]: fp32 tensors holding bf16 values; bias [N] fp32 or None;
    act: a name of ACTS (kind 'act'); resid [M, N] fp32 holding bf16 values and ls [N] fp32 or None (kind 'resid'); ln = (rt [M, 2] fp32, s [N] fp32)
    or None.  kind 'vt' returns the LOGICAL [M, N] result (compare through vt_unpermute).  Derivation: module docstring."""
    A, W = a.double(), w.double()
    return epilogue_reference(kind, A @ W.t(), A.abs() @ W.abs().t(), A.shape[1], bias, act=act, resid=resid, ls=ls, ln=ln)


def epilogue_reference(kind, acc, mag, K, bias, *, act=None, resid=None, ls=None, ln=None, dacc=None):
    """The epilogue half of `gemm_reference` for an accumulation computed elsewhere (tests/_conv_cases.py: a convolution is the same sum of K
    products): acc [M, N] = the float64 sum, mag [M, N] = the same sum of magnitudes, K = the number of products the device adds per element.
    dacc (optional, [M, N]): an absolute error of acc that is known on top of its summation error (operands that may round the other way)."""
    assert kind in KINDS
    b = torch.zeros(acc.shape[1], dtype=torch.float64, device=acc.device) if bias is None else bias.double()
    if ln is None:
        z = acc + b
        dz = (K + 8) * U * (mag + b.abs())
        if dacc is not None:
            dz = dz + dacc
    else:
        rt, s = ln[0].double(), ln[1].double()
        rstd, t = rt[:, :1], rt[:, 1:2]
        z = rstd * acc + t * s + b
        dz = (K + 8) * U * rstd.abs() * mag + 3 * U * ((rstd * acc).abs() + (t * s).abs() + b.abs())
    if kind == "f32":
        return z, dz + 0.0 * z
    if kind == "act":
        y = act_exact(act, z)
        d = LIPSCHITZ[act] * dz + act_allowance(act, z)
    elif kind == "resid":
        l = torch.ones_like(b) if ls is None else ls.double()
        r = resid.double()
        v = l * z
        y = r + v
        d = l.abs() * dz + U * (2 * v.abs() + r.abs())
    else:
        y, d = z, dz
    return y, d * (1.0 + 2.0 ** -7) + 2.0 ** -8 * y.abs() + TINY


def arithmetic_bound(kind, want, bound):
    """The part of `bound` that is not the output's rounding: what a result taken BEFORE the rounding to bf16 must satisfy."""
    return bound if kind == "f32" else (bound - 2.0 ** -8 * want.abs() - TINY) / (1.0 + 2.0 ** -7)


def perm16(m):
    """Stored column of token m inside its V^T row: the 4-token groups of every aligned 16-token block in the order 0, 2, 1, 3."""
    return (m & ~15) | (((m >> 2) & 1) << 3) | (((m >> 3) & 1) << 2) | (m & 3)


def vt_unpermute(buf, M, col0=0, row0=0, N=None):
    """Logical [M, N] view of a V^T buffer [rows, ld]: out[m, n] = buf[row0 + n, col0 + perm16(m)]."""
    N = buf.shape[0] - row0 if N is None else N
    idx = torch.tensor([col0 + perm16(m) for m in range(M)], dtype=torch.long, device=buf.device)
    return buf[row0:row0 + N].index_select(1, idx).t()


def row_stats_reference(x_bf16, eps, rms):
    """(rt [M, 2], bound [M, 2]) in float64 for the rows x_bf16 [M, N] the kernel actually wrote: rt = (rstd, -mean rstd), or
    (rsqrt(mean(x^2) + eps), 0) for RMS; the bound is that of the device's one-pass fp32 formula (module docstring)."""
    x = x_bf16.double()
    N = x.shape[1]
    ex2, eabs = (x * x).mean(1), x.abs().mean(1)
    if rms:
        rstd = (ex2 + eps).rsqrt()
        return torch.stack([rstd, torch.zeros_like(rstd)], 1), torch.stack([rstd * (0.55 * (N + 8) * U + 4 * U), torch.zeros_like(rstd)], 1)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = (var + eps).rsqrt()
    t = -mean * rstd
    dmean = (N + 4) * U * eabs
    dvar = (N + 8) * U * ex2 + 2 * mean.abs() * dmean
    assert (dvar < 0.1 * (var + eps)).all(), "the first-order statistics bound does not hold for these rows"
    drstd = rstd * (0.55 * dvar / (var + eps) + 4 * U)
    dt = rstd * dmean + mean.abs() * drstd + 2 * U * t.abs()
    return torch.stack([rstd, t], 1), torch.stack([drstd, dt], 1)


def one_pass_stats_fp32(x_bf16, eps, rms, drop_cols=0, renorm=True):
    """CPU fp32 emulation of the device formula with sequential sums.  drop_cols: the mutation 'mean over N - drop_cols columns' - their average
    (renorm) or, with renorm=False, the sum that lost them divided by N."""
    x = x_bf16.float()
    N = x.shape[1]
    s1 = torch.zeros(x.shape[0])
    s2 = torch.zeros(x.shape[0])
    for j in range(N):
        if j < N - drop_cols:
            s1 = s1 + x[:, j]
        s2 = s2 + x[:, j] * x[:, j]
    inv = torch.tensor(1.0 / N, dtype=torch.float32)
    if rms:
        return torch.stack([1.0 / torch.sqrt(s2 * inv + eps), torch.zeros_like(s2)], 1)
    mean = s1 * (torch.tensor(1.0 / (N - drop_cols), dtype=torch.float32) if (drop_cols and renorm) else inv)
    rstd = 1.0 / torch.sqrt(torch.clamp_min(s2 * inv - mean * mean, 0.0) + eps)
    return torch.stack([rstd, -mean * rstd], 1)


# ------------------------------------------------------------------------------------------------ sentinel windows
SENTINEL = {torch.bfloat16: (torch.int16, 0x7FB5), torch.float32: (torch.int32, 0x7FB5A5A5)}   # quiet NaNs with a payload
GUARD_TOP, GUARD_BOTTOM, VT_GUARD_ROWS, VT_GUARD_COLS = 1, 2, 2, 64


def round_up(x, m):
    return (x + m - 1) // m * m


def vt_min_ld(M, col0=0):
    """Columns a V^T buffer needs: the window's offset, the round_up(M, 64) + 64 the kernel may legitimately own, and the guard."""
    return col0 + round_up(M, 64) + 64 + VT_GUARD_COLS


def window_box(M, N, col0, vt=False):
    """(row0, row1, c0, c1): the box of a make_window buffer that holds the window.  V^T: the columns of whole 16-token blocks; which of them
    the kernel may write is `window_mask`'s business (perm16 scatters the last block's tokens)."""
    if vt:
        return VT_GUARD_ROWS, VT_GUARD_ROWS + N, col0, col0 + round_up(M, 16)
    return GUARD_TOP, GUARD_TOP + M, col0, col0 + N


def window_mask(buf, M, N, col0, vt=False):
    """bool mask over buf: True where the kernel may write.  Row-major: the box.  V^T: the N feature rows x the stored columns
    col0 + perm16(m) of the tokens m < round_up(M, 4) (whole 4-token groups; the groups of the last 16-token block at or past M stay out)."""
    mask = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    r0, r1, c0, c1 = window_box(M, N, col0, vt)
    if vt:
        cols = torch.tensor([col0 + perm16(m) for m in range(round_up(M, 4))], dtype=torch.long, device=buf.device)
        mask[r0:r1, cols] = True
    else:
        mask[r0:r1, c0:c1] = True
    return mask


def make_window(M, N, ldc, col0, dtype, vt=False, device="cpu"):
    """(buf, view): a sentinel-filled buffer and the box that holds the window.  Row-major: buf [1 + M + 2, ldc], view = rows [1, 1 + M) x columns
    [col0, col0 + N).  V^T: buf [2 + N + 2, ldc] (guard rows of FEATURES), ldc >= vt_min_ld(M, col0), view = the N feature rows x columns
    [col0, col0 + round_up(M, 16)), of which the kernel may write `window_mask`."""
    idt, pat = SENTINEL[dtype]
    if vt:
        assert dtype == torch.bfloat16 and ldc >= vt_min_ld(M, col0), (ldc, vt_min_ld(M, col0))
        rows = VT_GUARD_ROWS + N + VT_GUARD_ROWS
    else:
        assert ldc >= col0 + N
        rows = GUARD_TOP + M + GUARD_BOTTOM
    buf = torch.full((rows, ldc), pat, dtype=idt, device=device).view(dtype)
    r0, r1, c0, c1 = window_box(M, N, col0, vt)
    return buf, buf[r0:r1, c0:c1]


def stray_writes(buf, M, N, col0, vt=False):
    """Number of elements OUTSIDE the window whose bits are no longer the sentinel's (bitwise on the integer view: a NaN written outside counts)."""
    idt, pat = SENTINEL[buf.dtype]
    changed = (buf.view(idt) != pat) & ~window_mask(buf, M, N, col0, vt)
    return int(changed.sum().item())


def c_offset_bytes(M, N, ldc, col0, dtype, vt=False):
    """Byte offset of the window's first element from the (256-byte aligned) start of its buffer: decides the alignment class of C."""
    r0, _, c0, _ = window_box(M, N, col0, vt)
    return (r0 * ldc + c0) * (4 if dtype == torch.float32 else 2)


# ------------------------------------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    group: str                     # rowmajor | vt | f32 | ln | rows | stats | splitk | headtail
    kind: str                      # one of KINDS
    variant: int                   # visrep_set_gemm_variant
    M: int                         # rows (head-plus-tail: the EDGE; M = 256 * CUs / (N / 256) + edge is computed on the device)
    N: int
    K: int
    win: str                       # window class, see WINDOWS
    route: str                     # '128' | '256' | 'splitk' | 'headtail': the kernel family that must run (asserted from _lib.routes())
    act: Optional[str] = None
    ls: bool = False
    ln: bool = False
    resid: Optional[str] = None    # 'in' (resid is C) | 'same' | 'r8' (resid 8-byte, C 16-byte aligned) | 'c8' (the reverse)
    rows: Optional[Tuple[int, int, int]] = None     # (period, stride, first) of visrep_gemm_bf16_rows
    stats: Optional[str] = None    # 'ln' | 'rms': visrep_gemm_bf16_resid_stats / _resid_rms_stats
    dist: str = "plain"            # statistics rows: 'plain' | 'offset'
    note: str = ""                 # why the route is what it is when a variant falls back

    @property
    def id(self):
        parts = [self.kind + ("-" + self.act if self.act else "") + ("-ls" if self.ls else "") + ("-ln" if self.ln else "") +
                 ("-resid_" + self.resid if self.resid else "") + ("-" + self.stats + "stats-" + self.dist if self.stats else ""),
                 f"v{self.variant}", f"M{self.M}{'+full_rounds' if self.group == 'headtail' else ''}", f"N{self.N}", f"K{self.K}", self.win, "route" + self.route]
        if self.rows:
            parts.append("map%d_%d_%d" % self.rows)
        if self.note:
            parts.append(self.note)
        return "-".join(parts)


# window classes -> (ldc - N, col0) in elements.  Row-major bf16 buffers start 256-byte aligned and the window starts one row down:
#   c   contiguous (ldc = N)                       AL        al  ldc = N + 16, col0 = 8: ldc % 8 == 0 and C 16-byte aligned      AL (WIDE / RWIDE)
#   a8  ldc = N + 16, col0 = 4: C 8-byte aligned only   not AL    l4  ldc = N + 12, col0 = 4: ldc % 8 == 4 (C itself 16-byte aligned)  not AL
#   f4  fp32 outputs: ldc = N + 8, col0 = 4 floats (16-byte aligned, as EPI_F32 requires)
# every class leaves at least 4 elements (8 bytes) of sentinel on both sides of the window inside each row.
WINDOWS = {"c": (0, 0), "al": (16, 8), "a8": (16, 4), "l4": (12, 4), "f4": (8, 4)}
# V^T: (ld - vt_min_ld(M, col0), col0); two guard rows above, so C is 16-byte aligned iff (2 ld + col0) % 8 == 0
#   c / al: wide (16-byte) stores;  a8: col0 = 20, C 8-byte aligned only;  l4: ld % 8 == 4  -> both narrow
VT_WINDOWS = {"c": (0, 0), "al": (16, 16), "a8": (16, 20), "l4": (12, 16)}
RESID_COL0 = {"same": None, "r8": 4, "c8": 8}          # out-of-place residual: its own window of the same ldc at this col0 (None: C's)


def window_of(case, M=None):
    """(ldc, col0) of the case's C."""
    M = case.M if M is None else M
    if case.kind == "vt":
        extra, col0 = VT_WINDOWS[case.win]
        return vt_min_ld(M, col0) + extra, col0
    extra, col0 = WINDOWS[case.win]
    return case.N + extra, col0


def is_al(case, M=None):
    """The epilogue's uniform `al` (row-major) / `wide` (V^T) decision for this case, from the same alignment rule the kernel applies."""
    M = case.M if M is None else M
    ldc, col0 = window_of(case, M)
    if case.kind == "f32":
        return False
    ok = ldc % 8 == 0 and c_offset_bytes(M, case.N, ldc, col0, torch.bfloat16, case.kind == "vt") % 16 == 0
    if case.kind == "resid" and case.resid not in (None, "in"):
        rc = RESID_COL0[case.resid]
        ok = ok and c_offset_bytes(M, case.N, ldc, col0 if rc is None else rc, torch.bfloat16) % 16 == 0
    return ok


def wave_rows(case):
    return 64 if case.route == "128" else 128          # rows of one wave tile: 128 x 128 kernel 64, every 256-wide kernel 128


def expected_family(case):
    """The dispatcher's rule (csrc/gemm_bf16.hip: dispatch_one / duo_wanted / try_split_k) restated for the shapes of the table: K < 1024 is never
    split, K >= 1024 with few tiles and registered scratch always is; no table shape but the head-plus-tail group fills a round of tiles."""
    if case.group == "headtail":
        return "headtail"
    if case.K >= 1024:
        return "splitk"
    v = case.variant
    duo = v >= 6 and case.N % 128 == 0 and case.K >= 128 and case.kind in ("bias", "act", "resid", "vt") and case.rows is None and (v != 7 or case.N <= 1024)
    if duo:
        return "256"
    return "256" if v >= 2 and case.N % 256 == 0 else "128"


def _rm(kind, v, M, N, K, win, route, **kw):
    return Case("rowmajor", kind, v, M, N, K, win, route, **kw)


ROWMAJOR = [
    # ---- BIAS: 128 x 128 kernel (N % 256 != 0; 192: last column tile half empty), every M, every window class
    _rm("bias", 5, 1, 64, 64, "c", "128"), _rm("bias", 5, 17, 64, 64, "al", "128"), _rm("bias", 5, 127, 192, 64, "a8", "128"),
    _rm("bias", 5, 129, 192, 64, "l4", "128"), _rm("bias", 5, 255, 64, 128, "al", "128"), _rm("bias", 5, 257, 192, 64, "c", "128"),
    _rm("bias", 5, 300, 192, 192, "al", "128"), _rm("bias", 1, 300, 256, 64, "al", "128"), _rm("bias", 1, 129, 256, 64, "l4", "128"),
    # 256 x 256 kernels: v5 (default), v2, duo (6, 7 = duo for N <= 1024, 8 = unpipelined duo; N = 128)
    _rm("bias", 5, 1, 256, 64, "al", "256"), _rm("bias", 5, 17, 256, 64, "a8", "256"), _rm("bias", 5, 127, 256, 128, "l4", "256"),
    _rm("bias", 5, 129, 256, 64, "al", "256"), _rm("bias", 5, 255, 512, 64, "c", "256"), _rm("bias", 5, 257, 256, 192, "al", "256"),
    _rm("bias", 5, 300, 512, 64, "a8", "256"),
    _rm("bias", 2, 129, 256, 64, "al", "256"), _rm("bias", 2, 300, 256, 192, "l4", "256"), _rm("bias", 2, 257, 512, 128, "a8", "256"),
    _rm("bias", 6, 129, 128, 128, "al", "256"), _rm("bias", 6, 300, 128, 128, "l4", "256"), _rm("bias", 7, 257, 128, 128, "a8", "256"),
    _rm("bias", 7, 127, 128, 192, "al", "256"), _rm("bias", 8, 255, 128, 128, "al", "256"), _rm("bias", 8, 17, 128, 128, "l4", "256"),
    _rm("bias", 6, 129, 128, 64, "al", "128", note="duo_needs_K128_falls_back"), _rm("bias", 6, 129, 192, 128, "al", "128", note="duo_needs_N128_falls_back"),
    # ---- ACT
    _rm("act", 5, 17, 64, 64, "al", "128", act="quick_gelu"), _rm("act", 5, 127, 192, 64, "l4", "128", act="gelu"),
    _rm("act", 5, 129, 64, 128, "a8", "128", act="gelu_tanh"), _rm("act", 5, 300, 192, 64, "c", "128", act="gelu"),
    _rm("act", 1, 257, 256, 64, "al", "128", act="gelu"), _rm("act", 5, 257, 192, 64, "a8", "128", act="quick_gelu"),
    _rm("act", 5, 127, 64, 64, "al", "128", act="gelu_tanh"),
    _rm("act", 5, 129, 256, 64, "al", "256", act="quick_gelu"), _rm("act", 5, 257, 256, 128, "a8", "256", act="gelu"),
    _rm("act", 5, 300, 512, 64, "l4", "256", act="gelu_tanh"), _rm("act", 5, 1, 256, 64, "c", "256", act="gelu"),
    _rm("act", 5, 255, 256, 192, "al", "256", act="quick_gelu"),
    _rm("act", 2, 129, 256, 64, "l4", "256", act="gelu"), _rm("act", 2, 257, 256, 64, "al", "256", act="gelu_tanh"),
    _rm("act", 6, 300, 128, 128, "al", "256", act="gelu"), _rm("act", 7, 129, 128, 128, "a8", "256", act="quick_gelu"),
    _rm("act", 8, 257, 128, 128, "l4", "256", act="gelu_tanh"),
    # ---- RESID: with / without LayerScale, in place and out of place (same / mixed alignment of C and resid)
    _rm("resid", 5, 17, 64, 64, "al", "128", ls=True, resid="in"), _rm("resid", 5, 127, 192, 64, "a8", "128", resid="in"),
    _rm("resid", 5, 129, 192, 64, "l4", "128", ls=True, resid="same"), _rm("resid", 5, 257, 64, 64, "al", "128", resid="r8"),
    _rm("resid", 5, 300, 192, 64, "a8", "128", ls=True, resid="c8"), _rm("resid", 5, 1, 64, 64, "c", "128", resid="in"),
    _rm("resid", 5, 255, 64, 128, "l4", "128", ls=True, resid="in"), _rm("resid", 1, 300, 256, 64, "al", "128", ls=True, resid="in"),
    _rm("resid", 5, 129, 256, 64, "al", "256", ls=True, resid="in"), _rm("resid", 5, 257, 256, 128, "a8", "256", resid="in"),
    _rm("resid", 5, 300, 512, 64, "al", "256", ls=True, resid="same"), _rm("resid", 5, 129, 256, 64, "al", "256", resid="r8"),
    _rm("resid", 5, 257, 256, 192, "a8", "256", ls=True, resid="c8"), _rm("resid", 5, 17, 256, 64, "l4", "256", resid="in"),
    _rm("resid", 5, 1, 256, 64, "c", "256", ls=True, resid="in"), _rm("resid", 5, 255, 256, 64, "l4", "256", resid="same"),
    _rm("resid", 5, 127, 512, 64, "al", "256", ls=True, resid="in"), _rm("resid", 5, 300, 256, 64, "al", "256", resid="in"),
    _rm("resid", 2, 127, 256, 128, "al", "256", resid="same"),
    _rm("resid", 2, 300, 256, 64, "al", "256", ls=True, resid="in"), _rm("resid", 2, 129, 256, 192, "al", "256", resid="r8"),
    _rm("resid", 2, 257, 256, 64, "l4", "256", ls=True, resid="same"),
    _rm("resid", 6, 129, 128, 128, "al", "256", ls=True, resid="in"), _rm("resid", 6, 300, 128, 128, "al", "256", resid="r8"),
    _rm("resid", 7, 257, 128, 128, "a8", "256", ls=True, resid="c8"), _rm("resid", 8, 127, 128, 128, "l4", "256", resid="in"),
    _rm("resid", 8, 255, 128, 192, "al", "256", ls=True, resid="in"),
]

F32 = [Case("f32", "f32", *t) for t in [
    (5, 1, 64, 64, "c", "128"), (5, 17, 192, 64, "f4", "128"), (5, 127, 64, 128, "f4", "128"), (1, 300, 256, 64, "f4", "128"),
    (5, 129, 256, 64, "f4", "256"), (5, 255, 256, 192, "c", "256"), (5, 257, 512, 64, "f4", "256"), (5, 300, 256, 128, "f4", "256"),
    (2, 129, 256, 64, "f4", "256")]] + [
    Case("f32", "f32", 6, 129, 128, 128, "f4", "128", note="duo_has_no_F32_falls_back"),
    Case("f32", "f32", 6, 257, 256, 128, "f4", "256", note="duo_has_no_F32_runs_v5")]

# V^T: M = 24 and 40 have M % 16 == 8 (the wide body's m + 8 == M chunk), 17 / 127 / 129 / 255 / 257 have M % 4 != 0
VT = [Case("vt", "vt", *t) for t in [
    (5, 1, 64, 64, "c", "128"), (5, 17, 192, 64, "al", "128"), (5, 24, 64, 64, "al", "128"), (5, 24, 64, 64, "l4", "128"),
    (5, 127, 192, 64, "a8", "128"), (5, 129, 64, 128, "al", "128"), (5, 300, 192, 64, "l4", "128"), (5, 257, 64, 64, "c", "128"),
    (1, 300, 256, 64, "al", "128"),
    (5, 1, 256, 64, "al", "256"), (5, 17, 256, 64, "al", "256"), (5, 24, 256, 64, "c", "256"), (5, 40, 256, 64, "al", "256"),
    (5, 127, 256, 128, "l4", "256"), (5, 129, 256, 64, "a8", "256"), (5, 255, 512, 64, "al", "256"), (5, 257, 256, 192, "al", "256"),
    (5, 300, 256, 64, "al", "256"),
    (2, 129, 256, 64, "al", "256"), (2, 24, 256, 64, "l4", "256"), (2, 300, 256, 192, "al", "256"),
    (6, 129, 128, 128, "al", "256"), (6, 24, 128, 128, "a8", "256"), (7, 300, 128, 128, "al", "256"), (8, 257, 128, 128, "l4", "256"),
    (8, 40, 128, 128, "al", "256")]]

LN = [
    Case("ln", "bias", 5, 129, 64, 64, "al", "128", ln=True), Case("ln", "bias", 5, 17, 192, 64, "l4", "128", ln=True),
    Case("ln", "bias", 5, 300, 256, 64, "a8", "256", ln=True), Case("ln", "bias", 2, 257, 256, 64, "al", "256", ln=True),
    Case("ln", "bias", 6, 129, 128, 128, "l4", "256", ln=True),
    Case("ln", "act", 5, 127, 192, 64, "al", "128", act="gelu", ln=True), Case("ln", "act", 5, 257, 256, 128, "l4", "256", act="quick_gelu", ln=True),
    Case("ln", "act", 7, 300, 128, 128, "al", "256", act="gelu_tanh", ln=True), Case("ln", "act", 5, 1, 256, 64, "al", "256", act="gelu", ln=True),
    Case("ln", "vt", 5, 127, 64, 64, "al", "128", ln=True), Case("ln", "vt", 5, 24, 192, 64, "al", "128", ln=True),
    Case("ln", "vt", 5, 300, 256, 64, "al", "256", ln=True), Case("ln", "vt", 5, 129, 256, 64, "l4", "256", ln=True),
    Case("ln", "vt", 6, 257, 128, 128, "al", "256", ln=True), Case("ln", "vt", 2, 24, 256, 64, "a8", "256", ln=True),
]

# row maps: A = (12, 13, 1): period % 16 != 0 (the patch tokens of 13-token images);  B = (16, 20, 3)
MAP_A, MAP_B = (12, 13, 1), (16, 20, 3)
ROWS = [
    Case("rows", "bias", 5, 132, 256, 64, "al", "256", ln=True, rows=MAP_A), Case("rows", "bias", 5, 130, 64, 64, "l4", "128", rows=MAP_A),
    Case("rows", "vt", 5, 132, 64, 64, "l4", "128", rows=MAP_A), Case("rows", "vt", 5, 150, 256, 64, "al", "256", ln=True, rows=MAP_B),
    Case("rows", "act", 5, 150, 192, 64, "a8", "128", act="gelu", rows=MAP_B), Case("rows", "f32", 5, 150, 256, 64, "f4", "256", rows=MAP_B),
    Case("rows", "act", 6, 132, 128, 128, "al", "128", act="quick_gelu", ln=True, rows=MAP_A, note="duo_takes_no_row_map_falls_back"),
    # folded V^T whose last 4-token group straddles M (the group keeps its own rows' statistics), and fewer rows than one group
    Case("rows", "vt", 5, 134, 64, 64, "l4", "128", ln=True, rows=MAP_A), Case("rows", "vt", 5, 2, 64, 64, "al", "128", ln=True, rows=MAP_A),
]

# statistics GEMMs: N = 256 (K = 64): the epilogue's partial sums;  N = 1024 (K = 1024, few tiles): the split-K reduction emits them itself
STATS = [Case("stats", "resid", 5, M, N, K, "al", route, ls=ls, resid="in", stats=st, dist=dist)
         for st in ("ln", "rms") for (N, K, route) in ((256, 64, "256"), (1024, 1024, "splitk")) for dist in ("plain", "offset")
         for (ls, M) in ((False, 129), (True, 300))] + [
    # the LayerNorm entry also takes windows that are not AL (8-byte aligned C, ldc % 8 == 4): the 8-byte-store RESID body emits the partial sums,
    # and the reduction's own statistics at N = 1024.  (Routes that READ the rows back - split-K at N != 1024, tail rows - need ldc % 8 == 0.)
    Case("stats", "resid", 5, 129, 256, 64, "l4", "256", ls=True, resid="in", stats="ln", dist="offset"),
    Case("stats", "resid", 5, 300, 256, 64, "a8", "256", resid="in", stats="ln", dist="plain"),
    Case("stats", "resid", 2, 257, 256, 128, "l4", "256", resid="in", stats="ln", dist="offset"),
    Case("stats", "resid", 5, 129, 1024, 1024, "l4", "splitk", ls=True, resid="in", stats="ln", dist="plain")]

# K = 1024, few tiles, scratch registered: the split-K pair, one case per epilogue of each reduce kernel (splitk_reduce_rms: STATS above)
SPLITK = [
    Case("splitk", "bias", 5, 129, 256, 1024, "al", "splitk"), Case("splitk", "act", 5, 129, 256, 1024, "l4", "splitk", act="gelu"),
    Case("splitk", "resid", 5, 257, 256, 1024, "a8", "splitk", ls=True, resid="in"), Case("splitk", "resid", 5, 129, 256, 1024, "al", "splitk", resid="r8"),
    Case("splitk", "f32", 5, 129, 256, 1024, "f4", "splitk"), Case("splitk", "bias", 5, 129, 256, 1024, "a8", "splitk", ln=True),
    Case("splitk", "vt", 5, 129, 256, 1024, "al", "splitk"), Case("splitk", "vt", 5, 130, 256, 1024, "l4", "splitk"),
    Case("splitk", "vt", 5, 127, 256, 1024, "al", "splitk", ln=True),
]

# head plus tail: M = one full round of 256 x 256 tiles + the edge below, N = 256, K = 64, windowed C (the only large-M cases)
HEADTAIL = [
    Case("headtail", "bias", 5, 129, 256, 64, "al", "headtail"), Case("headtail", "act", 5, 129, 256, 64, "l4", "headtail", act="quick_gelu"),
    Case("headtail", "resid", 5, 129, 256, 64, "a8", "headtail", ls=True, resid="in"), Case("headtail", "resid", 5, 77, 256, 64, "al", "headtail", resid="r8"),
    Case("headtail", "f32", 5, 129, 256, 64, "f4", "headtail"), Case("headtail", "bias", 5, 129, 256, 64, "al", "headtail", ln=True),
    Case("headtail", "vt", 5, 129, 256, 64, "al", "headtail"),
    # statistics across the split: the head's rows from its epilogue's partial sums, the tail's (stat_rt + m1, C + m1 * ldc) read back
    Case("headtail", "resid", 5, 129, 256, 64, "al", "headtail", ls=True, resid="in", stats="ln", dist="offset"),
    Case("headtail", "resid", 5, 77, 256, 64, "al", "headtail", resid="in", stats="rms", dist="plain"),
]

GROUPS = {"rowmajor": ROWMAJOR, "vt": VT, "f32": F32, "ln": LN, "rows": ROWS, "stats": STATS, "splitk": SPLITK, "headtail": HEADTAIL}
ALL_CASES = [c for g in GROUPS.values() for c in g]
STATS_EPS = 1e-6
OFFSET_MEAN = 16.0


def head_tail_rows(cus, case):
    """Rows of a head-plus-tail case on a device with `cus` CUs: N = 256 is one column tile, so one full round is `cus` row tiles of 256."""
    assert case.N == 256
    return cus * 256 + case.M


def phys_rows(case, M):
    if case.rows is None:
        return M
    p, s, f = case.rows
    return (M - 1) // p * s + (M - 1) % p + f + 1


def row_index(case, M):
    if case.rows is None:
        return torch.arange(M)
    p, s, f = case.rows
    r = torch.arange(M)
    return r // p * s + r % p + f


def make_inputs(case, M=None, seed=None):
    """Seeded operands of a case (CPU tensors): a [physical rows, K] bf16, w [N, K] bf16 (|acc| of order 2 whatever K), bias [N] fp32,
    resid [M, N] bf16 / ls [N] fp32 (never within 0.25 of 1), ln = (rt [physical rows, 2], s [N]) fp32."""
    M = case.M if M is None else M
    g = torch.Generator().manual_seed(ALL_CASES.index(case) + 1 if seed is None else seed)
    P = phys_rows(case, M)
    d = {"a": bf(torch.randn(P, case.K, generator=g)), "w": bf(torch.randn(case.N, case.K, generator=g) * (2.0 / math.sqrt(case.K))),
         "bias": torch.randn(case.N, generator=g), "resid": None, "ls": None, "ln": None}
    if case.kind == "resid":
        if case.stats:
            off = OFFSET_MEAN if case.dist == "offset" else 1.0
            d["resid"] = bf(off + (1.0 if case.dist == "offset" else 1.5) * torch.randn(M, case.N, generator=g))
        else:
            d["resid"] = bf(2.0 * torch.randn(M, case.N, generator=g))
        if case.ls:
            d["ls"] = 0.25 + 0.5 * torch.rand(case.N, generator=g)
    if case.ln:
        d["ln"] = (torch.stack([torch.rand(P, generator=g) * 1.5 + 0.5, torch.randn(P, generator=g)], dim=1), torch.randn(case.N, generator=g))
    return d


def reference_for(case, inp, M=None):
    """gemm_reference on the case's logical rows."""
    M = case.M if M is None else M
    idx = row_index(case, M)
    ln = None if inp["ln"] is None else (inp["ln"][0][idx], inp["ln"][1])
    return gemm_reference(case.kind, inp["a"].float()[idx], inp["w"].float(), inp["bias"], act=case.act,
                          resid=None if inp["resid"] is None else inp["resid"].float(), ls=inp["ls"], ln=ln)
