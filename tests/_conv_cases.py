"""Shared pieces of the 3x3 convolution contract tests (tests/test_host_conv_cases.py, tests/test_gpu_conv_contract.py): a float64 oracle with the
derived per-element bound of tests/_gemm_cases.py, index-exact integer inputs that need no tolerance at all, isolated (sentinel-surrounded)
inputs, weights and outputs, the dispatcher's route plan restated, and the case table.  Nothing here touches a GPU; every function works on
the device of the tensors it is given (the GPU tests run the oracle's float64 products on the device, the host tests on the CPU).

Operation.  x [B, H, W, C] and w [Cout, 3, 3, C] are bf16 (held in fp32 tensors), bias fp32, resid bf16.  nn.Conv2d(kernel 3) as the
entry points of include/visrep.h define it: stride 1 | 2; pad_mode 0 = padding 1 on every side, pad_mode 1 = F.pad(x, (0, 1, 0, 1)) and no
padding; up = the source is read through a nearest-neighbour 2x upsample (floor(i / 2)).  Output rows are tokens ((b Ho + oy) Wo + ox).
    BIAS y = bf16(acc + bias)      RESID y = bf16(resid + acc + bias)      F32 y = acc + bias (fp32)
Fused input GroupNorm (conv3x3_halo only): the operand is h = bf16(silu?(fma(x, scale, shift))) with (scale, shift) = table[b, c] (fp32) inside the
image and 0 outside it: Conv2d's padding pads the NORMALISED tensor.

Oracle (`conv_reference`): nine shifted strided slices of the explicitly padded float64 tensor, each multiplied with its tap's [Cout, C] matrix -
independent of every project kernel and of the im2col wrapper; the host test holds it to F.conv2d in float64 at every (stride, pad_mode, up).

Bound: `_gemm_cases.epilogue_reference` (the epilogue half of `gemm_reference`: U, TINY, the RESID terms and the output rounding live there and
are not restated) with K = 9 C products per output and mag = the same convolution of |x| with |w|.
  * split-K (csrc/gemm_bf16.hip, try_split_k): S = min(2 CUs / tiles, (K / 64) / 4) slices, lowered until it divides K / 64, so S <= K / 256:
    9 at K = 2304, 4 at K = 1152 (3 after the divisibility step).  The reduction adds the S planes in slice order: S - 1 <= 8 additions on top of
    the K - 1 inside the slices - what the factor K + 8 already counts at every K of this table (K <= 2304).  No widening.
  * conv3x3_c8 multiplies K = 96 columns per output (72 real products, 24 products with an exact zero): K = 96 in the factor.
  * fused GroupNorm: the oracle forms h in float64 from the same fp32 table and rounds it to bf16 itself (`bf16_round64`, round to nearest even
    on the float64 value - no intermediate fp32 rounding).  The device evaluates fma(x, scale, shift) in fp32 (one rounding; counted as two: 2 u
    (|x scale| + |shift|)) and, for SiLU, o * rcp(1 + exp2(o * -log2 e)): the quick_gelu analysis of _gemm_cases with c = log2 e - allowance
    2^-23 (4 + 3 |arg| (1 - sigma)) |y| + 2^-126 (1 + |t|), arg = t log2 e (`silu_allowance`), and the argument's error through the Lipschitz
    constant 1.1.  Where the float64 value lies within that evaluation error of a bf16 rounding tie, the device may round to the neighbour:
    an error of one ulp_bf16(h) of that operand, |w| ulp on every output it feeds.  The bound's accumulation error is widened per output by
    sum |w| ulp_bf16(h) over exactly those operands (`dacc`); `conv_reference` reports the share of outputs the widening touches.
Nothing in the bound depends on anything a GPU produced.

Index-exact inputs (`exact_inputs`).  Every pixel carries ONE nonzero channel c(b, y, x) with a value in {+-1, +-2}; weights are integers
w[co, ky, kx, c] = ((3 ky + kx) + off(co, c)) mod 15 - 7 in [-7, 7]: the nine taps of a (co, c) pair take nine DIFFERENT values, so no two taps
and no ky / kx transpose agree.  |acc| <= 9 * 2 * 7 = 126, bias and residual are integers of magnitude <= 64: every output is an integer of
magnitude <= 254, every partial sum an integer below 2^24 - exact in fp32 under ANY summation order and exact in bf16.  The device result
must EQUAL the integer result.  Exact fused norm (silu = 0): scale[c] in {+-1, +-2, 0.5} and the pixel's value chosen so that |x scale| <= 2
(scale +-2: x = +-1; scale 0.5: x = +-2 - 0.5 times an even value), shift an integer != 0 for EVERY channel.  h = x scale + shift is an exact
integer for all 128 channels of every pixel, so that the sum stays small the shifts of a channel pair (2 p, 2 p + 1) are (+s_p, -s_p) and the
pair shares its weights (off(co, c >> 1)) - the shifts of an in-image pixel cancel exactly - except pair 0, whose shifts are (2, -1): every
in-image tap adds w[co, tap, 0] and a kernel that normalises the zero padding (or pads before normalising) adds it for the padded taps too.
The host test asserts the magnitude limit on the computed outputs of every fused-norm case and every case of at most 4096 rows (without
the fused norm it holds by construction: 126 + 64 + 64).

Isolation.  Outputs (and an out-of-place residual) live in `_gemm_cases.make_window` buffers pre-filled with the NaN sentinel; the input tokens
sit in the middle of a sentinel buffer with at least (W + 2) C elements of NaN on both sides (`isolate`): a gather that reads one pixel row
before image 0 or past image B - 1 turns a border output into NaN; weights have ldw = 9 C + 8 with NaN padding columns.  conv3x3_c8 reads
K = 96 columns: 72 .. 95 must be zero (include/visrep.h) and are, columns >= 96 are NaN, and the token's channels 3 .. 7 are zero over finite
nonzero weights.
"""
import math
import zlib
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F

import _gemm_cases as GC
from _gemm_cases import SENTINEL, TINY, U, WINDOWS, make_window, round_up, stray_writes  # noqa: F401  (re-exported to the tests)

LOG2E = math.log2(math.e)
GEOMS = ((1, 0, 0), (2, 0, 0), (2, 1, 0), (1, 0, 1))          # (stride, pad_mode, up): every combination the towers use
KIND_OF_EPI = ("bias", "resid", "f32")


def bf(x):
    return x.to(torch.bfloat16)


def out_hw(H, W, stride, pad_mode, up):
    """Conv2d's output size: floor((H_logical + pad_total - 3) / stride) + 1."""
    Hl, Wl, pt = H << up, W << up, (2 if pad_mode == 0 else 1)
    return (Hl + pt - 3) // stride + 1, (Wl + pt - 3) // stride + 1


# ------------------------------------------------------------------------------------------------ the oracle
def _padded(x, pad_mode, up):
    """x [B, H, W, C] -> the tensor Conv2d(padding = 0) would see."""
    if up:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return F.pad(x, (0, 0, 1, 1, 1, 1)) if pad_mode == 0 else F.pad(x, (0, 0, 0, 1, 0, 1))


def conv64(x, w, stride, pad_mode, up):
    """Nine shifted slices: [B Ho Wo, Cout] float64 of x [B, H, W, C] with w [Cout, 3, 3, C] (both float64, any device)."""
    xp = _padded(x, pad_mode, up)
    B, Hp, Wp, C = xp.shape
    Ho, Wo = (Hp - 3) // stride + 1, (Wp - 3) // stride + 1
    out = torch.zeros(B * Ho * Wo, w.shape[0], dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            sl = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :]
            out += sl.reshape(-1, C) @ w[:, ky, kx, :].t()
    return out


def bf16_round64(v):
    """float64 -> the nearest bf16 value (ties to even), as float64: one rounding, straight from the float64 value."""
    m, e = torch.frexp(v)                                      # |v| in [2^(e-1), 2^e): bf16 spacing 2^(e-8)
    q = torch.ldexp(torch.ones_like(v), e - 8)
    return torch.round(v / q) * q                              # v / q is exact (a power of two), torch.round rounds half to even


def ulp_bf16(v):
    _, e = torch.frexp(v)
    return torch.ldexp(torch.ones_like(v), e - 8)


def silu_allowance(t):
    """|device SiLU formula in fp32 - t sigmoid(t)| at the exact argument t: `_gemm_cases.act_allowance('quick_gelu')` with c = log2 e."""
    t = t.double()
    y = (t * torch.sigmoid(t)).abs()
    arg = LOG2E * t
    return 2.0 ** -23 * (4.0 + 3.0 * arg.abs() * torch.sigmoid(-arg * math.log(2.0))) * y + TINY * (1.0 + t.abs())


def silu_device_formula_fp32(o):
    """conv3x3_halo / groupnorm_apply_rows: o * rcp(1 + exp2(o * -log2 e)) evaluated in fp32 on the CPU."""
    o = o.float()
    return o * torch.reciprocal(1.0 + torch.exp2(o * torch.tensor(-1.4426950408889634, dtype=torch.float32)))


def gn_operand64(x, gn):
    """(h, flip): h [B, H, W, C] float64 = bf16(silu?(x scale + shift)) formed in float64 from the fp32 table; flip = ulp_bf16(h) where the
    float64 value lies within the fp32 evaluation error of a rounding tie (the device may hold the neighbouring bf16 value), else 0."""
    table, silu = gn
    sc, sh = table[..., 0].double()[:, None, None, :], table[..., 1].double()[:, None, None, :]
    t = x * sc + sh
    dt = 2 * U * ((x * sc).abs() + sh.abs())
    if silu:
        v, dv = t * torch.sigmoid(t), 1.1 * dt + silu_allowance(t)
    else:
        v, dv = t, dt
    h = bf16_round64(v)
    q = ulp_bf16(v)
    frac = v / q - torch.floor(v / q)
    near = ((frac - 0.5).abs() * q <= dv) & (v != 0)
    return h, torch.where(near, q, torch.zeros_like(q))


def conv_parts(x, w, *, stride=1, pad_mode=0, up=0, gn=None, report=None):
    """(acc, mag, dacc): the float64 accumulation, the same sum of magnitudes and the tie widening (None without a fused norm) - everything of the
    reference that does not depend on the epilogue, so that cases which share their operands share it."""
    X, W = x.double(), w.double()
    dacc = None
    if gn is not None:
        X, flip = gn_operand64(X, gn)
        dacc = conv64(flip, W.abs(), stride, pad_mode, up)
        if report is not None:
            report["widened"] = (dacc > 0).double().mean().item()
            report["operands"] = (flip > 0).double().mean().item()
    return conv64(X, W, stride, pad_mode, up), conv64(X.abs(), W.abs(), stride, pad_mode, up), dacc


def conv_reference(kind, x, w, bias, *, stride=1, pad_mode=0, up=0, resid=None, gn=None, K=None, report=None):
    """(want, bound) [B Ho Wo, Cout] in float64.  x [B, H, W, C], w [Cout, 3, 3, C]: fp32 tensors holding bf16 values; bias [Cout] fp32 or None;
    resid [B Ho Wo, Cout] holding bf16 values (kind 'resid'); gn = (table [B, C, 2] fp32, silu) or None; K: products per output where the
    kernel pads them (conv3x3_c8: 96), default 9 C.  report: a dict that receives 'widened' (share of outputs the tie widening touches) and
    'operands' (share of operands near a tie)."""
    assert kind in KIND_OF_EPI
    acc, mag, dacc = conv_parts(x, w, stride=stride, pad_mode=pad_mode, up=up, gn=gn, report=report)
    return GC.epilogue_reference(kind, acc, mag, 9 * x.shape[3] if K is None else K, bias, resid=resid if kind == "resid" else None, dacc=dacc)


def arithmetic_bound(kind, want, bound):
    return GC.arithmetic_bound(kind, want, bound)


def im2col_index_oracle(x, stride, pad_mode, up, ld):
    """The pure gather: [B Ho Wo, ld] with column (3 ky + kx) C + c = x[b, oy stride + ky - pad, ox stride + kx - pad, c], zero outside the image
    and in columns [9 C, ld).  x [B, H, W, C] of any dtype; nothing is computed, so the result is bit-exact."""
    xp = _padded(x, pad_mode, up)
    B, Hp, Wp, C = xp.shape
    Ho, Wo = (Hp - 3) // stride + 1, (Wp - 3) // stride + 1
    cols = [xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :].reshape(-1, C) for ky in range(3) for kx in range(3)]
    out = torch.zeros(B * Ho * Wo, ld, dtype=x.dtype, device=x.device)
    out[:, :9 * C] = torch.cat(cols, dim=1)
    return out


# ------------------------------------------------------------------------------------------------ index-exact inputs
def _grid(B, H, W):
    b = torch.arange(B)[:, None, None]
    y = torch.arange(H)[None, :, None]
    x = torch.arange(W)[None, None, :]
    return b, y, x


def exact_channel(B, H, W, C, live=None):
    """c(b, y, x): the one nonzero channel of each pixel.  Along y (x fixed) the 16-byte chunk c >> 3 steps by one, so sixteen rows put a nonzero
    into every chunk at every x - hence at every halo x-position; the position inside the chunk varies with (x, y, b).  live: only channels
    [0, live) are used (conv3x3_c8: 3 of the token's 8)."""
    b, y, x = _grid(B, H, W)
    if live is not None:
        return (x + 2 * y + b) % live + 0 * (b + y + x)
    return (8 * (y + 5 * x) + (3 * x + y + b) % 8) % C + 0 * b


def exact_scale_shift(B, C, seed):
    """The exact fused-norm table [B, C, 2]: scale in {1, -1, 2, -2, 0.5}, shift = (+s_p, -s_p) per channel pair, (2, -1) for pair 0."""
    c = torch.arange(C)
    tab = torch.zeros(B, C, 2)
    for b in range(B):
        scale = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5])[(c * 3 + b + seed) % 5]
        s = (1 + ((c >> 1) + b + seed) % 3).float()
        shift = torch.where(c % 2 == 0, s, -s)
        shift[0], shift[1] = 2.0, -1.0
        tab[b, :, 0], tab[b, :, 1] = scale, shift
    return tab


def exact_inputs(B, H, W, C, Cout, seed, *, M_out=None, gn=False, live=None):
    """Integer data (module docstring): dict of x [B, H, W, C], w [Cout, 3, 3, C], bias [Cout], resid [M_out, Cout] (when M_out is given) as fp32
    tensors, and table [B, C, 2] for the exact fused norm (gn=True, C = 128)."""
    ch = exact_channel(B, H, W, C, live)
    b, y, x = _grid(B, H, W)
    val = torch.tensor([1.0, -1.0, 2.0, -2.0])[(x + 2 * y + 3 * b + seed) % 4]
    d = {"table": None, "resid": None}
    if gn:
        d["table"] = exact_scale_shift(B, C, seed)
        sc = torch.gather(d["table"][..., 0], 1, ch.reshape(B, -1)).reshape(B, H, W)
        sign = torch.sign(val)
        val = torch.where(sc.abs() == 2.0, sign, torch.where(sc.abs() == 0.5, 2.0 * sign, val))      # |x scale| <= 2, and an integer
    X = torch.zeros(B, H, W, C)
    X.scatter_(3, ch[..., None], val[..., None])
    co = torch.arange(Cout)[:, None, None]
    t = torch.arange(9)[None, :, None]
    c = torch.arange(C)[None, None, :]
    cw = (c >> 1) if gn else c                                  # exact fused norm: a channel pair shares its weights (its shifts cancel)
    off = (co * 7 + cw * 11 + seed) % 15
    d["x"] = X
    d["w"] = (((t + off) % 15) - 7).float().reshape(Cout, 3, 3, C)
    d["bias"] = ((torch.arange(Cout) * 37 + seed) % 129 - 64).float()
    if M_out is not None:
        m = torch.arange(M_out)[:, None]
        d["resid"] = ((m * 13 + torch.arange(Cout)[None, :] * 29 + seed) % 129 - 64).float()
    return d


def random_inputs(B, H, W, C, Cout, seed, *, M_out=None, gn=False, live=None):
    """Seeded bf16-valued operands: |acc| of order 2 whatever C; table = a plausible (rstd gamma, beta - mean rstd gamma)."""
    g = torch.Generator().manual_seed(seed)
    x = bf(torch.randn(B, H, W, C, generator=g)).float()
    if live is not None:
        x[..., live:] = 0.0
    n_live = C if live is None else live
    d = {"x": x, "w": bf(torch.randn(Cout, 3, 3, C, generator=g) * (2.0 / math.sqrt(9 * n_live))).float(),
         "bias": torch.randn(Cout, generator=g), "resid": None, "table": None}
    if M_out is not None:
        d["resid"] = bf(2.0 * torch.randn(M_out, Cout, generator=g)).float()
    if gn:
        d["table"] = torch.stack([0.5 + torch.rand(B, C, generator=g) * 1.5, torch.randn(B, C, generator=g)], dim=2)
    return d


# ------------------------------------------------------------------------------------------------ isolation
def sentinel_fill(shape, dtype, device="cpu"):
    idt, pat = SENTINEL[dtype]
    return torch.full(shape, pat, dtype=idt, device=device).view(dtype)


def isolate(tokens, guard):
    """(buf, view): the token matrix [M, C] in the middle of a 1-D sentinel buffer with `guard` (>= (W + 2) C, rounded up to 64 elements so that
    the view stays 128-byte aligned) elements of NaN on both sides."""
    guard = round_up(guard, 64)
    M, C = tokens.shape
    buf = sentinel_fill((guard + M * C + guard,), tokens.dtype, tokens.device)
    view = buf[guard:guard + M * C].view(M, C)
    view.copy_(tokens)
    return buf, view


def pack_weights(w, ldw, zero_to=None):
    """w [Cout, 3, 3, C] -> [Cout, ldw] bf16 in K order (ky, kx, c); columns [9 C, zero_to) zero, the rest of the padding the NaN sentinel."""
    Cout, K = w.shape[0], 9 * w.shape[3]
    out = sentinel_fill((Cout, ldw), torch.bfloat16, w.device)
    out[:, :K] = bf(w.reshape(Cout, K))
    if zero_to is not None:
        out[:, K:zero_to] = 0
    return out


# ------------------------------------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    route: str                     # '128' | '128gn' | 'splitk' | '256' | '256tail' | 'c8' | 'halo': what must run (asserted from _lib.routes())
    B: int
    H: int
    W: int
    C: int
    Cout: int
    kind: str = "bias"             # bias | resid | f32
    geom: tuple = (1, 0, 0)        # (stride, pad_mode, up)
    win: str = "c"                 # window class of the output (and of an out-of-place residual), _gemm_cases.WINDOWS
    variant: int = 5               # visrep_set_gemm_variant
    cus: Optional[int] = None      # run with this many CUs left (reserved_cus), None = the whole device
    tile: int = 16                 # conv3x3_halo tile height
    gn: Optional[str] = None       # halo: None | 'tab' (exact mode: the exact table, silu = 0; bound mode: a random table with `silu`)
    silu: int = 1
    groups: int = 0                # GroupNorm partial sums of the OUTPUT requested with this many groups: must not change a bit of the output

    @property
    def M(self):
        Ho, Wo = out_hw(self.H, self.W, *self.geom)
        return self.B * Ho * Wo

    @property
    def K(self):
        return 96 if self.route == "c8" else 9 * self.C

    @property
    def id(self):
        s, p, u = self.geom
        parts = [self.route, f"{self.B}x{self.H}x{self.W}x{self.C}-{self.Cout}", self.kind, f"s{s}p{p}u{u}", self.win]
        if self.route in ("128", "128gn", "splitk", "256", "256tail"):
            parts.append(f"v{self.variant}")
        if self.route == "halo":
            parts += [f"t{self.tile}", ("gn_silu" if self.silu else "gn_lin") if self.gn else "nogn"]
        if self.groups:
            parts.append(f"g{self.groups}")
        if self.cus:
            parts.append(f"cus{self.cus}")
        return "-".join(parts)


def _rot(seq, i):
    return seq[i % len(seq)]


# 128 x 128 kernel, C = 64 (K = 576: never split).  M = 70 is below one tile; at 243 = 3 x 81 the image changes inside a tile and inside a lane's
# four staged rows; Cout = 192 leaves the second column tile half empty.  Every shape meets every geometry; epilogue, window class and variant rotate
# so that each shape meets each epilogue, and each (epilogue, variant) pair and each window class the ABI accepts (ldc % 4 == 0: c, al, a8, l4;
# fp32: c, f4) occurs (asserted by the host test); it is not the full cross.
SHAPES_128 = ((2, 5, 7, 64), (3, 9, 9, 128), (1, 13, 10, 192))
CASES_128 = []
for _i, (_sh, _g) in enumerate((s, g) for s in SHAPES_128 for g in GEOMS):
    _kind = _rot(KIND_OF_EPI, _i + _i // 3)
    _win = _rot(("f4", "c"), _i) if _kind == "f32" else _rot(("al", "a8", "c", "l4"), _i)
    CASES_128.append(Case("128", _sh[0], _sh[1], _sh[2], 64, _sh[3], _kind, _g, _win, _rot((1, 5), _i // 2)))
CASES_128 += [Case("128", 3, 9, 9, 64, 128, "resid", (1, 0, 0), "l4", 1), Case("128", 1, 13, 10, 64, 192, "f32", (2, 1, 0), "f4", 5),
              Case("128", 2, 5, 7, 64, 64, "bias", (1, 0, 1), "a8", 1), Case("128", 2, 5, 7, 64, 64, "resid", (2, 1, 0), "al", 5)]
# the _gn entry on a shape that passes visrep_conv_gn_supported (Ho Wo = 128, 4 channels per group): bitwise the plain call's output
CASES_128GN = [Case("128gn", 2, 8, 16, 64, 64, "bias", (1, 0, 0), "al", 5, groups=16), Case("128gn", 2, 8, 16, 64, 64, "resid", (1, 0, 0), "c", 1, groups=16)]

# split-K: K = 1152 and 2304 (the SAM neck's width), few tiles, scratch registered
CASES_SPLITK = [
    Case("splitk", 2, 6, 6, 128, 64, "bias", (1, 0, 0), "al"), Case("splitk", 1, 12, 20, 128, 128, "resid", (1, 0, 0), "a8"),
    Case("splitk", 2, 6, 6, 256, 128, "f32", (1, 0, 0), "f4"), Case("splitk", 1, 12, 20, 256, 256, "bias", (1, 0, 0), "l4"),
    Case("splitk", 1, 12, 20, 128, 64, "f32", (2, 1, 0), "c"), Case("splitk", 2, 6, 6, 256, 64, "resid", (2, 1, 0), "al"),
    Case("splitk", 1, 12, 20, 256, 256, "resid", (2, 1, 0), "c"),
]

# 256 x 256 persistent kernel: with 64 CUs two rounds are 128 tiles = 32768 rows at Cout = 256.  182 x 182 = 33124 rows = 130 tiles (129.4): the
# last 356 rows (33124 - 32768; 33124 % 256 = 100) go to a 128 x 128 tail launch that carries the row offset 32768.  257 x 257 at stride 2, pad_mode 1
# gives 128 x 128 outputs from odd H and W.  At the full CU count the first shape has 128 < 512 tiles and must fall back to the 128 x 128 kernel.
CASES_256 = [
    Case("256", 2, 128, 128, 64, 256, "bias", (1, 0, 0), "al", cus=64), Case("256", 2, 128, 128, 64, 256, "resid", (1, 0, 0), "a8", cus=64),
    Case("256tail", 1, 182, 182, 64, 256, "resid", (1, 0, 0), "al", cus=64), Case("256tail", 1, 182, 182, 64, 256, "bias", (1, 0, 0), "l4", cus=64),
    Case("256", 2, 257, 257, 64, 256, "bias", (2, 1, 0), "c", cus=64), Case("256", 2, 257, 257, 64, 256, "resid", (2, 1, 0), "al", cus=64),
    Case("128", 2, 128, 128, 64, 256, "bias", (1, 0, 0), "al"),
]

# conv3x3_c8: 64 pixels that all lie on a border, then an image change, a wider row, more than one workgroup.  ldc % 8 is required (refusal
# tested); an 8-byte aligned window (a8) is served by the shared epilogue's narrow stores.
CASES_C8 = [
    Case("c8", 1, 4, 16, 8, 128, "bias", win="c"), Case("c8", 1, 4, 16, 8, 128, "bias", win="al"), Case("c8", 2, 8, 16, 8, 128, "bias", win="al", groups=32),
    Case("c8", 3, 4, 32, 8, 128, "bias", win="c", groups=32), Case("c8", 3, 4, 32, 8, 128, "bias", win="a8"), Case("c8", 1, 16, 48, 8, 128, "bias", win="al", groups=16),
]

# conv3x3_halo: one tile with all four borders; two tiles sharing an edge + an image change (both orientations); an interior tile; and, with 64 CUs,
# 3 x 80 x 80 = 75 tiles against a cap of 64 (150 against 128 at tile height 8): a workgroup walks more than one tile.  Tile height 8 exists for
# Cout = 128 only.
SHAPES_HALO = ((1, 16, 16), (2, 16, 32), (2, 32, 16), (1, 48, 48))
HALO_KERNELS = ((128, 16), (128, 8), (256, 16))                # (Cout, tile height)
HALO_TABLES = ((None, 1), ("tab", 0), ("tab", 1))               # no table | a table without SiLU | a SiLU table (exact mode: the exact table, silu = 0)
# the full cross: shape (the four above and, with 64 CUs, 3 x 80 x 80) x kernel x fused norm x epilogue.  EVERY case asks for the output's partial
# sums (32 groups) and re-runs the plain call (groups = 0), which must give the same bits; the window class alternates.  Cases that share their
# operands (same shape, Cout and table) are neighbours, so that the GPU test computes their float64 accumulation once.
CASES_HALO = [Case("halo", _sh[0], _sh[1], _sh[2], 128, _co, _kind, (1, 0, 0), _rot(("al", "c"), _n + _k), tile=_t, gn=_gn, silu=_silu, groups=32,
                   cus=64 if _sh == (3, 80, 80) else None)
              for _n, _sh in enumerate(SHAPES_HALO + ((3, 80, 80),)) for (_co, _t) in HALO_KERNELS for (_gn, _silu) in HALO_TABLES
              for _k, _kind in enumerate(("bias", "resid"))]

def data_key(case):
    """What a case's operands depend on: cases with the same key get the same x, w, bias, residual and table, whatever their epilogue, window,
    variant or kernel - so they can share the accumulation half of the reference."""
    return ("c8" if case.route == "c8" else "conv", case.B, case.H, case.W, case.C, case.Cout, case.geom, case.gn is not None)


def _neighbours(cases):
    """The same cases, those that share their operands next to each other (stable: in the order of each key's first case)."""
    first = {}
    for i, c in enumerate(cases):
        first.setdefault(data_key(c), i)
    return sorted(cases, key=lambda c: first[data_key(c)])


CASES_128, CASES_256, CASES_HALO = _neighbours(CASES_128), _neighbours(CASES_256), _neighbours(CASES_HALO)
GROUPS = {"128": CASES_128, "128gn": CASES_128GN, "splitk": CASES_SPLITK, "256": CASES_256, "c8": CASES_C8, "halo": CASES_HALO}
ALL_CASES = [c for g in GROUPS.values() for c in g]

# im2col3x3 alone: C x ld x shape x geometry, bit-exact
IM2COL_CASES = [(C, ld_pad, sh, g) for C in (8, 64) for ld_pad in (False, True) for sh in ((2, 5, 7), (1, 13, 10)) for g in GEOMS]


def seed_of(case):
    """A stable hash of the data key: adding a case to the table moves nobody else's operands (nor the recorded worst ratios)."""
    return zlib.crc32(repr(data_key(case)).encode()) & 0x7FFFFFFF


def window_of(case):
    extra, col0 = WINDOWS[case.win]
    return case.Cout + extra, col0


def inputs_for(case, mode):
    """mode 'exact' | 'bound' -> (inputs dict, gn argument of conv_reference or None, silu flag handed to the kernel).  A function of
    (data_key, mode) only; the residual is always built and used by the RESID cases."""
    use_gn = case.gn is not None
    live = 3 if case.route == "c8" else None
    build = exact_inputs if mode == "exact" else random_inputs
    d = build(case.B, case.H, case.W, case.C, case.Cout, seed_of(case), M_out=case.M, gn=use_gn, live=live)
    silu = 0 if mode == "exact" else case.silu
    return d, ((d["table"], silu) if use_gn else None), silu


def parts_for(case, d, gn, device="cpu", report=None):
    s, p, u = case.geom
    return conv_parts(d["x"].to(device), d["w"].to(device), stride=s, pad_mode=p, up=u, gn=None if gn is None else (gn[0].to(device), gn[1]), report=report)


def finish_reference(case, d, parts):
    """(want, bound) of the case's epilogue on shared parts (on the parts' device)."""
    acc, mag, dacc = parts
    resid = d["resid"].to(acc.device) if case.kind == "resid" else None
    return GC.epilogue_reference(case.kind, acc, mag, case.K, d["bias"].to(acc.device), resid=resid, dacc=dacc)


def reference_for(case, d, gn, device="cpu", report=None):
    return finish_reference(case, d, parts_for(case, d, gn, device, report))


# ------------------------------------------------------------------------------------------------ the dispatcher's plan
ROUTE_KEYS = ("gemm_256", "gemm_128", "gemm_tail", "splitk", "conv_256", "conv_128", "conv_128_gn", "conv_halo", "conv_c8")


def split_k_slices(M, N, K, cus):
    """try_split_k of csrc/gemm_bf16.hip with a registered scratch: the number of slices, 0 = not split."""
    tiles = -(-M // 128) * -(-N // 128)
    if K < 1024 or N % 4 or tiles >= 2 * cus:
        return 0
    kt = K // 64
    S = min(2 * cus // tiles, kt // 4)
    while S > 1 and kt % S:
        S -= 1
    return S if S > 1 else 0


def route_plan(case, cus, gn_entry=False):
    """{counter: launches} of one call, from visrep_gemm_dispatch / dispatch_one / try_split_k restated (scratch registered, variants 1 and 5).
    csrc/gemm_bf16.hip points here: the two change together."""
    r = dict.fromkeys(ROUTE_KEYS, 0)
    if case.route in ("c8", "halo"):
        r["conv_" + case.route] = 1
        return r
    M, N, K = case.M, case.Cout, 9 * case.C
    s, p, u = case.geom
    Wo = out_hw(case.H, case.W, s, p, u)[1]
    c128 = "conv_128_gn" if gn_entry else "conv_128"
    if not gn_entry and split_k_slices(M, N, K, cus):
        r["splitk"] = 1
        return r
    conv5 = case.variant >= 5 and N % 256 == 0 and case.C % 64 == 0 and not u and Wo >= 8 and case.kind in ("bias", "resid")
    one = lambda m: "conv_256" if conv5 and -(-m // 256) * (N // 256) >= 2 * cus else c128
    if case.variant >= 2 and N % 256 == 0 and conv5:
        ntn, ntm = N // 256, -(-M // 256)
        tiles = ntm * ntn
        rounds, rem = tiles // cus, tiles % cus
        if rounds >= 1 and rem > 0 and rem * 4 <= cus and (rounds * cus) % ntn == 0:
            m1 = rounds * cus // ntn * 256
            if 0 < m1 < M:
                r[one(m1)] += 1
                r["gemm_tail"] = 1
                if not gn_entry and split_k_slices(M - m1, N, K, cus):
                    r["splitk"] = 1
                else:
                    r[c128] += 1
                return r
    r[one(M)] = 1
    return r


EXPECTED = {"128": {"conv_128": 1}, "128gn": {"conv_128_gn": 1}, "splitk": {"splitk": 1}, "256": {"conv_256": 1},
            "256tail": {"conv_256": 1, "conv_128": 1, "gemm_tail": 1}, "c8": {"conv_c8": 1}, "halo": {"conv_halo": 1}}


def expected_routes(case):
    """What the case NAMES: the counters of one call of its main entry (every other counter 0)."""
    r = dict.fromkeys(ROUTE_KEYS, 0)
    r.update(EXPECTED[case.route])
    return r
