"""Every persistent kernel at CU counts other than 256 (VISREP_RESERVE_CUS / visrep_set_reserved_cus).

The dispatchers size their grids, their head / tail splits, the split-K slice count and the convolution routes from visrep_cu_count();
a reservation of k CUs makes that 256 - k.  Which block computes a tile must never show in a result, so every case here is held to
  1. the bar of the existing test of the same operation against a reference that does not come from the library (float64 on the CPU from the
     bf16-rounded inputs; torch fp32 on the device only where a test says so), at k = 0 and at every other k, and
  2. bitwise equality with the k = 0 result wherever the decomposition is the same - decided from the route counters around the call
     (_lib.routes): equal counts of every GEMM / convolution route and no tail launch or split-K in either run.  Where a hand-written table
     pins the split point (GEMM_PLAN), two runs that split at the same row are compared bitwise as well.
Where the decomposition differs the route deltas are asserted from hand-written tables (evaluated by hand from the rule in
csrc/gemm_bf16.hip, visrep_gemm_dispatch), so a head / tail decision is pinned and not only tolerated.

k = 0, 8, 16, 64, 128, 192 -> 256, 248, 240, 192, 128, 64 CUs; k = 200 is ignored (fewer than 64 CUs would remain), k = 13 rounds down to 8.

Every result lands in a NaN-filled buffer (poisoned(); zero-filled where the contract is "the rest stays zero", as for V^T): a tile that a
persistent block skips at some grid size fails both assertions instead of showing what an earlier call left in a recycled allocation.

Worst measured error per family on an MI355X (max |got - want| / max |want| unless said otherwise) is in each test's docstring as
`worst: ... (k = 0: ...)`; every test prints its figures and its bitwise / by-tolerance (case, k) lists (`[cu-counts]` lines, pytest -s).
The worst error of every family is reached at k = 0 already: no case needs a wider bar than its existing counterpart.

Which (case, k) are compared how (CUs in brackets; "split" = head on the 256x256 kernel + 128x128 tail, routes gemm_256 + gemm_128 + gemm_tail):
  GEMM v5, all five epilogues  bitwise: 4000 x 1024 and 256 x 256 at every k; 65201 x 1024 at 64, 128, 192, 200; 36928 x 4096 at 64, 128, 192, 200
                               (same split row 36864); 16717 x 1024 at 128, 192, 200 (16384); 10243 x 2048 and 4685 x 1024 at all but 192;
                               70000 x 256 at 128, 200 (65536).
                               by tolerance: 65201 x 1024 at 8, 13 (split 63488), 16 (61440); 36928 x 4096 at 8, 13, 16 (whole: gemm_256 only);
                               16717 x 1024 at 8, 13 (15872), 16 (15360), 64 (whole); 10243 x 2048 at 192 (split 10240, a 3-row tail); 4685 x 1024
                               at 192 (4096); 70000 x 256 at 8, 13 (63488), 16 (61440), 64 and 192 (whole).
  GEMM v2                      as v5 on 16717 x 1024 and 4000 x 1024 (BIAS, ACT, RESID, VT).
  duo 6 / 7 / 8                16717 x 1024: bitwise at 192 (16384), by tolerance at 16 (15360); 10243 x 2048: bitwise at 16, by tolerance at 192 (10240).
  LN fold, row map, statistics bitwise at 192 (split 16384 as at k = 0), by tolerance at 16 (15360).
  walk codes                   every (k, code) bitwise.
  split-K                      by tolerance at every k (route splitk); bitwise run to run, and k = 200 == 0, 13 == 8.
  conv3x3 (+ GroupNorm sums)   8 x 128 x 160: bitwise at every k (conv_256); 2 x 128 x 128: bitwise (conv_128) but 192 (conv_256, by tolerance);
                               4 x 192 x 192: k = 0 and 200 conv_256 + 128x128 tail, every other k one conv_256 launch (by tolerance).
  conv3x3_halo, A score        every (shape, k) bitwise.

Not reachable through the ABI, hence not here: variant 5 with K % 64 != 0 (the dispatcher refuses K % 64 != 0 before any kernel is chosen);
the v2 kernel is reached through variant 2."""
import contextlib
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _hostile_gn_cases as HC  # noqa: E402
from test_oracle_golden import load_sd_case, load_vit_hip_case  # noqa: E402

from law_of_vision_representation_in_mllms_amd import _lib, ascore_ops, engine, sd_engine as SE  # noqa: E402
from law_of_vision_representation_in_mllms_amd import vit_weights as VW  # noqa: E402
from oracle import ascore as OA, diffusion as OD, vit as OV  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

KS = (0, 8, 16, 64, 128, 192, 200, 13)
CUS = {0: 256, 8: 248, 16: 240, 64: 192, 128: 128, 192: 64, 200: 256, 13: 248}
DECOMP = ("gemm_256", "gemm_128", "gemm_tail", "splitk", "conv_256", "conv_128", "conv_128_gn", "conv_halo")


@pytest.fixture
def reserved_cus():
    """reserved_cus(k): a context in which k CUs are reserved - the library reports 256 - k (or 256 where the never-below-64 floor applies, or
    the next multiple of 8 below k) before the body runs, and the previous reservation is back afterwards.  The setting is process-wide: the
    fixture also puts back the walk, GEMM variant, A-score variant and halo tile of the test's start, whatever the test did to them."""
    lib = _lib.require_gpu()
    start = lib.visrep_set_reserved_cus(0)
    lib.visrep_set_reserved_cus(start)
    walk = lib.visrep_set_gemm_walk(0)
    variant = lib.visrep_set_gemm_variant(5)
    lib.visrep_set_gemm_variant(variant)
    asv = lib.visrep_set_ascore_variant(0)
    lib.visrep_set_ascore_variant(asv)
    tile = lib.visrep_set_conv_halo_tile(16)
    lib.visrep_set_conv_halo_tile(tile)

    @contextlib.contextmanager
    def ctx(k):
        old = lib.visrep_set_reserved_cus(k)
        try:
            assert lib.visrep_device_cu_count() == CUS[k], (k, lib.visrep_device_cu_count())
            yield CUS[k]
            torch.cuda.synchronize()
        except BaseException:
            lib.visrep_set_reserved_cus(old)                     # restore unconditionally; the body's own error is the one to report
            raise
        assert lib.visrep_set_reserved_cus(old) == max(k, 0) // 8 * 8
    try:
        yield ctx
    finally:
        lib.visrep_set_reserved_cus(start)
        lib.visrep_set_gemm_walk(walk)
        lib.visrep_set_gemm_variant(variant)
        lib.visrep_set_ascore_variant(asv)
        lib.visrep_set_conv_halo_tile(tile)
        assert lib.visrep_device_cu_count() == (256 - start if 256 - start >= 64 else 256)


def bf(x):
    return x.to(torch.bfloat16)


def max_err(got, want):
    """max |got - want| / max |want| in float64 on the device (`want` is the float64 reference)."""
    want = want.to(DEV)
    return ((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()


def rel_err(got, want):
    want = want.to(DEV)
    return ((got.double() - want).norm() / want.norm().clamp_min(1e-300)).item()


def poisoned(*shape, dtype=torch.bfloat16):
    """An output buffer full of NaN.  Every result buffer of this file is one (or torch.zeros where the kernel's contract is "the rest stays
    zero"): a fresh torch.empty block is usually the block an earlier call of the same case freed, correct values included, and a tile that a
    persistent block skipped at another grid size would read as computed."""
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def routed(fn):
    """(fn(), route deltas of the call)."""
    _lib.routes(reset=True)
    out = fn()
    torch.cuda.synchronize()
    r = _lib.routes(reset=True)
    return out, {k: r[k] for k in DECOMP}


def same_decomposition(r, r0):
    return r == r0 and r["gemm_tail"] == 0 and r["splitk"] == 0


def equal(a, b):
    if isinstance(a, (tuple, list)):
        return all(equal(x, y) for x, y in zip(a, b))
    return torch.equal(a, b)


def perm16(m):
    """Column of token m in the attention kernel's V^T layout: the two middle 4-token groups of every aligned 16 swap (csrc/attention.hip)."""
    return (m & ~15) | (((m >> 2) & 1) << 3) | (((m >> 3) & 1) << 2) | (m & 3)


def vt_layout(want_mn, ld):
    """[M, N] float64 -> the V^T buffer [N, ld] the EPI_VT epilogue writes; every other column is zero."""
    M, N = want_mn.shape
    out = torch.zeros(N, ld, dtype=torch.float64, device=want_mn.device)
    out[:, perm16(torch.arange(M, device=want_mn.device))] = want_mn.t()
    return out


def vt_defined(got, M):
    """The V^T buffer without the columns the epilogue leaves undefined: it stores four consecutive tokens at a time (csrc/gemm_epilogue.h), so the
    columns of tokens M .. the next multiple of 4 hold the bias-only product of the zero rows past M.  Attention never reads them (keys >= M are
    masked); here they are zeroed before the comparison with the reference, and they ARE part of every bitwise comparison between two k."""
    pad = torch.arange(M, (M + 3) // 4 * 4, device=got.device)
    if pad.numel() == 0:
        return got
    got = got.clone()
    got[:, perm16(pad)] = 0
    return got


class Tally:
    """Per family: which (case, k) were bitwise, which by tolerance only, the worst error at k = 0 and at any k."""

    def __init__(self, name):
        self.name, self.bitwise, self.tol, self.err0, self.err = name, {}, {}, 0.0, 0.0

    def sweep(self, case, ks, reserved_cus, call, check, plan=None, expect=None):
        """call() at every k of ks (k = 0 first); check(out) -> error (asserts its bar); plan: {cus: ("whole",) | ("split", m1)};
        expect(plan entry) -> route deltas."""
        out0 = r0 = None
        for k in ks:
            with reserved_cus(k) as cus:
                out, r = routed(call)
                e = check(out)
                if k == 0:
                    out0, r0, self.err0 = out, r, max(self.err0, e)
                self.err = max(self.err, e)
                if plan is not None:
                    assert r == expect(plan[cus]), (self.name, case, k, r, plan[cus])
                same = same_decomposition(r, r0) or (plan is not None and r == r0 and plan[cus] == plan[256])
                if same:
                    assert equal(out, out0), f"{self.name} {case}: k = {k} ({cus} CUs) differs from k = 0 with the same decomposition {r}"
                    self.bitwise.setdefault(case, []).append(k)
                else:
                    self.tol.setdefault(case, []).append((k, {n: v for n, v in r.items() if v}))
        return out0

    def report(self):
        print(f"[cu-counts] {self.name}: worst {self.err:.3e} (k = 0: {self.err0:.3e}); bitwise {self.bitwise}; by tolerance {self.tol}")

    def require(self, ks, changed=0):
        """Coverage conditions: one case bitwise at every k; `changed` cases whose decomposition differs at some k."""
        self.report()
        assert any(sorted(v) == sorted(ks) for v in self.bitwise.values()), (self.name, self.bitwise)
        assert len(self.tol) >= changed, (self.name, self.tol)


def test_setter_semantics(reserved_cus):
    """visrep_set_reserved_cus: rounds down to a multiple of 8, clamps negatives to 0, returns the previous setting, is ignored where fewer than
    64 CUs would remain; the count is back at 256 afterwards."""
    lib = _lib.require_gpu()
    for k in KS:
        with reserved_cus(k) as cus:
            assert cus == lib.visrep_device_cu_count()
            assert engine.best_chunk(577, 1024, 128) == engine.best_chunk(577, 1024, 128, cus=cus)
    assert lib.visrep_set_reserved_cus(-5) == 0 and lib.visrep_set_reserved_cus(23) == 0 and lib.visrep_set_reserved_cus(0) == 16
    assert lib.visrep_device_cu_count() == 256


# ------------------------------------------------------------------------------------------------ GEMM, variant 5
W_, S_ = ("whole",), lambda m1: ("split", m1)
# (M, N) -> {CUs: whole launch | head of m1 rows on the 256x256 kernel + 128x128 tail}: the rule of visrep_gemm_dispatch evaluated by hand
GEMM_PLAN = {
    (65201, 1024): {256: W_, 248: S_(63488), 240: S_(61440), 192: W_, 128: W_, 64: W_},                 # 1020 tiles
    (36928, 4096): {256: S_(36864), 248: W_, 240: W_, 192: S_(36864), 128: S_(36864), 64: S_(36864)},   # 2320 tiles: flips split <-> whole
    (16717, 1024): {256: S_(16384), 248: S_(15872), 240: S_(15360), 192: W_, 128: S_(16384), 64: S_(16384)},
    (10243, 2048): {256: W_, 248: W_, 240: W_, 192: W_, 128: W_, 64: S_(10240)},                        # a 3-row tail at 64 CUs
    (4685, 1024): {256: W_, 248: W_, 240: W_, 192: W_, 128: W_, 64: S_(4096)},                          # grid = 76 tiles < CUs until 64
    (70000, 256): {256: S_(65536), 248: S_(63488), 240: S_(61440), 192: W_, 128: S_(65536), 64: W_},
    (4000, 1024): {c: W_ for c in (256, 248, 240, 192, 128, 64)},                                       # 64 tiles: grid = tiles at every k
    (256, 256): {c: W_ for c in (256, 248, 240, 192, 128, 64)},                                         # one tile, fewer blocks than XCDs
    (16704, 1024): {256: S_(16384), 248: S_(15872), 240: S_(15360), 192: W_, 128: S_(16384), 64: S_(16384)},
    (16384, 4096): {c: W_ for c in (256, 248, 240, 192, 128, 64)},                                      # 1024 tiles: whole row panels per XCD
}


def gemm_routes(p):
    r = dict.fromkeys(DECOMP, 0)
    r["gemm_256"] = 1
    if p[0] == "split":
        r["gemm_128"] = r["gemm_tail"] = 1
    return r


def gemm_inputs(M, N, K, seed=None):
    g = torch.Generator().manual_seed(M + N + K if seed is None else seed)
    a = bf(torch.randn(M, K, generator=g))
    w = bf(torch.randn(N, K, generator=g) * 0.1)
    bias = torch.randn(N, generator=g)
    ls = torch.randn(N, generator=g)
    x = bf(torch.randn(M, N, generator=g))
    prod = (a.double() @ w.double().t()).to(DEV)                # float64 on the CPU from the bf16-rounded inputs
    return a.to(DEV), w.to(DEV), bias.to(DEV), ls.to(DEV), x.to(DEV), prod


def quick_gelu64(x):
    return x * torch.sigmoid(1.702 * x)


def gemm_epilogue_cases(a, w, bias, ls, x, prod):
    """name -> (call, float64 reference, bar): the bars of tests/test_gpu_kernels.py (EPI_F32 1e-5, BIAS 4e-3, ACT / RESID 6e-3; the V^T buffer
    holds the BIAS values in the attention kernel's column order and takes the BIAS bar)."""
    M, N = prod.shape
    lin = prod + bias.double()
    ld = (M + 63) // 64 * 64 + 64
    return {
        "f32": (lambda: engine.gemm(a, w, bias, _lib.EPI_F32, out=poisoned(M, N, dtype=torch.float32)), lin, 1e-5),
        "bias": (lambda: engine.gemm(a, w, bias, _lib.EPI_BIAS, out=poisoned(M, N)), lin, 4e-3),
        "act": (lambda: engine.gemm(a, w, bias, _lib.EPI_ACT, act="quick_gelu", out=poisoned(M, N)), quick_gelu64(lin), 6e-3),
        "resid": (lambda: engine.gemm(a, w, bias, _lib.EPI_RESID, resid=x, ls=ls, out=poisoned(M, N)), x.double() + ls.double() * lin, 6e-3),
        "vt": (lambda: engine.linear_vt(a, w, bias), vt_layout(lin, ld), 4e-3),          # a zero-filled buffer: a skipped tile stays zero
    }


def barred(want, bar, what, vt_rows=0):
    def check(out):
        e = max_err(vt_defined(out, vt_rows) if vt_rows else out, want)
        assert e < bar, (what, e, bar)
        return e
    return check


def run_gemm_matrix(tally, shapes, epis, ks, reserved_cus, K=256, plan=True):
    for (M, N) in shapes:
        a, w, bias, ls, x, prod = gemm_inputs(M, N, K)
        cases = gemm_epilogue_cases(a, w, bias, ls, x, prod)
        for epi in epis:
            call, want, bar = cases[epi]
            tally.sweep((M, N, epi), ks, reserved_cus, call, barred(want, bar, (tally.name, M, N, epi), M if epi == "vt" else 0),
                        GEMM_PLAN[(M, N)] if plan else None, gemm_routes)
            del want
        del cases, a, w, bias, ls, x, prod
        torch.cuda.empty_cache()


def test_gemm_v5_every_epilogue_at_every_cu_count(reserved_cus):
    """The persistent 256x256 kernel (variant 5), EPI_F32 / BIAS / ACT / RESID with LayerScale / VT, K = 256 (no split-K), at every k, on the
    shapes of GEMM_PLAN: whole launches with grid = CUs, grid = tiles (76, 64 - the G == ntiles edge at 64 CUs - and one tile), head / tail
    splits that appear, move and disappear with the CU count, a 3-row tail, and the V^T tail's column offset.  Reference: float64 on the CPU.
    worst: 3.220e-03 (k = 0: 3.220e-03), an EPI_ACT case against its 6e-3 bar."""
    t = Tally("gemm_v5")
    shapes = [(65201, 1024), (36928, 4096), (16717, 1024), (10243, 2048), (4685, 1024), (70000, 256), (4000, 1024), (256, 256)]
    run_gemm_matrix(t, shapes, ("f32", "bias", "act", "resid", "vt"), KS, reserved_cus)
    t.require(KS, changed=2)
    assert len({c[:2] for c in t.tol}) >= 2


def test_gemm_v2_at_every_cu_count(reserved_cus):
    """The v2 256x256 kernel (variant 2): the same neutrality matrix on two shapes (one that splits, one whose grid is its 64 tiles).
    worst: 3.220e-03 (k = 0: 3.220e-03)."""
    lib = _lib.require_gpu()
    lib.visrep_set_gemm_variant(2)
    t = Tally("gemm_v2")
    run_gemm_matrix(t, [(16717, 1024), (4000, 1024)], ("bias", "act", "resid", "vt"), KS, reserved_cus)
    t.require(KS, changed=1)


# 256 x 128 tiles, rounds of 2 x CUs (variants 6 / 8 everywhere, 7 for N <= 1024 and variant 5's rule - with the same outcome - for N = 2048)
DUO_PLAN = {(16717, 1024): {256: S_(16384), 240: S_(15360), 64: S_(16384)}, (10243, 2048): {256: W_, 240: W_, 64: S_(10240)}}


@pytest.mark.parametrize("variant", [6, 7, 8])
def test_gemm_duo_variants_at_cu_counts(variant, reserved_cus):
    """The duo kernel (two 4-wave workgroups per CU, 256 x 128 tiles) at k = 0, 16, 192: float64 reference, split points from DUO_PLAN, bitwise
    where two runs split at the same row.
    worst (each of 6, 7, 8): 3.192e-03 (k = 0: 3.192e-03)."""
    lib = _lib.require_gpu()
    lib.visrep_set_gemm_variant(variant)
    t = Tally(f"gemm_duo_v{variant}")
    for (M, N) in DUO_PLAN:
        a, w, bias, ls, x, prod = gemm_inputs(M, N, 256)
        cases = gemm_epilogue_cases(a, w, bias, ls, x, prod)
        for epi in ("bias", "resid", "vt"):
            call, want, bar = cases[epi]
            t.sweep((M, N, epi), (0, 16, 192), reserved_cus, call, barred(want, bar, (variant, M, N, epi), M if epi == "vt" else 0), DUO_PLAN[(M, N)], gemm_routes)
    t.report()
    assert len(t.tol) >= 1 and all(0 in v for v in t.bitwise.values())


@pytest.mark.parametrize("variant", [7, 8])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (130, 64, 64), (300, 320, 128), (200, 256, 192), (1731, 384, 1024), (577 * 4, 1024, 256), (256 * 9 + 77, 512, 64),
                                   (70000, 256, 1024)])
def test_gemm_bias_and_f32_variants_7_and_8(M, N, K, variant, reserved_cus):
    """tests/test_gpu_kernels.py::test_gemm_bias_and_f32 under GEMM variants 7 and 8, which its fixture does not list (same body, same bars;
    the reference is torch fp32 on the device, as there)."""
    lib = _lib.require_gpu()
    lib.visrep_set_gemm_variant(variant)
    g = torch.Generator().manual_seed(M + N + K)
    a = bf(torch.randn(M, K, generator=g)).to(DEV)
    w = bf(torch.randn(N, K, generator=g) * 0.1).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    want = (a.float() @ w.float().t() + bias).double()
    got32 = engine.gemm(a, w, bias, _lib.EPI_F32, out=poisoned(M, N, dtype=torch.float32))
    assert max_err(got32, want) < 1e-5
    got = engine.gemm(a, w, bias, _lib.EPI_BIAS, out=poisoned(M, N))
    assert torch.equal(got.float(), bf(got32).float()) or max_err(got, want) < 4e-3
    got_nb = engine.gemm(a, w, None, _lib.EPI_F32, out=poisoned(M, N, dtype=torch.float32))
    assert max_err(got_nb, want - bias.double()) < 1e-5


def test_gemm_walk_codes_are_bitwise_neutral(reserved_cus):
    """visrep_set_gemm_walk 2 / 4 / 8 (column-group-major tile order) on a shape where the walk is taken (16384 x 4096: 1024 tiles, every XCD
    owns 8 whole row panels of 16 column panels) and on one where it silently falls back (4685 x 1024: 76 tiles, XCD chunks that do not start
    on a row panel): bitwise the default order's result, at k = 0 and k = 16, and the EPI_ACT bar against float64.  An XCD's chunk of tiles
    (cstart, csize in gemm_bf16_256q) depends on the tile count and the number of XCDs in use, not on the grid size, so on 16384 x 4096 the walk
    is taken at 240 CUs as well - there with 30 blocks per XCD striding through it instead of 32.  The test proves neutrality of the knob; it has no
    way to observe that a walk was taken (the route counters do not show the tile order).
    worst: 3.202e-03 (one result per shape: every other (k, code) is bitwise it)."""
    lib = _lib.require_gpu()
    worst = 0.0
    for (M, N) in [(16384, 4096), (4685, 1024)]:
        a, w, bias, ls, x, prod = gemm_inputs(M, N, 256)
        call, want, bar = gemm_epilogue_cases(a, w, bias, ls, x, prod)["act"]
        base = None
        for k in (0, 16):
            with reserved_cus(k) as cus:
                for code in (0, 2, 4, 8):
                    lib.visrep_set_gemm_walk(code)
                    try:
                        out, r = routed(call)
                    finally:
                        lib.visrep_set_gemm_walk(0)
                    assert r == gemm_routes(GEMM_PLAN[(M, N)][cus]), (M, N, k, code, r)
                    if base is None:
                        base = out
                        e = max_err(out, want)
                        worst = max(worst, e)
                        assert e < bar, (M, N, e)
                    assert torch.equal(out, base), (M, N, k, code)
    print(f"[cu-counts] gemm_walk: worst {worst:.3e}")
    assert lib.visrep_set_gemm_walk(0) == 0


# ------------------------------------------------------------------------------------------------ LN fold, row map, statistics
def test_gemm_folded_layernorm_where_the_split_moves(reserved_cus):
    """Linear(LayerNorm(x)) from the raw rows (tests/test_gpu_kernels.py::test_gemm_with_folded_layernorm, its 6e-3 relative-L2 bar) on 16717 x
    1024 x 256: the tail carries ln_rt + m1, and m1 is 16384 at 256 and 64 CUs, 15360 at 240.  BIAS and VT.  The row statistics are computed
    in float64 here, not by the library.
    worst (relative L2): 2.329e-03 (k = 0: 2.329e-03)."""
    M, N, K = 16717, 1024, 256
    g = torch.Generator().manual_seed(M + N)
    x = bf(torch.randn(M, K, generator=g) * 2 + torch.randn(M, 1, generator=g))
    gam, bet = torch.randn(K, generator=g) * 0.3 + 1, torch.randn(K, generator=g) * 0.2
    W = bf(torch.randn(N, K, generator=g) / math.sqrt(K)).float()
    bias = torch.randn(N, generator=g) * 0.1
    want = (F.layer_norm(x.double(), (K,), gam.double(), bet.double(), 1e-5) @ W.double().t() + bias.double()).to(DEV)
    Wf = bf(W * gam[None])
    s, bp = Wf.float().sum(1), W @ bet + bias
    mu, var = x.double().mean(1), x.double().var(1, unbiased=False)
    rt = torch.zeros((M + 127) // 128 * 128 + 8, 2, dtype=torch.float32)
    rt[:M, 0], rt[:M, 1] = (var + 1e-5).rsqrt().float(), (-mu * (var + 1e-5).rsqrt()).float()
    lib = _lib.require_gpu()
    xd, Wd, sd, bd, rt = x.to(DEV), Wf.to(DEV), s.to(DEV), bp.to(DEV), rt.to(DEV)
    ld = (M + 63) // 64 * 64 + 64

    def run(epi):
        out = torch.zeros(N, ld, dtype=torch.bfloat16, device=DEV) if epi == _lib.EPI_VT else poisoned(M, N)
        _lib.check(lib.visrep_gemm_bf16_ln(_lib.ptr(xd), K, _lib.ptr(Wd), K, _lib.ptr(bd), _lib.ptr(rt), _lib.ptr(sd), _lib.ptr(out), out.stride(0), M, N, K,
                                           epi, 0, _lib.stream_ptr()), "gemm_ln")
        return out

    def check(ref, vt=False):
        def f(out):
            e = rel_err(vt_defined(out, M) if vt else out, ref)
            assert e < 6e-3, e
            return e
        return f
    t = Tally("gemm_ln_fold (relative L2)")
    t.sweep("bias", (0, 16, 192), reserved_cus, lambda: run(_lib.EPI_BIAS), check(want), GEMM_PLAN[(M, N)], gemm_routes)
    t.sweep("vt", (0, 16, 192), reserved_cus, lambda: run(_lib.EPI_VT), check(vt_layout(want, ld), True), GEMM_PLAN[(M, N)], gemm_routes)
    t.report()
    assert t.bitwise == {"bias": [0, 192], "vt": [0, 192]} and set(t.tol) == {"bias", "vt"}


def test_gemm_row_map_where_the_split_moves(reserved_cus):
    """visrep_gemm_bf16_rows on the patch rows of 29 images of 577 tokens (16704 logical rows, N = 1024): the tail carries a_row0 + m1.  As in
    tests/test_gpu_kernels.py::test_gemm_row_map the result is bitwise the plain GEMM's on the gathered rows at the same k (with and without
    the folded LayerNorm, statistics indexed by physical row); here also against float64 (BIAS bar) and with the split point pinned.
    worst: 2.037e-03 (k = 0: 2.037e-03)."""
    period, stride, first, groups, N, K = 576, 577, 1, 29, 1024, 256
    rows, phys = period * groups, (groups - 1) * stride + period + first + 3
    g = torch.Generator().manual_seed(period + N)
    a = bf(torch.randn(phys, K, generator=g))
    w = bf(torch.randn(N, K, generator=g) / math.sqrt(K))
    bias = torch.randn(N, generator=g)
    r_ = torch.arange(rows)
    idx = (r_ // period) * stride + r_ % period + first
    lin = (a[idx].double() @ w.double().t() + bias.double()).to(DEV)
    ad, wd, bd = a.to(DEV), w.to(DEV), bias.to(DEV)
    gathered = ad[idx.to(DEV)].contiguous()
    ld = (rows + 63) // 64 * 64 + 64
    lib = _lib.require_gpu()
    mu, var = a.double().mean(1), a.double().var(1, unbiased=False)
    rt = torch.zeros(phys + 8, 2, dtype=torch.float32)
    rt[:phys, 0], rt[:phys, 1] = (var + 1e-5).rsqrt().float(), (-mu * (var + 1e-5).rsqrt()).float()
    rt = rt.to(DEV)
    rt_g = torch.zeros(rows + 8, 2, dtype=torch.float32, device=DEV)
    rt_g[:rows] = rt[idx.to(DEV)]
    s_n = wd.float().sum(1).contiguous()
    t = Tally("gemm_row_map")
    for name, e, want in (("bias", _lib.EPI_BIAS, lin), ("vt", _lib.EPI_VT, vt_layout(lin, ld))):
        def call(e=e):
            buf = lambda: None if e == _lib.EPI_VT else poisoned(rows, N)      # V^T: the wrappers' own zero-filled buffer
            got = engine.gemm_rows(ad, period, stride, first, rows, wd, bd, epilogue=e, out=buf())
            plain = engine.linear_vt(gathered, wd, bd) if e == _lib.EPI_VT else engine.gemm(gathered, wd, bd, epilogue=e, out=buf())
            assert torch.equal(got, plain)
            got_ln = engine.gemm_rows(ad, period, stride, first, rows, wd, bd, epilogue=e, ln_rt=rt, ln_s=s_n, out=buf())
            want_ln = torch.zeros_like(got_ln) if e == _lib.EPI_VT else buf()
            _lib.check(lib.visrep_gemm_bf16_ln(_lib.ptr(gathered), K, _lib.ptr(wd), K, _lib.ptr(bd), _lib.ptr(rt_g), _lib.ptr(s_n), _lib.ptr(want_ln),
                                               want_ln.stride(0), rows, N, K, e, 0, _lib.stream_ptr()), "gemm_ln")
            assert torch.equal(got_ln, want_ln)
            return got, got_ln
        plan = GEMM_PLAN[(rows, N)]
        t.sweep(name, (0, 16, 192), reserved_cus, call, lambda o, want=want: barred(want, 4e-3, name)(o[0]), plan,
                lambda p: {k: 4 * v for k, v in gemm_routes(p).items()})
    t.report()
    assert t.bitwise == {"bias": [0, 192], "vt": [0, 192]}


def test_residual_gemm_statistics_where_the_split_moves(reserved_cus):
    """visrep_gemm_bf16_resid_stats on 16717 x 1024 x 512 with LayerScale (tests/test_gpu_kernels.py::
    test_residual_gemm_emits_the_next_layernorm_statistics): the tail carries stat_rt + m1.  x against float64 (6e-3), bitwise the plain residual
    GEMM's at the same k; the statistics against float64 statistics of the stored rows at that test's tolerances.
    worst (x): 2.498e-03 (k = 0: 2.498e-03)."""
    M, N, K = 16717, 1024, 512
    g = torch.Generator().manual_seed(M + N + K)
    A = bf(torch.randn(M, K, generator=g))
    W = bf(torch.randn(N, K, generator=g) / math.sqrt(K))
    bias = torch.randn(N, generator=g) * 0.1
    gamma = torch.randn(N, generator=g) * 0.2 + 1
    x0 = bf(torch.randn(M, N, generator=g) * 1.5 + torch.randn(M, 1, generator=g) + 3 * (torch.arange(N) % 97 == 0).float())
    want = (x0.double() + gamma.double() * (A.double() @ W.double().t() + bias.double())).to(DEV)
    A, W, bias, gamma, x0 = A.to(DEV), W.to(DEV), bias.to(DEV), gamma.to(DEV), x0.to(DEV)
    lib = _lib.require_gpu()

    def call():
        plain = x0.clone()
        _lib.check(lib.visrep_gemm_bf16(_lib.ptr(A), K, _lib.ptr(W), K, _lib.ptr(bias), _lib.ptr(plain), N, M, N, K, _lib.EPI_RESID, 0, _lib.ptr(plain),
                                        _lib.ptr(gamma), _lib.stream_ptr()), "gemm")
        x = x0.clone()
        rt = torch.full((M + 8, 2), float("nan"), dtype=torch.float32, device=DEV)
        part = torch.full((M, N // 64, 2), float("nan"), dtype=torch.float32, device=DEV)
        _lib.check(lib.visrep_gemm_bf16_resid_stats(_lib.ptr(A), K, _lib.ptr(W), K, _lib.ptr(bias), _lib.ptr(x), N, M, N, K, _lib.ptr(x), _lib.ptr(gamma),
                                                    _lib.ptr(rt), _lib.ptr(part), 1e-5, _lib.stream_ptr()), "gemm_resid_stats")
        assert torch.equal(x, plain)
        assert torch.isnan(rt[M:]).all() and torch.isfinite(rt[:M]).all()       # nothing written past the last row, by the head or by the tail
        return x, rt[:M].clone()

    def check(out):
        x, rt = out
        e = max_err(x, want)
        assert e < 6e-3, e
        mu, var = x.double().mean(1), x.double().var(1, unbiased=False)
        rstd = (var + 1e-5).rsqrt()
        torch.testing.assert_close(rt[:M, 0].double(), rstd, rtol=2e-5, atol=0)
        torch.testing.assert_close(rt[:M, 1].double(), -mu * rstd, rtol=2e-4, atol=2e-5)
        return e
    t = Tally("gemm_resid_stats")
    # two launches of the statistics-emitting GEMM per call (plain + emitting)
    t.sweep("resid_stats", (0, 16, 192), reserved_cus, call, check, GEMM_PLAN[(M, N)], lambda p: {k: 2 * v for k, v in gemm_routes(p).items()})
    t.report()
    assert t.bitwise == {"resid_stats": [0, 192]}


# ------------------------------------------------------------------------------------------------ convolutions into NaN-filled buffers
def conv3x3_into_nan(xt, B, H, W, wp, bias, epi=_lib.EPI_BIAS, resid=None, groups=0):
    """sd_engine.conv3x3 (stride 1, symmetric padding) through the ABI, with the output - and the GroupNorm partial sums when groups > 0 - in
    NaN-filled buffers (see poisoned).  Returns out, or (out, partial)."""
    lib = _lib.require_gpu()
    Ci, Co = xt.shape[1], wp.shape[0]
    out = poisoned(B * H * W, Co, dtype=torch.float32 if epi == _lib.EPI_F32 else torch.bfloat16)
    if not groups:
        _lib.check(lib.visrep_conv3x3_bf16(_lib.ptr(xt), B, H, W, Ci, _lib.ptr(wp), wp.stride(0), _lib.ptr(bias), _lib.ptr(out), out.stride(0), Co, 1, 0, 0, epi,
                                           _lib.ptr(resid), _lib.stream_ptr()), "visrep_conv3x3_bf16")
        return out
    part = poisoned(lib.visrep_conv_gn_partial_bytes(B, H * W, groups) // 4, dtype=torch.float32)
    _lib.check(lib.visrep_conv3x3_bf16_gn(_lib.ptr(xt), B, H, W, Ci, _lib.ptr(wp), wp.stride(0), _lib.ptr(bias), _lib.ptr(out), out.stride(0), Co, 1, 0, epi,
                                          _lib.ptr(resid), _lib.ptr(part), groups, _lib.stream_ptr()), "visrep_conv3x3_bf16_gn")
    return out, part


def conv3x3_halo_into_nan(xt, B, H, W, wp, bias, groups):
    """sd_engine.conv3x3_halo (EPI_BIAS, no GroupNorm in front) through the ABI, output and partial sums in NaN-filled buffers."""
    lib = _lib.require_gpu()
    Co = wp.shape[0]
    out = poisoned(B * H * W, Co)
    part = poisoned(lib.visrep_conv_gn_partial_bytes(B, H * W, groups) // 4, dtype=torch.float32)
    _lib.check(lib.visrep_conv3x3_bf16_halo(_lib.ptr(xt), B, H, W, xt.shape[1], _lib.ptr(wp), wp.stride(0), _lib.ptr(bias), _lib.ptr(out), out.stride(0), Co,
                                            _lib.EPI_BIAS, None, None, 0, _lib.ptr(part), groups, _lib.stream_ptr()), "visrep_conv3x3_bf16_halo")
    return out, part


# ------------------------------------------------------------------------------------------------ split-K
def test_split_k_slice_count_follows_the_cu_count(reserved_cus):
    """Few tiles, deep K, scratch registered: S = 2 CUs / tiles (capped at K-tiles / 4, rounded down to a divisor) - 16 slices at 256 CUs and 4 at
    64 for the ViT-tail-sized GEMM (333 x 1024 x 4096: 24 tiles, 64 K-tiles), 10 and 2 for the diffusion-sized 3x3 convolution (1 x 24 x 24 x
    1280 -> 1280: 50 tiles, 180 K-tiles).  Every k against float64 at the bars of tests/test_gpu_sd.py (test_gemm_split_k_small_m_deep_k:
    1e-4 x max(1, max |want|) absolute for EPI_F32, 4e-3 relative L2 for RESID; test_conv3x3_implicit_gemm: 2e-3 x max(1, max |want|) and 5e-3),
    two launches at one k bitwise equal, the `splitk` route counted.  Errors here: max |d| / max(1, max |want|).
    worst (EPI_F32): GEMM 1.97e-07 (k = 0: 1.30e-07), convolution 1.08e-06 (k = 0: 2.89e-07)."""
    SE.ensure_scratch(torch.device(DEV))
    M, N, K = 333, 1024, 4096
    g = torch.Generator().manual_seed(M + K)
    a = bf(torch.randn(M, K, generator=g))
    w = bf(torch.randn(N, K, generator=g) / math.sqrt(K))
    bias, ls = torch.randn(N, generator=g), torch.randn(N, generator=g)
    x = bf(torch.randn(M, N, generator=g))
    lin = (a.double() @ w.double().t() + bias.double()).to(DEV)
    a, w, bias, ls, x = a.to(DEV), w.to(DEV), bias.to(DEV), ls.to(DEV), x.to(DEV)
    want_r = x.double() + ls.double() * lin
    B, H, Wd, Ci, Co = 1, 24, 24, 1280, 1280
    g = torch.Generator().manual_seed(H * 100 + Ci)
    cx = bf(torch.randn(B, Ci, H, Wd, generator=g))
    cw = bf(torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci))
    cb = torch.randn(Co, generator=g) * 0.1
    cols = F.unfold(cx.double(), 3, padding=1)[0]                                       # [Ci * 9, H W], rows in (c, ky, kx) order as cw.view(Co, -1)
    cwant = ((cw.double().view(Co, -1) @ cols).t() + cb.double()).contiguous().to(DEV)
    cres = bf(torch.randn(B * H * Wd, Co, generator=g)).to(DEV)
    wp = bf(cw.float().permute(0, 2, 3, 1).reshape(Co, 9 * Ci)).to(DEV)
    xt = cx.permute(0, 2, 3, 1).reshape(B * H * Wd, Ci).contiguous().to(DEV)
    cb = cb.to(DEV)
    worst = {"gemm": [0.0, 0.0], "conv": [0.0, 0.0]}
    outs = {}
    for k in KS:
        with reserved_cus(k):
            for rep in range(2):
                (g32, gr), r = routed(lambda: (engine.gemm(a, w, bias, _lib.EPI_F32, out=poisoned(M, N, dtype=torch.float32)),
                                                 engine.gemm(a, w, bias, _lib.EPI_RESID, resid=x, ls=ls, out=poisoned(M, N))))
                assert r["splitk"] == 2 and r["gemm_256"] + r["gemm_128"] + r["gemm_tail"] == 0, (k, r)
                (c32, cr), r = routed(lambda: (conv3x3_into_nan(xt, B, H, Wd, wp, cb, _lib.EPI_F32), conv3x3_into_nan(xt, B, H, Wd, wp, cb, _lib.EPI_RESID, resid=cres)))
                assert r["splitk"] == 2 and r["conv_256"] + r["conv_128"] == 0, (k, r)
                if rep:
                    assert equal((g32, gr, c32, cr), outs[k]), k                                   # slice order is fixed: bit-reproducible
                outs[k] = (g32, gr, c32, cr)
            e = ((g32.double() - lin).abs().max() / max(1.0, lin.abs().max().item())).item()
            assert e < 1e-4 and rel_err(gr, want_r) < 4e-3, (k, e)
            ec = ((c32.double() - cwant).abs().max() / max(1.0, cwant.abs().max().item())).item()
            assert ec < 2e-3 and rel_err(cr, cres.double() + cwant) < 5e-3, (k, ec)
            for name, v in (("gemm", e), ("conv", ec)):
                worst[name] = [max(worst[name][0], v), v if k == 0 else worst[name][1]]
    # another slice count is another summation tree: the fp32 results at 256 and 64 CUs are not the same bits (they would be if S did not follow the count)
    assert not torch.equal(outs[0][0], outs[192][0]) and not torch.equal(outs[0][2], outs[192][2])
    assert equal(outs[0], outs[200]) and equal(outs[8], outs[13])
    print(f"[cu-counts] split-K: worst {worst} ([any k, k = 0])")


# ------------------------------------------------------------------------------------------------ implicit 3x3 convolution
def conv_routes(**kw):
    r = dict.fromkeys(DECOMP, 0)
    r.update(kw)
    return r


# (B, H, W, Ci, Co) -> {CUs: route deltas of ONE convolution call}: 256-wide tiles = B H W / 256 (Co = 256); the 256x256 kernel from 2 x CUs tiles
CONV_PLAN = {
    (8, 128, 160, 64, 256): {c: ("conv_256",) for c in (256, 248, 240, 192, 128, 64)},                 # 640 tiles: no remainder small enough to split off at any count
    (2, 128, 128, 64, 256): {256: ("conv_128",), 248: ("conv_128",), 240: ("conv_128",), 192: ("conv_128",), 128: ("conv_128",), 64: ("conv_256",)},   # 128 tiles
    (4, 192, 192, 64, 256): {256: ("conv_256", "tail"), 248: ("conv_256",), 240: ("conv_256",), 192: ("conv_256",), 128: ("conv_256",),
                             64: ("conv_256",)},                                                        # 576 tiles: 2 x 256 + a 64-tile tail at 256 CUs, whole elsewhere
}


def conv_expect(p, gn):
    small = "conv_128_gn" if gn else "conv_128"
    r = conv_routes(**{small if p[0] == "conv_128" else "conv_256": 1})
    if "tail" in p:
        r[small] += 1
        r["gemm_tail"] = 1
    return r


def test_conv3x3_implicit_at_every_cu_count(reserved_cus, monkeypatch):
    """visrep_conv3x3_bf16 / _gn (EPI_BIAS, with and without GroupNorm partial sums) on the cases of CONV_PLAN at every k: one shape on the
    256x256 kernel throughout, one that moves from the 128x128 kernel to the 256x256 kernel at 64 CUs (128 tiles >= 2 x 64), one whose 64-tile
    remainder is split off at 256 CUs only.  Inputs and float64 reference (unrounded output) from tests/_hostile_gn_cases.py at its
    mildest ratio (|mean| = 10 sigma per (image, group)); bars of tests/test_gpu_hostile_gn.py: output 5e-3 relative L2, mean 1e-5, rstd 3e-4
    relative against float64 statistics of the unrounded output.  visrep_conv_gn_supported_epi(RESID) flips where 2 x CUs reaches the tile count.
    worst: output 1.789e-03 (k = 0: 1.789e-03), with and without the sums; mean 1.58e-07, rstd 1.37e-05."""
    monkeypatch.delenv("VISREP_GN_RESID_256", raising=False)
    t, tg = Tally("conv3x3 (relative L2)"), Tally("conv3x3_gn (relative L2)")
    stats = [0.0, 0.0]
    for shape, plan in CONV_PLAN.items():
        B, H, W, Ci, Co = shape
        case = ("conv", B, H, W, Ci, Co, 1, 0, HC.EPI_BIAS)
        c = HC.make_case(case, 10.0)
        G, HW = c["G"], H * W
        ref = c["ref"].view(B * HW, Co).to(DEV)
        m64, v64 = HC.stats64(c["ref"], G)
        r64 = (v64 + c["eps"]).rsqrt()
        xt = c["x"].permute(0, 2, 3, 1).reshape(B * HW, Ci).contiguous().to(DEV)
        wp = HC.bf16(c["w"].float().permute(0, 2, 3, 1).reshape(Co, 9 * Ci)).contiguous().to(DEV)
        bias = c["bias"].to(DEV)
        tiles = B * HW // 256
        for k in KS:
            with reserved_cus(k) as cus:
                assert SE.conv_gn_supported(B, HW, Co, G, _lib.EPI_BIAS)
                assert SE.conv_gn_supported(B, HW, Co, G, _lib.EPI_RESID) == (tiles < 2 * cus), (shape, k)

        def check(out):
            e = rel_err(out, ref)
            assert e < 5e-3, (shape, e)
            return e

        def check_gn(o):
            out, part = o
            st = SE.groupnorm_stats(out, B, G, c["eps"], partial=part).double().cpu()
            e_mean = ((st[..., 0] - m64).abs() / m64.abs()).max().item()
            e_rstd = ((st[..., 1] - r64).abs() / r64).max().item()
            assert e_mean < 1e-5 and e_rstd < 3e-4, (shape, e_mean, e_rstd)
            stats[0], stats[1] = max(stats[0], e_mean), max(stats[1], e_rstd)
            return check(out)
        plain = t.sweep(shape, KS, reserved_cus, lambda: conv3x3_into_nan(xt, B, H, W, wp, bias), check, plan,
                        lambda p: conv_expect(p, False))
        with_gn = tg.sweep(shape, KS, reserved_cus, lambda: conv3x3_into_nan(xt, B, H, W, wp, bias, groups=G), check_gn, plan,
                           lambda p: conv_expect(p, True))
        assert torch.equal(with_gn[0], plain)                    # K = 576: no split-K, the sums do not change the output
        del ref, xt
        torch.cuda.empty_cache()
    print(f"[cu-counts] conv3x3_gn statistics: worst mean {stats[0]:.3e} rstd {stats[1]:.3e}")
    t.require(KS, changed=2)
    tg.require(KS, changed=2)


# ------------------------------------------------------------------------------------------------ conv3x3_halo
@pytest.mark.parametrize("tile", [16, 8])
def test_conv3x3_halo_at_cu_counts(tile, reserved_cus):
    """conv3x3_halo, both tile heights, at k = 0, 16, 192: the resident-workgroup cap is CUs (16 x 16 tiles) or 2 x CUs (16 x 8) = 256 / 240 / 64
    or 512 / 480 / 128, and the images give 3, 64 | 128, 256 | 512 and 320 | 640 tiles - below, equal to, just above and several times the cap.
    Output and GroupNorm partial sums bitwise the k = 0 result; output 5e-3 relative L2 against the float64 convolution, statistics at the
    bars of tests/test_gpu_hostile_gn.py (inputs of tests/_hostile_gn_cases.py, ratio 10).
    worst (both tile heights): 1.831e-03 (k = 0: 1.831e-03); every (shape, k) bitwise."""
    lib = _lib.require_gpu()
    lib.visrep_set_conv_halo_tile(tile)
    t = Tally(f"conv_halo tile {tile} (relative L2)")
    for (B, H, W) in [(3, 16, 16), (1, 128, 128), (4, 128, 128), (5, 128, 128)]:
        c = HC.make_case(("conv_halo", B, H, W, 128, 128, 1, 0, HC.EPI_BIAS), 10.0)
        G, HW, Co = c["G"], H * W, 128
        assert SE.conv_halo_supported(B, H, W, 128, Co)
        ref = c["ref"].view(B * HW, Co).to(DEV)
        m64, v64 = HC.stats64(c["ref"], G)
        r64 = (v64 + c["eps"]).rsqrt()
        xt = c["x"].permute(0, 2, 3, 1).reshape(B * HW, 128).contiguous().to(DEV)
        wp = HC.bf16(c["w"].float().permute(0, 2, 3, 1).reshape(Co, 9 * 128)).contiguous().to(DEV)
        bias = c["bias"].to(DEV)

        def check(o):
            out, part = o
            e = rel_err(out, ref)
            st = SE.groupnorm_stats(out, B, G, c["eps"], partial=part).double().cpu()
            e_mean = ((st[..., 0] - m64).abs() / m64.abs()).max().item()
            e_rstd = ((st[..., 1] - r64).abs() / r64).max().item()
            assert e < 5e-3 and e_mean < 1e-5 and e_rstd < 3e-4, ((B, H, W), e, e_mean, e_rstd)
            return e
        t.sweep((B, H, W), (0, 16, 192), reserved_cus, lambda: conv3x3_halo_into_nan(xt, B, H, W, wp, bias, G), check)
    t.report()
    assert len(t.bitwise) == 4 and all(v == [0, 16, 192] for v in t.bitwise.values()) and not t.tol


# ------------------------------------------------------------------------------------------------ A score
@pytest.mark.parametrize("n,Nt,Nr,D", [(300, 96, 200, 64), (40, 192, 384, 128), (2, 190, 193, 64)])
def test_ascore_persistent_kernel_at_every_cu_count(n, Nt, Nr, D, reserved_cus):
    """The persistent ping-pong Gram kernel (visrep_set_ascore_variant(2)) with more tiles than CUs (n = 300, n = 40) and fewer than 64 (n = 2):
    at every k bitwise the k = 0 result and the 128 x 128 kernel's (variant 1), 1e-4 relative against oracle.ascore.max_cos_mean.
    worst: 1.14e-07 (bitwise at every k, so the same at k = 0)."""
    lib = _lib.require_gpu()
    g = torch.Generator().manual_seed(n * 1000 + Nt + Nr)
    shared = torch.randn(n, 1, D, generator=g)
    o = (torch.randn(n, Nt, D, generator=g) + 0.7 * shared).to(torch.bfloat16)
    r = (torch.randn(n, Nr, D, generator=g) + 0.7 * shared).to(torch.bfloat16)
    od, rd = o.to(DEV), r.to(DEV)
    idx = list(range(n)) if n <= 5 else [0, 1, n // 2, n - 2, n - 1]
    want = torch.tensor([OA.max_cos_mean(o[i], r[i]) for i in idx])

    def maxcos():                                                   # ascore_ops.max_cos_mean through the ABI: NaN scores, an all-ones-bits workspace
        scores = poisoned(n, dtype=torch.float32)
        ws = torch.full((lib.visrep_ascore_workspace_bytes(n, Nt, Nr),), 0xFF, dtype=torch.uint8, device=DEV)
        _lib.check(lib.visrep_ascore_maxcos_scaled(_lib.ptr(od), _lib.ptr(rd), None, None, n, Nt, Nr, D, _lib.BF16, _lib.ptr(scores), _lib.ptr(ws),
                                                   _lib.stream_ptr()), "visrep_ascore_maxcos_scaled")
        return scores.cpu()
    lib.visrep_set_ascore_variant(1)
    v1 = maxcos()
    assert torch.equal(v1, ascore_ops.max_cos_mean(od, rd).cpu())
    lib.visrep_set_ascore_variant(2)
    base, worst = None, 0.0
    for k in KS:
        with reserved_cus(k):
            got = maxcos()
        base = got if base is None else base
        e = ((got[idx] - want).abs() / want.abs()).max().item()
        worst = max(worst, e)
        assert e < 1e-4, (k, e)
        assert torch.equal(got, base) and torch.equal(got, v1), k
    print(f"[cu-counts] ascore n={n}: worst {worst:.3e} (the same at every k: bitwise)")


# ------------------------------------------------------------------------------------------------ engines under a reservation
def test_vit_engine_built_under_a_reservation(reserved_cus):
    """The clip_quick golden tower and CLIP-L/14-336 on 3 images, engines built and run with 16 CUs reserved: the assertions of
    tests/test_gpu_kernels.py::test_tower_matches_reference_golden and ::test_vit_l14_336_full_size_parity; the planner sees the library's count.
    measured (relative L2): clip_quick 4.79e-03 (bf16 reference run 5.42e-03), CLIP-L/14-336 1.23e-02 (1.35e-02)."""
    with reserved_cus(16):
        assert engine.best_chunk(577, 1024, 128) == engine.best_chunk(577, 1024, 128, cus=240)
        spec, w, px, want = load_vit_hip_case("clip_quick")
        hid = engine.VitEngine(spec, w, DEV).forward(px.to(DEV), n_layers=spec.layers - 1)
        ref_bf16 = OV.tower_features(spec, w, px, -2, "patch", dtype=torch.bfloat16)
        rel = lambda a, b: ((a.float().cpu() - b.float().cpu()).norm() / b.float().cpu().norm()).item()
        e_hip, e_ref = rel(hid[:, 1:], want), rel(ref_bf16, want)
        assert e_hip < max(2.0 * e_ref, 1e-2), (e_hip, e_ref)
        spec = VW.SPECS["openai/clip-vit-large-patch14-336"]
        w = VW.synthetic_weights(spec, seed=1, n_layers=23)
        px = torch.from_numpy(np.random.RandomState(2).standard_normal((3, 3, 336, 336)).astype(np.float32))
        got = engine.VitEngine(spec, w, DEV).forward(bf(px).to(DEV), n_layers=23)[:, 1:]
        torch.cuda.synchronize()
    want = OV.tower_features(spec, w, bf(px).float(), select_layer=23, select_feature="patch")
    ref_bf16 = OV.tower_features(spec, w, bf(px).float(), select_layer=23, select_feature="patch", dtype=torch.bfloat16)
    e_full, e_fref = rel(got, want), rel(ref_bf16, want)
    print(f"[cu-counts] ViT at k = 16: clip_quick {e_hip:.3e} (bf16 reference {e_ref:.3e}), CLIP-L/14-336 {e_full:.3e} ({e_fref:.3e})")
    assert e_full < max(1.5 * e_fref, 2e-2) and torch.isfinite(got.float()).all(), (e_full, e_fref)


def test_sd_graph_captured_before_the_setter_replays_unchanged(reserved_cus):
    """A graph-replaying SD engine captured at k = 0 and replayed after visrep_set_reserved_cus(64): bitwise the output from before the setter
    (grids captured into a HIP graph keep the size they were captured with).  A fresh engine built at k = 64 - its build-time
    visrep_conv_gn_supported_epi answers and its launches both see 192 CUs - meets the golden bar of test_sd_tower_matches_reference_golden.
    measured: 1.47e-02 (bf16 reference run 1.75e-02); the k = 64 engine's output was bitwise the k = 0 engine's."""
    sp, wu, wv, inp, want = load_sd_case("conv_up1_ens2")
    kw = dict(t=inp["t"], ensemble_size=inp["ensemble_size"], post_noise=inp["post_noise"], ddim_noise=inp["ddim_noise"])
    eng = SE.SdEngine(sp, wu, wv, DEV, up_ft_index=1, graph=True)
    first = eng.forward(inp["img"], inp["prompt_embeds"], **kw).clone()
    assert len(eng._graphs) == 1
    with reserved_cus(64):
        again = eng.forward(inp["img"], inp["prompt_embeds"], **kw)
        assert len(eng._graphs) == 1 and torch.equal(again, first)
        fresh = SE.SdEngine(sp, wu, wv, DEV, up_ft_index=1, graph=True)
        got = fresh.forward(inp["img"], inp["prompt_embeds"], **kw).clone()
        assert torch.equal(fresh.forward(inp["img"], inp["prompt_embeds"], **kw), got)
    ref_bf16 = OD.sd_features(sp, wu, wv, inp["img"], inp["prompt_embeds"], inp["post_noise"], inp["ddim_noise"], t=inp["t"], up_ft_index=1,
                              ensemble_size=inp["ensemble_size"], dtype=torch.bfloat16)
    rel = lambda a, b: ((a.float().cpu() - b.float().cpu()).norm() / b.float().cpu().norm()).item()
    e_hip, e_ref = rel(got, want), rel(ref_bf16, want)
    print(f"[cu-counts] tiny SD built at k = 64: {e_hip:.3e} (bf16 reference {e_ref:.3e}); bitwise the k = 0 engine: {torch.equal(got, first)}")
    assert e_hip < max(2.0 * e_ref, 2e-2), (e_hip, e_ref)


def test_tiny_sweep_under_a_reservation(reserved_cus, monkeypatch):
    """The reduced sweep of tests/test_gpu_sweep.py ('reference' precision) at k = 16 against the k = 0 run: equal A and PCK as Python floats
    when the route counters of the two runs agree, else that test's bars against the oracle chain.
    The routes are unchanged (the tiny towers' GEMMs are far below one round of tiles at either count), so it is the equality that holds."""
    import test_gpu_sweep as TS
    from law_of_vision_representation_in_mllms_amd import sweep as S
    monkeypatch.setattr(VW, "SPECS", {**VW.SPECS, **TS.TINY})
    build = lambda st: S.SettingModel(st, TS.DEV, hidden=TS.HIDDEN, precision="reference", fast_weights=False)
    run = lambda: S.run_sweep(TS.SETTINGS, TS.N_A, TS.spair_small(), TS.DEV, build=build, precision="reference", also_bf16=False)
    out0, r0 = routed(run)
    with reserved_cus(16):
        out, r = routed(run)
    same = r == r0
    print(f"[cu-counts] tiny sweep at k = 16: routes {'unchanged' if same else (r0, r)}")
    want = None if same else TS.oracle_sweep(torch.float32)
    for st in TS.SETTINGS:
        e0, e = out0["per_setting"][st.name], out["per_setting"][st.name]
        if same:
            assert e["A"] == e0["A"] and list(e["pck"]) == list(e0["pck"]), (st.name, e, e0)
        else:
            A, pck = want[st.name]
            assert abs(e["A"] - A) <= 2e-2 * abs(A), (st.name, e["A"], A)
            np.testing.assert_allclose(e["pck"], pck, atol=1e-6 if st.name != "SigLIP" else 0.1, err_msg=st.name)
