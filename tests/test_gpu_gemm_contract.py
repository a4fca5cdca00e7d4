"""Contract of the bf16 GEMM epilogues on the GPU: every case of tests/_gemm_cases.py runs through the C ABI into a sentinel-guarded window and is
held, element by element, to the float64 oracle's derived bound; the output is finite, nothing outside the window changed a bit, and the
kernel family that ran is the one the case names (_lib.routes()).  One parametrised test per group; tests/test_host_gemm_cases.py proves
the oracle, the bound and the table on the CPU."""
import ctypes as C
import os
import sys
import time
from collections import defaultdict

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _gemm_cases as GC  # noqa: E402

from law_of_vision_representation_in_mllms_amd import _lib, engine  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPI = {"bias": _lib.EPI_BIAS, "act": _lib.EPI_ACT, "resid": _lib.EPI_RESID, "f32": _lib.EPI_F32, "vt": _lib.EPI_VT}
COUNTERS = {"128": {"gemm_128": 1, "gemm_256": 0, "gemm_tail": 0, "splitk": 0}, "256": {"gemm_128": 0, "gemm_256": 1, "gemm_tail": 0, "splitk": 0},
            "splitk": {"gemm_128": 0, "gemm_256": 0, "gemm_tail": 0, "splitk": 1}, "headtail": {"gemm_128": 1, "gemm_256": 1, "gemm_tail": 1, "splitk": 0}}
STAT_SOURCE = {"256": "epilogue sums", "splitk": "split-K reduce", "headtail": "head sums + tail read-back"}
WORST = defaultdict(float)                                     # (epilogue, kernel family) -> worst device err / bound, printed when the module ends


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.time()
    yield
    for k in sorted(WORST):
        print(f"[gemm-contract] worst device err/bound  {k[0]:24s} {k[1]:22s} {WORST[k]:.4f}")
    print(f"[gemm-contract] wall time of this file: {time.time() - t0:.1f} s")


def epilogue_key(case):
    return case.kind + ("-" + case.act if case.act else "") + ("-ls" if case.ls else "") + ("-ln" if case.ln else "") + ("-" + case.stats if case.stats else "")


def family(case):
    if case.route in ("splitk", "headtail"):
        return case.route
    return {1: "v1 128x128", 2: "v2 256x256", 5: "v5 256x256", 6: "duo", 7: "duo (N <= 1024)", 8: "duo unpipelined"}[case.variant] if case.route == "256" else "v1 128x128"


def ptr_at(t):
    return C.c_void_p(t.data_ptr())


def run_case(case):
    lib = _lib.load()
    engine.ensure_scratch(torch.device(DEV))
    M = GC.head_tail_rows(lib.visrep_device_cu_count(), case) if case.group == "headtail" else case.M
    N, K, vt = case.N, case.K, case.kind == "vt"
    inp = GC.make_inputs(case, M)
    want, bound = GC.reference_for(case, inp, M)
    a, w, bias = inp["a"].to(DEV), inp["w"].to(DEV), inp["bias"].to(DEV)
    ls = None if inp["ls"] is None else inp["ls"].to(DEV)
    ln_rt = ln_s = None
    if case.ln:                                                # statistics by PHYSICAL row, padded with zeros (include/visrep.h)
        ln_rt = torch.zeros(GC.round_up(a.shape[0], 256) + 8, 2, device=DEV)
        ln_rt[:a.shape[0]] = inp["ln"][0].to(DEV)
        ln_s = inp["ln"][1].to(DEV)
    dtype = torch.float32 if case.kind == "f32" else torch.bfloat16
    ldc, col0 = GC.window_of(case, M)
    buf, view = GC.make_window(M, N, ldc, col0, dtype, vt=vt, device=DEV)
    resid = rbuf = rbefore = None
    if case.kind == "resid":
        if case.resid == "in":
            view.copy_(inp["resid"].to(DEV))
            resid = view
        else:                                                  # its own guarded window of the same leading dimension
            rcol0 = col0 if GC.RESID_COL0[case.resid] is None else GC.RESID_COL0[case.resid]
            rbuf, resid = GC.make_window(M, N, ldc, rcol0, dtype, device=DEV)
            resid.copy_(inp["resid"].to(DEV))
            rbefore = rbuf.clone()
    stat_rt = None
    old = lib.visrep_set_gemm_variant(case.variant)
    try:
        torch.cuda.synchronize()
        _lib.routes(reset=True)
        if case.stats:
            stat_rt = torch.full((M + 8, 2), GC.SENTINEL[torch.float32][1], dtype=torch.int32, device=DEV).view(torch.float32)
            partial = torch.empty(M * N // 64, 2, device=DEV)
            fn = lib.visrep_gemm_bf16_resid_rms_stats if case.stats == "rms" else lib.visrep_gemm_bf16_resid_stats
            _lib.check(fn(_lib.ptr(a), K, _lib.ptr(w), K, _lib.ptr(bias), ptr_at(view), ldc, M, N, K, ptr_at(resid), _lib.ptr(ls), _lib.ptr(stat_rt),
                          _lib.ptr(partial), GC.STATS_EPS, _lib.stream_ptr()), "resid stats GEMM")
        elif case.rows:
            p, s, f = case.rows
            engine.gemm_rows(a, p, s, f, M, w, bias, epilogue=EPI[case.kind], act=case.act or "none", ln_rt=ln_rt, ln_s=ln_s,
                             out=buf[GC.VT_GUARD_ROWS:GC.VT_GUARD_ROWS + N, col0:] if vt else view)
        elif case.ln:
            _lib.check(lib.visrep_gemm_bf16_ln(_lib.ptr(a), K, _lib.ptr(w), K, _lib.ptr(bias), _lib.ptr(ln_rt), _lib.ptr(ln_s), ptr_at(view), ldc, M, N, K,
                                               EPI[case.kind], _lib.ACT[case.act or "none"], _lib.stream_ptr()), "visrep_gemm_bf16_ln")
        elif vt and col0 % 16 == 0:
            engine.linear_vt(a, w, bias, out=buf[GC.VT_GUARD_ROWS:GC.VT_GUARD_ROWS + N], col_offset=col0)
        elif vt:                                               # a window linear_vt does not take (col0 % 16 != 0): the entry point itself
            _lib.check(lib.visrep_gemm_bf16(_lib.ptr(a), K, _lib.ptr(w), K, _lib.ptr(bias), ptr_at(view), ldc, M, N, K, _lib.EPI_VT, 0, None, None,
                                            _lib.stream_ptr()), "visrep_gemm_bf16(VT)")
        else:
            engine.gemm(a, w, bias, EPI[case.kind], act=case.act or "none", resid=resid, ls=ls, out=view)
        torch.cuda.synchronize()
        r = _lib.routes(reset=True)
    finally:
        lib.visrep_set_gemm_variant(old)
    routes = {k: v for k, v in r.items() if v}
    got = (GC.vt_unpermute(buf, M, col0, GC.VT_GUARD_ROWS, N) if vt else view).double().cpu()
    err = (got - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"[gemm-contract] {case.id} (M = {M}): max err/bound {worst:.4f}, max err {err.max().item():.3e}, routes {routes}")
    WORST[(epilogue_key(case), family(case))] = max(WORST[(epilogue_key(case), family(case))], worst)
    assert torch.isfinite(buf[GC.window_mask(buf, M, N, col0, vt)].float()).all(), case.id
    assert (err <= bound).all(), (case.id, worst, (err > bound).nonzero()[:8].tolist())
    assert GC.stray_writes(buf, M, N, col0, vt) == 0, (case.id, "the kernel wrote outside its window")
    if rbuf is not None:
        assert torch.equal(rbuf.view(torch.int16), rbefore.view(torch.int16)), (case.id, "the out-of-place residual was modified")
    for name, n in COUNTERS[case.route].items():
        assert r[name] == n, (case.id, routes)
    if case.stats:
        rms = case.stats == "rms"
        x = view.cpu()
        rt_want, rt_bound = GC.row_stats_reference(x, GC.STATS_EPS, rms)
        rt_got = stat_rt[:M].double().cpu()
        rerr = (rt_got - rt_want).abs()
        pos = rt_bound > 0
        sw = (rerr[pos] / rt_bound[pos]).max().item()
        ratio = x.double().mean(1).abs() / x.double().std(1, unbiased=False)
        print(f"[gemm-contract] {case.id}: statistics max err/bound {sw:.4f}, |mean| / std of the written rows {ratio.min().item():.2f} .. {ratio.max().item():.2f}")
        skey = ("row statistics " + case.stats + " " + case.dist, f"N = {N} " + STAT_SOURCE[case.route])
        WORST[skey] = max(WORST[skey], sw)
        assert (rerr <= rt_bound).all(), (case.id, sw)
        assert case.dist != "offset" or ratio.min() >= 5.0, (case.id, ratio.min().item())
        assert (stat_rt[M:].view(torch.int32) == GC.SENTINEL[torch.float32][1]).all(), (case.id, "statistics written past row M")
        # 256: the epilogue's partial sums;  splitk: the reduction emits them;  headtail: the head's from its partial sums, the tail's rows read back
        epi, red, rows = {"256": (1, 0, 0), "splitk": (0, 1, 0), "headtail": (1, 0, 1)}[case.route]
        assert (r["stats_epilogue"], r["stats_reduce"], r["stats_rows"]) == (epi, red, rows) and r["rms"] == ((epi + red + rows) if rms else 0), (case.id, routes)
    return r


def ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("case", GC.GROUPS["rowmajor"], ids=ids(GC.GROUPS["rowmajor"]))
def test_rowmajor_epilogues(case):
    """BIAS, ACT (quick_gelu, gelu, gelu_tanh), RESID with and without LayerScale, in place and out of place, on the 128 x 128, v2, v5 and duo
    kernels: interior and edge tiles, AL and not AL (window alignment; for an out-of-place residual through the third operand too)."""
    run_case(case)


@pytest.mark.parametrize("case", GC.GROUPS["vt"], ids=ids(GC.GROUPS["vt"]))
def test_vt_epilogue(case):
    """The V^T scatter, compared in logical coordinates: wide and narrow stores, m + 8 < M, m + 8 == M, M % 4 != 0."""
    run_case(case)


@pytest.mark.parametrize("case", GC.GROUPS["f32"], ids=ids(GC.GROUPS["f32"]))
def test_f32_epilogue(case):
    run_case(case)


@pytest.mark.parametrize("case", GC.GROUPS["ln"], ids=ids(GC.GROUPS["ln"]))
def test_folded_layernorm(case):
    """visrep_gemm_bf16_ln: rstd * acc + t * s[n] + bias in front of BIAS, ACT and V^T."""
    run_case(case)


@pytest.mark.parametrize("case", GC.GROUPS["rows"], ids=ids(GC.GROUPS["rows"]))
def test_row_map(case):
    """visrep_gemm_bf16_rows against the oracle on the gathered rows (statistics indexed by physical row)."""
    run_case(case)


@pytest.mark.parametrize("case", GC.GROUPS["stats"], ids=ids(GC.GROUPS["stats"]))
def test_statistics_gemms(case):
    """The two statistics-emitting residual GEMMs: x against the GEMM oracle, rt[:M] against the float64 statistics of the x that was written
    (one-pass bound), rt[M:] untouched; N = 256 from the epilogue's partial sums, N = 1024 from the split-K reduction; plain and offset rows."""
    run_case(case)


@pytest.mark.parametrize("case", GC.GROUPS["splitk"], ids=ids(GC.GROUPS["splitk"]))
def test_split_k_reductions(case):
    """K = 1024, few tiles, scratch registered: splitk_reduce and splitk_reduce_vt restate every epilogue; same oracle, windowed C."""
    run_case(case)


@pytest.mark.parametrize("case", GC.GROUPS["headtail"], ids=ids(GC.GROUPS["headtail"]))
def test_head_plus_tail(case):
    """One full round of 256 x 256 tiles plus an edge on the 128 x 128 kernel: the tail's C, resid, ln_rt and stat_rt pointer arithmetic with
    ldc != N (the two statistics cases: rows of the head from its epilogue's partial sums, rows of the tail read back from C + m1 * ldc)."""
    run_case(case)


# ------------------------------------------------------------------------------------------------ refusals: nothing is launched
def refused(call, code, word):
    _lib.routes(reset=True)
    rc = call()
    torch.cuda.synchronize()
    assert rc == code and word in _lib.last_error(), (rc, _lib.last_error())
    assert sum(_lib.routes(reset=True).values()) == 0


def test_misaligned_pointers_are_refused():
    """C or resid below 8-byte alignment (16 for fp32 outputs) is refused by every non-gated entry point, as the gated one always did; every pointer
    handed over still lies inside a guarded allocation, and the allocation keeps its sentinel."""
    lib = _lib.load()
    M, N, K = 17, 64, 64
    a = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    rt = torch.zeros(256 + 8, 2, device=DEV)
    s = torch.zeros(N, device=DEV)
    part = torch.zeros(M * N // 64, 2, device=DEV)
    buf, view = GC.make_window(M, N, N + 16, 8, torch.bfloat16, device=DEV)
    fbuf, fview = GC.make_window(M, N, N + 8, 4, torch.float32, device=DEV)
    good, odd = view.data_ptr(), C.c_void_p(view.data_ptr() + 2)
    A, W, st = _lib.ptr(a), _lib.ptr(w), _lib.stream_ptr()
    refused(lambda: lib.visrep_gemm_bf16(A, K, W, K, None, odd, N + 16, M, N, K, _lib.EPI_BIAS, 0, None, None, st), -1, "8-byte aligned")
    refused(lambda: lib.visrep_gemm_bf16(A, K, W, K, None, C.c_void_p(good + 4), N + 16, M, N, K, _lib.EPI_VT, 0, None, None, st), -1, "8-byte aligned")
    refused(lambda: lib.visrep_gemm_bf16(A, K, W, K, None, C.c_void_p(good), N + 16, M, N, K, _lib.EPI_RESID, 0, odd, None, st), -1, "resid must be 8-byte aligned")
    refused(lambda: lib.visrep_gemm_bf16(A, K, W, K, None, C.c_void_p(fview.data_ptr() + 8), N + 8, M, N, K, _lib.EPI_F32, 0, None, None, st), -1, "16-byte aligned")
    refused(lambda: lib.visrep_gemm_bf16_ln(A, K, W, K, None, _lib.ptr(rt), _lib.ptr(s), odd, N + 16, M, N, K, _lib.EPI_BIAS, 0, st), -1, "8-byte aligned")
    refused(lambda: lib.visrep_gemm_bf16_rows(A, K, 4, 4, 0, W, K, None, None, None, odd, N + 16, M, N, K, _lib.EPI_BIAS, 0, st), -1, "8-byte aligned")
    refused(lambda: lib.visrep_gemm_bf16_resid_stats(A, K, W, K, None, odd, N + 16, M, N, K, odd, None, _lib.ptr(rt), _lib.ptr(part), 1e-6, st), -1, "8-byte aligned")
    refused(lambda: lib.visrep_gemm_bf16_resid_stats(A, K, W, K, None, C.c_void_p(good), N + 16, M, N, K, odd, None, _lib.ptr(rt), _lib.ptr(part), 1e-6, st), -1,
            "resid must be 8-byte aligned")
    assert GC.stray_writes(buf, 0, N, 8) == 0 and GC.stray_writes(fbuf, 0, N, 4) == 0      # (M = 0: the whole buffer counts as outside)


def test_rms_statistics_entry_refuses_an_unaligned_window():
    """visrep_gemm_bf16_resid_rms_stats documents ldc % 8 == 0 and a 16-byte aligned C (its read-back route loads 16 bytes at a time)."""
    lib = _lib.load()
    M, N, K = 17, 256, 64
    a = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(N, K, dtype=torch.bfloat16, device=DEV)
    rt = torch.zeros(M, 2, device=DEV)
    part = torch.zeros(M * N // 64, 2, device=DEV)
    A, W, st = _lib.ptr(a), _lib.ptr(w), _lib.stream_ptr()
    for win in ("l4", "a8"):
        extra, col0 = GC.WINDOWS[win]
        buf, view = GC.make_window(M, N, N + extra, col0, torch.bfloat16, device=DEV)
        refused(lambda: lib.visrep_gemm_bf16_resid_rms_stats(A, K, W, K, None, ptr_at(view), N + extra, M, N, K, ptr_at(view), None, _lib.ptr(rt), _lib.ptr(part),
                                                            1e-6, st), -2, "16-byte aligned")
        assert GC.stray_writes(buf, 0, N, col0) == 0
