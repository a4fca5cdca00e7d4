"""The GEMM epilogue contract suite proved on the CPU (no GPU needed): the oracle holds its own bound for an fp32 emulation of every case of
the table, the activation allowance holds for the device formulas on a dense grid, every listed mutation of the emulation leaves the bound
(the suite can fail), the table contains what it claims, and the sentinel window sees a single stray 8-byte store on every side.
Oracle, bound, table: tests/_gemm_cases.py."""
import os
import sys
from collections import defaultdict

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _gemm_cases as GC  # noqa: E402

HOST_CUS = 8              # head-plus-tail cases: the oracle and the bound do not depend on how many full rounds precede the edge rows


def rows_of(case):
    return GC.head_tail_rows(HOST_CUS, case) if case.group == "headtail" else case.M


def epilogue_key(case):
    return case.kind + ("-" + case.act if case.act else "") + ("-ls" if case.ls else "") + ("-ln" if case.ln else "") + ("-" + case.stats if case.stats else "")


def to_bf16(v, truncate=False):
    if truncate:                                               # the mutation: drop the low 16 bits instead of rounding to nearest even
        return (v.float().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    return v.to(torch.bfloat16)


def emulate(case, inp, M, mut=None, unrounded=False):
    """The operation in fp32 with bf16 rounding (torch fp32 matmul, fp32 epilogue, .to(bfloat16)) -> logical [M, N] float64.
    mut: one of the mutations of test_mutations_are_caught.  unrounded: the fp32 value before the output rounding."""
    idx = GC.row_index(case, M)
    acc = inp["a"].float()[idx] @ inp["w"].float().t()
    bias = inp["bias"].clone()
    if mut == "drop_bias_block":
        bias[16:32] = 0.0
    if case.ln:
        rt, s = inp["ln"][0][idx], inp["ln"][1]
        if mut == "ln_neighbour_rt":
            rt = rt.clone()
            rt[5] = inp["ln"][0][idx][6]
        z = rt[:, :1] * acc + (rt[:, 1:2] * s + bias)
    else:
        z = acc + bias
    if case.kind == "act":
        z = GC.act_device_formula_fp32(case.act, z)
    if case.kind == "resid":
        r = inp["resid"].float()
        if mut == "resid_next_row":
            r = r.clone()
            r[5] = inp["resid"].float()[6]
        if case.ls and mut != "skip_ls":
            z = z * inp["ls"]
        z = z + r
    if unrounded:
        return z.double()
    y = z if case.kind == "f32" else to_bf16(z, mut == "truncate")
    if mut == "swap_groups":
        y = y.clone()
        y[5, 4:8], y[5, 8:12] = y[5, 8:12].clone(), y[5, 4:8].clone()
    if case.kind == "vt":                                      # through the stored layout and back: proves vt_unpermute against the scatter
        ld, col0 = GC.window_of(case, M)
        buf, _ = GC.make_window(M, case.N, ld, col0, torch.bfloat16, vt=True)
        cols = torch.tensor([col0 + (m if (mut == "vt_unswapped" and m < 16) else GC.perm16(m)) for m in range(M)])
        buf[GC.VT_GUARD_ROWS:GC.VT_GUARD_ROWS + case.N, cols] = y.t()
        assert GC.stray_writes(buf, M, case.N, col0, vt=True) == 0
        y = GC.vt_unpermute(buf, M, col0, GC.VT_GUARD_ROWS, case.N)
    return y.double()


def worst_ratio(got, want, bound):
    return ((got - want).abs() / bound.clamp_min(1e-300)).max().item()


def test_reference_within_its_own_bound():
    worst, arith = defaultdict(float), defaultdict(float)
    stat_worst = defaultdict(float)
    for case in GC.ALL_CASES:
        M = rows_of(case)
        inp = GC.make_inputs(case, M)
        want, bound = GC.reference_for(case, inp, M)
        got = emulate(case, inp, M)
        assert want.shape == (M, case.N) and torch.isfinite(want).all() and (bound > 0).all()
        r = worst_ratio(got, want, bound)
        assert r < 1.0, (case.id, r)
        worst[epilogue_key(case)] = max(worst[epilogue_key(case)], r)
        ra = worst_ratio(emulate(case, inp, M, unrounded=True), want, GC.arithmetic_bound(case.kind, want, bound))
        arith[epilogue_key(case)] = max(arith[epilogue_key(case)], ra)
        if case.stats:
            x = got.to(torch.bfloat16)
            rt, rb = GC.row_stats_reference(x, GC.STATS_EPS, case.stats == "rms")
            emu = GC.one_pass_stats_fp32(x, GC.STATS_EPS, case.stats == "rms").double()
            ok = rb > 0
            sr = ((emu - rt).abs()[ok] / rb[ok]).max().item()
            assert ((emu - rt).abs() <= rb).all() and sr < 1.0, (case.id, sr)
            stat_worst[(case.stats, case.N, case.dist)] = max(stat_worst[(case.stats, case.N, case.dist)], sr)
            ratio = (x.double().mean(1).abs() / x.double().std(1, unbiased=False))
            if case.dist == "offset":
                assert ratio.min() >= 5.0, (case.id, ratio.min().item())
                # the bound has visibly grown: at least 20 times the bound of a row with the same spread around zero
                centred, cb = GC.row_stats_reference((x.double() - x.double().mean(1, keepdim=True)).to(torch.bfloat16), GC.STATS_EPS, False)
                if case.stats == "ln":
                    assert (rb[:, 0] / rt[:, 0]).min() > 20 * (cb[:, 0] / centred[:, 0]).max(), case.id
            print(f"[gemm-cases] {case.id}: |mean| / std of the written rows {ratio.min().item():.2f} .. {ratio.max().item():.2f}, statistics emulation err/bound {sr:.4f}")
    for k in sorted(worst):
        print(f"[gemm-cases] worst CPU-emulation err/bound  {k:28s} {worst[k]:.4f}   before the output rounding, against the arithmetic part alone {arith[k]:.4f}")
    for k in sorted(stat_worst):
        print(f"[gemm-cases] worst one-pass fp32 statistics err/bound {k}: {stat_worst[k]:.4f}")
    # the rounded ratio approaches 1 by construction (2^-8 |y| is attained on rounding ties, see the case module); the arithmetic must not
    assert max(worst.values()) < 1.0
    assert max(arith.values()) < 0.5, "a ratio near 1 from the emulation's arithmetic alone means the bound is wrong, not tight"


@pytest.mark.parametrize("name", GC.ACTS)
def test_activation_allowance_on_a_dense_grid(name):
    """The device formulas in fp32 against the exact activation in float64: inside the derived allowance everywhere; and the Lipschitz constant
    the bound propagates the argument's error with really bounds the derivative."""
    x = torch.cat([torch.linspace(-24.0, 24.0, 1_200_001), torch.linspace(-1.0, 1.0, 400_001), torch.linspace(-88.0, 88.0, 20_001)]).float()
    want = GC.act_exact(name, x)
    got = GC.act_device_formula_fp32(name, x).double()
    assert torch.isfinite(got).all()
    allow = GC.act_allowance(name, x)
    ratio = ((got - want).abs() / allow)
    i = ratio.argmax()
    print(f"[gemm-cases] {name}: worst fp32-formula err/allowance {ratio[i].item():.3f} at x = {x[i].item():.4f} (err {(got - want).abs()[i].item():.3e})")
    assert ratio.max() <= 1.0
    # the allowance is at most a quarter of the output rounding wherever the output is not tiny: it cannot hide a wrong activation
    big = want.abs() > 1e-3
    assert (allow[big] < 2.0 ** -10 * want.abs()[big]).all()
    xd = torch.linspace(-12.0, 12.0, 2_400_001, dtype=torch.float64)
    slope = (GC.act_exact(name, xd)[1:] - GC.act_exact(name, xd)[:-1]).abs() / (xd[1] - xd[0])
    print(f"[gemm-cases] {name}: sup |act'| on the grid {slope.max().item():.5f} <= L = {GC.LIPSCHITZ[name]}")
    assert slope.max() <= GC.LIPSCHITZ[name] and slope.max() > GC.LIPSCHITZ[name] - 0.01


def representative(pred):
    return next(c for c in GC.ALL_CASES if pred(c) and c.M >= 17 and c.group != "headtail")


MUTATIONS = [
    ("swap_groups", lambda c: True),
    ("drop_bias_block", lambda c: True),
    ("truncate", lambda c: c.kind != "f32"),
    ("resid_next_row", lambda c: c.kind == "resid"),
    ("skip_ls", lambda c: c.kind == "resid" and c.ls),
    ("ln_neighbour_rt", lambda c: c.ln),
    ("vt_unswapped", lambda c: c.kind == "vt"),
]
EPILOGUES = [
    ("bias", lambda c: c.kind == "bias" and not c.ln), ("bias-ln", lambda c: c.kind == "bias" and c.ln),
    ("act-quick_gelu", lambda c: c.act == "quick_gelu" and not c.ln), ("act-gelu", lambda c: c.act == "gelu" and not c.ln),
    ("act-gelu_tanh", lambda c: c.act == "gelu_tanh" and not c.ln), ("act-ln", lambda c: c.kind == "act" and c.ln),
    ("resid", lambda c: c.kind == "resid" and not c.ls and not c.stats), ("resid-ls", lambda c: c.kind == "resid" and c.ls and not c.stats),
    ("f32", lambda c: c.kind == "f32"), ("vt", lambda c: c.kind == "vt" and not c.ln), ("vt-ln", lambda c: c.kind == "vt" and c.ln),
]


def test_mutations_are_caught():
    """Each mutation of the fp32 emulation must fall outside the bound somewhere, for a representative case of every epilogue it applies to."""
    caught = []
    for name, pred in EPILOGUES:
        case = representative(pred)
        M = case.M
        inp = GC.make_inputs(case, M)
        want, bound = GC.reference_for(case, inp, M)
        assert worst_ratio(emulate(case, inp, M), want, bound) < 1.0
        for mut, applies in MUTATIONS:
            if not applies(case):
                continue
            bad = emulate(case, inp, M, mut)
            n = int(((bad - want).abs() > bound).sum())
            print(f"[gemm-cases] mutation {mut:16s} on {name:15s} ({case.id}): {n} elements outside the bound - caught" if n else f"NOT caught: {mut} on {case.id}")
            assert n > 0, (mut, case.id)
            caught.append((name, mut))
    assert {m for _, m in caught} == {m for m, _ in MUTATIONS}
    for st in ("ln", "rms"):                                   # statistics: the mean over N - 4 columns (RMS: the sum of squares over N - 4)
        for dist in ("plain", "offset"):
            case = next(c for c in GC.STATS if c.stats == st and c.dist == dist and c.N == 1024)
            inp = GC.make_inputs(case)
            x = emulate(case, inp, case.M).to(torch.bfloat16)
            rt, rb = GC.row_stats_reference(x, GC.STATS_EPS, st == "rms")
            if st == "ln":
                bad = GC.one_pass_stats_fp32(x, GC.STATS_EPS, False, drop_cols=4).double()
                lost = GC.one_pass_stats_fp32(x, GC.STATS_EPS, False, drop_cols=4, renorm=False).double()
                assert ((lost - rt).abs() > rb).any(1).float().mean() >= (1.0 if dist == "offset" else 0.9), (st, dist)   # a sum that lost four columns
            else:
                bad = GC.one_pass_stats_fp32(x[:, :-4], GC.STATS_EPS, True).double()
            n = int(((bad - rt).abs() > rb).any(1).sum())
            print(f"[gemm-cases] mutation mean_over_N-4 on {st} statistics, {dist} rows: {n} of {case.M} rows outside the bound - caught")
            # "Somewhere" is what is required, half the rows is what is asserted.  The average of N - 4 columns is a WEAK mutation for the LayerNorm
            # statistics: it moves the mean by (mean of the dropped four - mean) * 4 / N, about 2 std / N, which the one-pass bound (N u E[x^2]
            # on var) separates on most rows only, plain or offset.  The mutation with separating power is the sum that LOST four columns
            # (mean = s1' / N, asserted above on every offset row and nine plain rows in ten): the bug a kernel that drops a quad would have.
            assert n >= case.M // 2, (st, dist, n)


def test_table_covers_what_it_claims():
    ids = [c.id for c in GC.ALL_CASES]
    assert len(set(ids)) == len(ids)
    for c in GC.ALL_CASES:                                     # the stated kernel family is what the dispatcher's rule gives; fallbacks are named
        assert GC.expected_family(c) == c.route, c.id
        fallback = c.variant >= 6 and c.route != "headtail" and c.K < 1024 and not (c.N % 128 == 0 and c.K >= 128 and c.kind != "f32" and c.rows is None)
        assert bool(c.note) == fallback, c.id
        ldc, col0 = GC.window_of(c, rows_of(c))
        assert ldc % 4 == 0 and GC.c_offset_bytes(rows_of(c), c.N, ldc, col0, torch.float32 if c.kind == "f32" else torch.bfloat16, c.kind == "vt") % (16 if c.kind == "f32" else 8) == 0
    tile = [c for c in GC.ALL_CASES if c.route in ("128", "256")]
    rm_keys = {epilogue_key(c) for c in tile if c.kind in ("bias", "act", "resid") and not c.stats}
    assert rm_keys == {"bias", "bias-ln", "act-quick_gelu", "act-gelu", "act-gelu_tanh", "act-gelu-ln", "act-quick_gelu-ln", "act-gelu_tanh-ln", "resid", "resid-ls"}
    for key in ("bias", "bias-ln", "act-quick_gelu", "act-gelu", "act-gelu_tanh", "resid", "resid-ls"):
        cs = [c for c in tile if epilogue_key(c) == key]
        for fam in ("128", "256"):
            assert {GC.is_al(c) for c in cs if c.route == fam} == {True, False}, (key, fam)
            assert any(c.M >= GC.wave_rows(c) for c in cs if c.route == fam) and any(c.M % GC.wave_rows(c) for c in cs if c.route == fam), (key, fam)
    assert {GC.is_al(c) for c in tile if c.kind == "act" and c.ln} == {True, False}
    # out-of-place residual: the third operand flips `al` both ways
    assert {(c.resid, GC.is_al(c)) for c in tile if c.kind == "resid"} >= {("in", True), ("in", False), ("same", True), ("same", False), ("r8", False), ("c8", False)}
    assert {c.route for c in tile if c.resid == "r8"} == {"128", "256"}
    # F32: interior and edge tiles on both families, windowed
    f32 = [c for c in tile if c.kind == "f32"]
    assert {(c.route, c.win) for c in f32} >= {("128", "f4"), ("256", "f4"), ("128", "c"), ("256", "c")}
    # V^T: wide and narrow x {m + 8 < M, m + 8 == M, M % 4 != 0}, with and without the fold
    vt = [c for c in tile if c.kind == "vt"]
    tails = lambda c: ("m+8==M" if c.M % 16 == 8 else None, "M%4" if c.M % 4 else None, "m+8<M" if c.M > 16 else None)
    for wide in (True, False):
        seen = {t for c in vt if GC.is_al(c) == wide for t in tails(c) if t}
        assert seen == {"m+8==M", "M%4", "m+8<M"}, (wide, seen)
    assert {(GC.is_al(c), c.route) for c in vt if c.ln} >= {(True, "128"), (True, "256"), (False, "256")}
    # kernel families: every variant the product build accepts runs a 256-wide kernel somewhere, for every epilogue it serves
    assert {(c.variant, c.kind) for c in tile if c.route == "256"} >= {(v, k) for v in (2, 5, 6, 7, 8) for k in ("bias", "act", "resid", "vt")}
    assert {c.kind for c in tile if c.variant == 1} >= {"bias", "act", "resid", "vt", "f32"}
    assert {c.M for c in GC.ROWMAJOR} == {1, 17, 127, 129, 255, 257, 300} and {c.N for c in GC.ROWMAJOR} == {64, 128, 192, 256, 512}
    assert {c.K for c in tile} == {64, 128, 192}
    # every reduce kernel with a window: splitk_reduce (each row-major epilogue + F32 + the fold), splitk_reduce_vt, splitk_reduce_rms
    sk = [c for c in GC.ALL_CASES if c.route == "splitk"]
    assert all(c.win != "c" and c.K == 1024 for c in sk)
    assert {epilogue_key(c) for c in sk} >= {"bias", "bias-ln", "act-gelu", "resid", "resid-ls", "f32", "vt", "vt-ln", "resid-ln", "resid-ls-ln", "resid-rms", "resid-ls-rms"}
    assert {GC.is_al(c) for c in sk if c.kind == "vt"} == {True, False} and any(c.M % 4 for c in sk if c.kind == "vt")
    # statistics: both entries x both routes x both row distributions x LayerScale on / off
    assert {(c.stats, c.N, c.dist, c.ls) for c in GC.STATS} == {(s, n, d, l) for s in ("ln", "rms") for n in (256, 1024) for d in ("plain", "offset") for l in (True, False)}
    # head plus tail: every row-major epilogue and V^T, all windowed;  row maps: two maps, one with period % 16 != 0, windowed
    assert {c.kind for c in GC.HEADTAIL} == set(GC.KINDS) and all(c.win != "c" and c.N == 256 and c.K == 64 for c in GC.HEADTAIL)
    assert {c.rows for c in GC.ROWS} == {GC.MAP_A, GC.MAP_B} and GC.MAP_A[0] % 16 and all(c.win != "c" for c in GC.ROWS)
    assert {c.kind for c in GC.ROWS} == {"bias", "act", "vt", "f32"}


def test_no_case_is_skipped_by_the_gpu_file():
    """Every case of the table is a parameter of exactly one test of the GPU module, and no test there (nor the module) carries a mark other than
    `gpu` and `parametrize` - read from the imported module's marks, not from its text."""
    import test_gpu_gemm_contract as G
    marks = lambda obj: [m for m in (getattr(obj, "pytestmark", []) if isinstance(getattr(obj, "pytestmark", []), list) else [obj.pytestmark])]
    assert [m.name for m in marks(G)] == ["gpu"]
    seen = []
    for name, fn in vars(G).items():
        if not name.startswith("test_"):
            continue
        assert {m.name for m in marks(fn)} <= {"parametrize"}, name
        for m in marks(fn):
            assert m.args[0] == "case" and len(m.kwargs["ids"]) == len(m.args[1])
            assert list(m.kwargs["ids"]) == [c.id for c in m.args[1]], name
            seen += list(m.args[1])
    assert len(seen) == len(GC.ALL_CASES) and set(seen) == set(GC.ALL_CASES)


@pytest.mark.parametrize("vt,dtype", [(False, torch.bfloat16), (False, torch.float32), (True, torch.bfloat16)])
def test_window_helper_detects_a_single_stray_store(vt, dtype):
    M, N, col0 = 21, 64, 8
    ldc = GC.vt_min_ld(M, col0) + 8 if vt else N + 16
    per8 = 2 if dtype == torch.float32 else 4                  # elements of one 8-byte store
    buf, view = GC.make_window(M, N, ldc, col0, dtype, vt=vt)
    r0, r1, c0, c1 = GC.window_box(M, N, col0, vt)
    assert view.shape == (r1 - r0, c1 - c0) and view.data_ptr() == buf[r0, c0:].data_ptr() and r0 >= 1 and buf.shape[0] - r1 >= 2
    assert torch.isnan(buf.float()).all() and GC.stray_writes(buf, M, N, col0, vt) == 0
    buf[GC.window_mask(buf, M, N, col0, vt)] = 1.5             # the whole window written: still nothing stray
    view[0, 0] = float("nan")
    assert GC.stray_writes(buf, M, N, col0, vt) == 0
    c1 = c0 + 24 if vt else c1                                 # V^T, M = 21: tokens 0 .. 23 are stored in columns 0 .. 19 and 24 .. 27 of the window
    spots = {"above": (r0 - 1, c0), "below": (r1, c1 - per8), "two below": (r1 + 1, c0), "left": (r0, c0 - per8), "right": (r1 - 1, c1 + 4 if vt else c1),
             "first element of the buffer": (0, 0), "last elements of the buffer": (buf.shape[0] - 1, ldc - per8)}
    for value in (0.0, float("nan"), float("inf")):            # a NaN written outside must be seen too (bitwise comparison, not isnan)
        for where, (r, c) in spots.items():
            b2 = buf.clone()
            b2[r, c:c + per8] = value
            assert GC.stray_writes(b2, M, N, col0, vt) == per8, (where, value)
    if vt:                                                     # V^T: tokens 21 .. 23 (stored with token 20 in columns 24 .. 27) belong to the window,
        b2 = buf.clone()                                       # the unwritten groups of the last block (columns 20 .. 23, 28 .. 31) do not
        b2[r0, c0 + 24:c0 + 28] = 0.0
        assert GC.stray_writes(b2, M, N, col0, vt) == 0
        for c in (20, 28):
            b2 = buf.clone()
            b2[r0 + 3, c0 + c:c0 + c + 4] = 0.0
            assert GC.stray_writes(b2, M, N, col0, vt) == 4, c


def test_perm16_is_the_documented_order():
    assert [GC.perm16(m) for m in range(16)] == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]
    assert GC.perm16(37) == 32 + GC.perm16(5) and sorted(GC.perm16(m) for m in range(64)) == list(range(64))
