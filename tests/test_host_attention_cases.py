"""tests/_attention_cases.py is what it claims (no GPU): buffers bf16-exact and windows aligned, the case tables cover what they say, the
growth cases produce their exponent gaps in float64, the oracle equals a naive per-image loop, the rounding model - the reference alone -
stays inside the bound the GPU test holds the kernels to, and the entry points refuse what they must before any device work."""
import ctypes as C
import itertools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _attention_cases as AC  # noqa: E402

from law_of_vision_representation_in_mllms_amd import _lib  # noqa: E402

ids = lambda cases: [c.id for c in cases]


def test_bf16_helpers_and_perm16():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.14159, 3000.0, 1e30, 2.0 ** -130])
    r = AC.bf16_round(x)
    assert r[0] == 1.0 and r[1] == 1.0 and r[2] == 1.0 + 2.0 ** -6 and abs(r[3] + 3.14159) <= 2.0 ** -7      # ties to even, both ways
    assert np.array_equal(AC.bf16_from_bits(AC.bf16_bits(r)), r)
    with pytest.raises(AssertionError):
        AC.bf16_bits(np.array([1.0 + 2.0 ** -9]))
    assert not AC.finite_bits(np.array([AC.NAN_BITS])).any() and AC.finite_bits(np.array([AC.PAD_POS, AC.PAD_NEG, 0])).all()
    m = np.arange(1024)
    other = (m & ~15) | (((m >> 2) & 1) << 3) | (((m >> 3) & 1) << 2) | (m & 3)       # the statement of tests/test_gpu_cu_counts.py
    assert np.array_equal(AC.perm16(m), other) and sorted(AC.perm16(m)) == list(m)
    assert list(AC.perm16(np.arange(16))) == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]


def test_table_sizes_and_coverage():
    assert (len(AC.EDGE_GRID), len(AC.CLS_GRID), len(AC.WIDE_GRID), len(AC.GROWTH), len(AC.EXACT), len(AC.REFUSALS)) == (81, 24, 48, 38, 12, 23)
    edge = AC.EDGE_GRID
    rows = [(c.Tq, c.Tk, c.route, c.shared, c.causal) for c in edge]
    factors = (AC.TQS, AC.TKS, AC.EDGE_ROUTES, (0, 1), (0, 1))
    for i, j in itertools.combinations(range(5), 2):                                   # pairwise cover
        assert {(r[i], r[j]) for r in rows} == set(itertools.product(factors[i], factors[j])), (i, j)
    assert any(c.causal and c.Tq < c.Tk for c in edge) and any(c.causal and c.Tq > c.Tk for c in edge)
    assert any(c.causal and c.shared for c in edge)
    for tk in AC.TKS:                                                                  # start residues actually reached
        got = set()
        for c in edge:
            if c.Tk == tk and not c.shared:
                got |= {b * tk % 64 for b in range(c.B)}
        need = AC.required_residues(tk)
        assert set(need) <= got, (tk, need, sorted(got))
        assert len(need) >= (1 if tk == 64 else 5), (tk, need)
    assert any(c.Tk == 1 and c.B == 130 for c in edge) and any(c.Tk == 3 and c.B == 50 for c in edge)
    big = sorted(c.B * c.Tq for c in edge)
    assert big[-1] <= 2500
    assert {(c.Tq, c.B, c.H) for c in AC.CLS_GRID} == set(itertools.product((65, 129, 257, 577), (1, 3, 70), (1, 3)))
    assert {(c.Tk, c.Tq, c.H, c.shared) for c in AC.WIDE_GRID} == set(itertools.product((64, 128, 576), (1, 96, 130, 300), (1, 2), (0, 1)))
    seen = {(c.route, lay) for grid in (edge, AC.CLS_GRID, AC.WIDE_GRID) for c, lay in AC.grid_layouts(grid)}
    assert seen == set(itertools.product(AC.ROUTE_D, AC.LAYOUTS))                      # every route under every layout
    for c in AC.GROWTH:
        if c.kind == "wgrow":
            assert c.param[2] in (1, 2)
    assert {c.param[2] for c in AC.GROWTH if c.kind == "wgrow"} == {1, 2}              # growth in a middle tile and in the LAST tile
    assert {(c.route, c.kind) for c in AC.EXACT} == set(itertools.product(AC.ROUTE_D, ("ones", "qzero")))


PACK_CASES = AC.GROWTH[::5] + AC.EXACT + AC.EDGE_GRID[::9] + AC.CLS_GRID[:2] + AC.WIDE_GRID[:2]


@pytest.mark.parametrize("layout", AC.LAYOUTS)
@pytest.mark.parametrize("case", PACK_CASES, ids=ids(PACK_CASES))
def test_packed_buffers(case, layout):
    """Values bf16-exact; q / k / vt pointers 16-byte aligned, out / vcls 8-byte; the leading dimensions pass the ABI's own conditions; the
    windows hold the values and everything else the NaN pattern (V^T: +- the largest finite bf16); the store path is the one the layout names."""
    inp = AC.make_inputs(case)
    for n in ("q", "k", "v"):
        assert np.array_equal(AC.bf16_round(inp[n]), inp[n])
    p = AC.pack(inp, case, layout)
    d, bufs, HD = p["dims"], p["bufs"], p["HD"]
    assert d["ldq"] % 8 == 0 and d["ldk"] % 8 == 0 and d["ldvt"] % 64 == 0 and d["ldo"] % 4 == 0 and d["ldvc"] % 4 == 0
    assert bufs["q"][1] * 2 % 16 == 0 and bufs["vt"][1] == 0 and bufs["out"][1] * 2 % 8 == 0
    wide_store = d["ldo"] % 8 == 0 and bufs["out"][1] * 2 % 16 == 0
    assert wide_store == (layout in ("tight", "window"))
    q, qoff = bufs["q"]
    qw = 2 * HD if case.route == "cls" else HD
    assert AC.finite_bits(q[:p["M"] if case.route != "cls" else case.B * case.Tk, qoff:qoff + qw]).all()
    assert (np.delete(q, np.s_[qoff:qoff + qw], 1) == AC.NAN_BITS).all()
    vt = bufs["vt"][0]
    nkeys = case.B * (case.Tk - 1) if case.route == "cls" else (case.Tk if case.shared else case.B * case.Tk)
    cols = AC.perm16(np.arange(nkeys))
    rest = np.delete(vt, cols, 1)
    assert AC.finite_bits(vt).all() and ((rest == AC.PAD_POS) | (rest == AC.PAD_NEG)).all() and rest.shape[1] == d["ldvt"] - nkeys
    v2 = inp["v"].reshape(-1, HD)
    if case.route == "cls":
        v2 = v2[np.arange(case.B * case.Tk) % case.Tk != 0]
        vc, off = bufs["vcls"]
        assert off * 2 % 8 == 0 and np.array_equal(AC.bf16_from_bits(vc[:, off:off + HD]), inp["v"][:, 0].reshape(case.B, HD))
    else:
        k, koff = bufs["k"]
        assert koff * 2 % 16 == 0 and k.shape[0] == nkeys + 70 and (k[nkeys:] == AC.NAN_BITS).all()
        assert np.array_equal(AC.bf16_from_bits(k[:nkeys, koff:koff + HD]), inp["k"].reshape(-1, HD))
    assert np.array_equal(AC.bf16_from_bits(vt[:, cols]), v2.T)
    out, lead = bufs["out"]
    assert (out == AC.NAN_BITS).all()
    w = AC.out_window(out, p)
    assert w.shape == (p["M"], HD)
    out[lead + HD if d["ldo"] > HD else lead - 1] = 0                                  # a stray write just outside the window is seen
    with pytest.raises(AssertionError, match="outside the output window"):
        AC.out_window(out, p)


def naive(inp, case):
    """softmax(QK^T scale) V, one (image, head, query) at a time with math.exp."""
    q, k, v = inp["q"], inp["k"], inp["v"]
    out = np.zeros_like(q)
    for b, h, i in itertools.product(range(case.B), range(case.H), range(case.Tq)):
        kb = 0 if case.shared else b
        keys = [t for t in range(case.Tk) if not (case.causal and t > i)]
        s = [float(q[b, i, h] @ k[kb, t, h]) for t in keys]
        if case.route in AC.PRESCALED:
            w = [2.0 ** (x - max(s)) for x in s]
        else:
            w = [math.exp((x - max(s)) * inp["scale"]) for x in s]
        out[b, i, h] = sum(wi * v[kb, t, h] for wi, t in zip(w, keys)) / sum(w)
    return out


TINY = (AC.Case("d64", 2, 5, 7, 2, 0, 1, seed=1), AC.Case("d128", 3, 4, 3, 1, 1, 0, seed=2), AC.Case("cls", 2, 65, 65, 1, seed=3))


@pytest.mark.parametrize("case", TINY, ids=ids(TINY))
def test_oracle_equals_naive_loop(case):
    inp = AC.make_inputs(case)
    O, A, L = AC.oracle(inp, case)
    want = naive(inp, case)
    assert np.abs(O - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    assert (A >= np.abs(O) - 1e-15).all() and L > 0


@pytest.mark.parametrize("case", AC.GROWTH, ids=ids(AC.GROWTH))
def test_growth_cases_produce_their_gaps(case):
    inp = AC.make_inputs(case)
    f = AC.growth_figures(inp, case)
    if case.kind == "wgrow":
        g = case.param[0]
        assert (np.abs(f["gap"] - g) < 0.5).all() and ((f["gap"] > 100.0) == (g > 100)).all(), f["gap"]
        assert (f["other_gap"] == 0).all()                  # untouched rows: the first tile holds their maximum (no repeat of their own)
        if g > 0:
            assert f["tile"] == case.param[2]
        absent = AC.growth_figures(AC.make_inputs(case, absent=True), case)
        assert (absent["gap"] == 0).all() and (absent["other_gap"] == 0).all()
    elif case.kind == "stair":
        step = case.param[0]
        assert f["steps"].shape[1] == 8 and (np.abs(f["steps"] - step) < 0.45).all() and ((f["steps"] > 8.0) == (step > 8.0)).all(), f["steps"]
    elif case.kind == "onelane":
        assert f["row"] > 8.0 and (f["others"] < 0).all(), (f["row"], f["others"].max())
    elif case.kind == "shift":
        assert (np.abs(f["first"] - case.param[0]) < 50).all()
    else:
        assert (f["gap"] * np.sign(case.param[0]) > 2900).all()


MODEL_CASES = AC.GROWTH + AC.EXACT


@pytest.mark.parametrize("case", MODEL_CASES, ids=ids(MODEL_CASES))
def test_rounding_model_stays_inside_the_bound(case):
    inp = AC.make_inputs(case)
    got = AC.rounding_model(inp, case)
    O, A, L = AC.oracle(inp, case)
    r = AC.ratio(got, O, A, L)
    print(f"[attn-model] {case.id}: ratio {r:.3f} (L = {L:.1f})")
    assert r <= 1.0
    if case.kind in ("ones", "qzero"):
        want, bnd = AC.exact_bound(inp, case)
        assert (np.abs(got - want) <= bnd).all(), float((np.abs(got - want) / bnd).max())


@pytest.mark.parametrize("spread", [1.0, 6.0, 25.0])
def test_rounding_model_at_score_spreads(spread):
    """N(0, 1) values at score spreads 1, 6, 25 (peaked rows, late keys that overtake the reference), every head width."""
    for route in AC.ROUTE_D:
        T = 129 if route == "cls" else 128
        case = AC.Case(route, 2, T, T, 1, seed=int(spread))
        inp = AC.make_inputs(case)
        inp["k"] = AC.bf16_round(inp["k"] * spread)
        O, A, L = AC.oracle(inp, case)
        r = AC.ratio(AC.rounding_model(inp, case), O, A, L)
        print(f"[attn-model] {route} spread {spread}: ratio {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("name,entry,over,rc,msg", AC.REFUSALS, ids=[r[0] for r in AC.REFUSALS])
def test_refusals_happen_before_any_device_work(name, entry, over, rc, msg):
    """Return code and message of every refusal, with pointers that point nowhere: the checks run before anything touches the device."""
    lib = _lib.load()
    fn = {"attn": lib.visrep_attention_fwd, "cls": lib.visrep_mhsa_cls_fwd, "mhsa": lib.visrep_mhsa_fwd}[entry]
    args = AC.refusal_args(entry, over, 0x7F0000001000)
    _lib.routes(reset=True)
    assert fn(*args, None) == rc, _lib.last_error()
    assert msg in _lib.last_error(), _lib.last_error()
    assert not any(_lib.routes(reset=True).values())
