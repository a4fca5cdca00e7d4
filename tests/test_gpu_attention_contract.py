"""Contract of the bf16 attention kernels (csrc/attention.hip) through the C ABI with ctypes: float64 oracle, derived per-element bound,
every edge.  Cases, packers, oracle and the derivation of the bound are in tests/_attention_cases.py (checked without a GPU by
tests/test_host_attention_cases.py); every assertion on an error here is `ratio = max |got - O| / bound <= 1`, printed per case
(`[attn-contract]` lines, pytest -s).  A ratio above 1 is a finding to explain from the kernel, not a constant to raise.

Every call: Q / K windows inside NaN-filled buffers, NaN K rows behind the last key, V^T pad columns +-3.4e38, the output a window in a buffer
pre-filled with a NaN pattern - after the call the window is finite and every element outside it still holds the pattern - and the route
counters say which kernel ran.

Worst ratio per route, measured on an MI355X (test_zz_report prints the table of a run; 265 tests, 9 s):
  d64   0.888  (B = 50, Tq = 31, Tk = 3)                    d64ps 0.795  (Tq = 129, Tk = 3, shared, causal)
  d128  0.705  (Tq = 100, Tk = 11, shared)                  d192  0.820  (Tq = 32, Tk = 3, shared, causal)
  cls   0.622  (B = 70, T = 65, H = 1)                      wide  0.962  (growth 60 on every row, in the last key tile)
The worst cases are the ones with the fewest keys (Tk = 3: the bound's u (A + |O|) has nothing to average over) and, for the wide kernel, the
fixed reference 2^60 below the row's maximum."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _attention_cases as AC  # noqa: E402

from law_of_vision_representation_in_mllms_amd import _lib, engine  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}                                 # route -> (ratio, case id, layout) of this run
ids = lambda cases: [c.id for c in cases]


def launch(case, packed, scale, entry=None, finite=True):
    """Upload, call, check the guard and the route counters; returns the output window as bf16 bits [B Tq, H D]."""
    lib = _lib.require_gpu()
    t = {n: torch.from_numpy(a.view(np.int16).copy()).to(DEV) for n, (a, _) in packed["bufs"].items()}
    p = lambda n: C.c_void_p(t[n].data_ptr() + 2 * packed["bufs"][n][1])
    d = packed["dims"]
    torch.cuda.synchronize()
    _lib.routes(reset=True)
    if case.route == "cls":
        rc = lib.visrep_mhsa_cls_fwd(p("q"), d["ldq"], p("vt"), d["ldvt"], p("vcls"), d["ldvc"], p("out"), d["ldo"], case.B, case.Tq, case.H, 64,
                                     _lib.stream_ptr())
    elif entry == "mhsa":
        rc = lib.visrep_mhsa_fwd(p("q"), d["ldq"], p("vt"), d["ldvt"], p("out"), d["ldo"], case.B, case.Tq, case.H, 64, scale, _lib.stream_ptr())
    else:
        rc = lib.visrep_attention_fwd(p("q"), d["ldq"], p("k"), d["ldk"], p("vt"), d["ldvt"], p("out"), d["ldo"], case.B, case.Tq, case.Tk,
                                      case.H, case.D, case.shared, case.causal, scale, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (case.id, _lib.last_error())
    r = _lib.routes(reset=True)
    assert {k: v for k, v in r.items() if v} == {AC.ROUTE_COUNTER[case.route]: 1}, (case.id, r)
    bits = AC.out_window(t["out"].cpu().numpy().view(np.uint16), packed)
    if finite:
        assert AC.finite_bits(bits).all(), f"{case.id}: {int((~AC.finite_bits(bits)).sum())} non-finite outputs"
    return bits


def run(case, layout="tight", inp=None, hostile=True, edit=None, finite=True):
    inp = AC.make_inputs(case) if inp is None else inp
    packed = AC.pack(inp, case, layout, hostile)
    if edit is not None:
        edit(packed)
    return launch(case, packed, inp["scale"], finite=finite)


def values(bits, case):
    return AC.bf16_from_bits(bits).reshape(case.B, case.Tq, case.H, case.D)


def held(case, layouts, inp=None):
    """The case under every layout of `layouts` against the oracle at ratio <= 1; returns the bits of the first layout."""
    inp = AC.make_inputs(case) if inp is None else inp
    O, A, L = AC.oracle(inp, case)
    first = None
    for lay in layouts:
        bits = run(case, lay, inp)
        r = AC.ratio(values(bits, case), O, A, L)
        print(f"[attn-contract] {case.id} {lay}: ratio {r:.3f} (L = {L:.1f})")
        if r > WORST.get(case.route, (0.0,))[0]:
            WORST[case.route] = (r, case.id, lay)
        assert r <= 1.0, (case.id, lay, r)
        first = bits if first is None else first
    return first


def _grid_params(grid):
    lays = {}
    for c, lay in AC.grid_layouts(grid):
        lays.setdefault(c, []).append(lay)
    return [pytest.param(c, tuple(l), id=c.id) for c, l in lays.items()]


@pytest.mark.parametrize("case,layouts", _grid_params(AC.EDGE_GRID))
def test_edge_grid(case, layouts):
    """Tq x Tk x route x kv_shared x causal (pairwise cover, 81 cases): start residues b Tk % 64 of the global key tiles, query tails, Tk = 1
    with 130 images in three key tiles, causal with Tq != Tk and with shared keys at every head width."""
    held(case, layouts)


@pytest.mark.parametrize("case,layouts", _grid_params(AC.CLS_GRID))
def test_cls_grid(case, layouts):
    held(case, layouts)


@pytest.mark.parametrize("case,layouts", _grid_params(AC.WIDE_GRID))
def test_wide_grid(case, layouts):
    held(case, layouts)


@pytest.mark.parametrize("case", AC.GROWTH, ids=ids(AC.GROWTH))
def test_growth(case):
    """The two reference-moving schemes at their thresholds.  attn_fwd_wide: later-tile growth of 0 .. 200 (exp2 units) over the fixed
    first-tile reference around the repeat threshold of 100, on every row / one row of wave 2 / the last row of a 130-row query tail: finite,
    inside the bound, and the rows WITHOUT growth bitwise what they are when the growth row is absent, in both 256-column halves (the two
    workgroups of a query tile take the same repeat decision, and a repeat changes nothing for a row whose reference was its maximum).
    Pre-scaled and plain attn_fwd, attn_fwd_cls: staircases of 7.5 / 8.5 per tile around the move threshold of 8, one lane tripping alone,
    first-tile maxima and CLS scores at +-3000."""
    inp = AC.make_inputs(case)
    bits = held(case, ("tight",), inp)
    if case.kind == "wgrow":
        rows = AC.growth_rows(case)
        others = [r for r in range(case.Tq) if r not in rows]
        base = run(case, "tight", AC.make_inputs(case, absent=True))
        assert np.array_equal(bits[others], base[others]), f"{case.id}: rows without growth differ from the run without the growth row"


@pytest.mark.parametrize("case", AC.EXACT, ids=ids(AC.EXACT))
def test_exact(case):
    """V == 1 -> every output within 2 u of 1 (the design's visible bias, pinned); Q == 0 -> the bf16 rounding of the mean of V over the keys
    (a key counted twice or not at all moves it by |v| / n)."""
    inp = AC.make_inputs(case)
    bits = held(case, ("tight", "narrow_a"), inp)
    want, bnd = AC.exact_bound(inp, case)
    err = np.abs(values(bits, case) - want)
    print(f"[attn-contract] {case.id}: exact ratio {float((err / bnd).max()):.3f}")
    assert (err <= bnd).all(), (case.id, float((err / bnd).max()))


def structure_case(route, H=2):
    """A case whose keys are whole tiles per image (so an image cannot depend on its place in the batch)."""
    if route == "cls":
        return AC.Case("cls", 5, 129, 129, H, seed=40)
    if route == "wide":
        return AC.Case("wide", 3, 130, 128, H, seed=41)
    return AC.Case(route, 4, 70, 128, H, seed=42 + AC.ROUTE_D[route])


def ragged_case(route, H=2):
    """Images that share key tiles with their neighbours where the route allows it."""
    return AC.Case(route, 4, 70, 77, H, seed=50 + AC.ROUTE_D[route]) if route in AC.EDGE_ROUTES else structure_case(route, H)


def image(inp, b):
    return {"q": inp["q"][b:b + 1], "k": inp["k"][b:b + 1], "v": inp["v"][b:b + 1], "scale": inp["scale"]}


@pytest.mark.parametrize("route", list(AC.ROUTE_D))
def test_image_in_batch_equals_image_alone(route):
    case = structure_case(route)
    inp = AC.make_inputs(case)
    full = run(case, "tight", inp).reshape(case.B, case.Tq, -1)
    for b in range(case.B):
        alone = run(case._replace(B=1), "tight", image(inp, b))
        assert np.array_equal(full[b], alone.reshape(case.Tq, -1)), (route, b)


@pytest.mark.parametrize("route", list(AC.ROUTE_D))
def test_neighbours_and_padding_change_nothing(route):
    """Image 1's output is bitwise the same with its neighbours' Q, K, V scaled to 1e30 (finite), and the whole output is bitwise the same
    with K ending at its last row and zero V^T pad columns instead of NaN rows and +-3.4e38."""
    case = ragged_case(route)
    inp = AC.make_inputs(case)
    base = run(case, "window", inp)
    assert np.array_equal(base, run(case, "window", inp, hostile=False))
    loud = {n: inp[n].copy() for n in ("q", "k", "v")}
    for n in loud:
        for b in [b for b in range(case.B) if b != 1]:
            loud[n][b] = AC.bf16_round(np.sign(loud[n][b]) * 1e30 * (1 + np.abs(loud[n][b])))
    loud["scale"] = inp["scale"]
    got = run(case, "window", loud, finite=False)
    assert np.array_equal(got.reshape(case.B, case.Tq, -1)[1], base.reshape(case.B, case.Tq, -1)[1])


@pytest.mark.parametrize("route", list(AC.ROUTE_D))
def test_head_permutation_permutes_output_blocks(route):
    H = 2 if route == "wide" else 3
    case = ragged_case(route, H)
    inp = AC.make_inputs(case)
    perm = [1, 0] if H == 2 else [2, 0, 1]
    pin = {n: np.ascontiguousarray(inp[n][:, :, perm]) for n in ("q", "k", "v")}
    pin["scale"] = inp["scale"]
    a = run(case, "tight", inp).reshape(-1, H, case.D)
    b = run(case, "tight", pin).reshape(-1, H, case.D)
    assert np.array_equal(a[:, perm], b)


@pytest.mark.parametrize("route", list(AC.ROUTE_D))
def test_narrow_store_equals_wide_store(route):
    case = ragged_case(route)._replace(Tq=97)
    if route == "cls":
        case = structure_case(route)
    inp = AC.make_inputs(case)
    wide = run(case, "tight", inp)
    for lay in ("window", "narrow_a", "narrow_b"):
        assert np.array_equal(wide, run(case, lay, inp)), (route, lay)


@pytest.mark.parametrize("scale", [0.125, 0.0])
def test_mhsa_equals_attention_on_split_pointers(scale):
    """visrep_mhsa_fwd(qk) == visrep_attention_fwd(q = qk, k = qk + H 64, ldq = ldk = ldqk), and the routes it takes are the same."""
    route = "d64" if scale > 0 else "d64ps"
    case = AC.Case(route, 3, 77, 77, 2, seed=60)
    inp = AC.make_inputs(case)
    HD = case.H * 64
    packed = AC.pack(inp, case, "tight")
    qk = AC._window(np.concatenate([inp["q"].reshape(-1, HD), inp["k"].reshape(-1, HD)], 1), 2 * HD + 8, 0, 70)
    packed["bufs"]["q"] = (qk, 0)
    packed["dims"]["ldq"] = 2 * HD + 8
    a = launch(case, packed, scale, entry="mhsa")
    packed["bufs"]["k"] = (qk, HD)
    packed["dims"]["ldk"] = 2 * HD + 8
    assert np.array_equal(a, launch(case, packed, scale))
    assert np.array_equal(a, run(case, "tight", inp))


@pytest.mark.parametrize("M", [77, 130, 64])
def test_linear_vt_equals_the_host_packer(M):
    """engine.linear_vt with an identity weight writes, in the columns of the M keys, what pack_vt puts there (two independent statements of
    perm16), and leaves the columns of keys >= round_up(M, 4) zero."""
    rs = np.random.RandomState(M)
    v = AC.bf16_round(rs.standard_normal((M, 128)))
    vd = torch.from_numpy(AC.bf16_bits(v).view(np.int16)).view(torch.bfloat16).to(DEV)
    eye = torch.eye(128, dtype=torch.bfloat16, device=DEV)
    got = engine.linear_vt(vd, eye, None).view(torch.int16).cpu().numpy().view(np.uint16)
    want = AC.pack_vt(v, got.shape[1], hostile=False)
    cols = AC.perm16(np.arange(M))
    assert np.array_equal(got[:, cols], want[:, cols])
    rest = AC.perm16(np.arange((M + 3) // 4 * 4, got.shape[1]))
    assert (got[:, rest] & 0x7FFF == 0).all()


@pytest.mark.parametrize("Tk", [11, 77])
@pytest.mark.parametrize("route", AC.EDGE_ROUTES)
def test_shared_prompt_with_nan_rows_behind_it(route, Tk):
    """kv_shared = 1: the K buffer holds exactly Tk rows followed, in the same allocation, by NaN rows - the last key tile reaches past the
    last key row and re-reads it (clamped) instead."""
    held(AC.Case(route, 3, 100, Tk, 2, 1, 0, seed=70 + Tk), ("tight", "window"))


@pytest.mark.parametrize("name,entry,over,rc,msg", AC.REFUSALS, ids=[r[0] for r in AC.REFUSALS])
def test_refusals(name, entry, over, rc, msg):
    """Return code, message, nothing launched (route counters) and nothing written (the output keeps its pattern)."""
    lib = _lib.require_gpu()
    buf = torch.full((1 << 16,), -1, dtype=torch.int16, device=DEV)                    # every pointer: the same 128 KB, 0xFFFF = a NaN
    fn = {"attn": lib.visrep_attention_fwd, "cls": lib.visrep_mhsa_cls_fwd, "mhsa": lib.visrep_mhsa_fwd}[entry]
    args = AC.refusal_args(entry, over, buf.data_ptr())
    _lib.routes(reset=True)
    assert fn(*args, _lib.stream_ptr()) == rc, _lib.last_error()
    assert msg in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    assert not any(_lib.routes(reset=True).values())
    assert bool((buf == -1).all())


def test_non_finite_isolation():
    """include/visrep.h, attention block, as documented.  B = 4 images of 77 keys on global 64-key tiles: image 1's keys 0 .. 50 share tile 1
    with image 0's keys 64 .. 76, its keys 51 .. 76 share tile 2 with image 2's keys 0 .. 37.
    NaN in image 1's Q or K: every other image bitwise unchanged (masked scores are overwritten).
    NaN in one element of image 1's V (key 5, head 1, channel 7): images 2 and 3 bitwise unchanged; image 0, which shares the key tile, gets
    0 * NaN = NaN in that column and only there - the known difference from softmax(QK^T)V, recorded in DESIGN.md."""
    case = AC.Case("d64", 4, 70, 77, 2, seed=80)
    inp = AC.make_inputs(case)
    base = run(case, "tight", inp).reshape(4, 70, 128)
    nan = 0x7FC0

    def in_q(p):
        p["bufs"]["q"][0][70 + 3, 64 + 7] = nan

    def in_k(p):
        p["bufs"]["k"][0][77 + 5, 64 + 7] = nan

    def in_v(p):
        p["bufs"]["vt"][0][64 + 7, AC.perm16(77 + 5)] = nan

    for edit in (in_q, in_k):
        got = run(case, "tight", inp, edit=edit, finite=False).reshape(4, 70, 128)
        assert not AC.finite_bits(got[1]).all()
        for b in (0, 2, 3):
            assert np.array_equal(got[b], base[b]), (edit.__name__, b)
    got = run(case, "tight", inp, edit=in_v, finite=False).reshape(4, 70, 128)
    for b in (2, 3):
        assert np.array_equal(got[b], base[b]), b
    col = np.zeros(128, dtype=bool)
    col[64 + 7] = True
    assert not AC.finite_bits(got[1][:, col]).any()
    assert np.array_equal(got[0][:, ~col], base[0][:, ~col])
    assert not AC.finite_bits(got[0][:, col]).any()                                    # the leak, as documented


def test_zz_report():
    for route, (r, cid, lay) in sorted(WORST.items()):
        print(f"[attn-contract] worst {route}: {r:.3f} ({cid}, {lay})")
    assert all(r <= 1.0 for r, _, _ in WORST.values())
