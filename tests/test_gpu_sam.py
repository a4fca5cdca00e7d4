"""SAM ViT towers on the GPU: the relative-position attention kernel through the C ABI against the float64 oracle at the derived bound
(tests/_sam_cases.py), exact index cases, structure, refusals; the table kernel against float64 and its host twin; the window gather / scatter;
the composed tower against transformers.SamVisionModel under the project's rule e_hip <= 2 e_ref; routes; the tower plug-in."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _attention_cases as AC  # noqa: E402
import _sam_cases as SC  # noqa: E402

from law_of_vision_representation_in_mllms_amd import _lib, engine, sam_weights as SW  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
cid = lambda c: c.id


def launch(case, packed, scale=0.125, S=None, head_dim=64, expect=0):
    lib = _lib.require_gpu()
    t = {n: torch.from_numpy(packed[n][0].view(np.int16).copy()).to(DEV) for n in ("qk", "vt", "out")}
    rh, rw = torch.from_numpy(packed["rel_h"]).to(DEV), torch.from_numpy(packed["rel_w"]).to(DEV)
    p = lambda n: C.c_void_p(t[n].data_ptr() + 2 * packed[n][1])
    torch.cuda.synchronize()
    _lib.routes(reset=True)
    rc = lib.visrep_mhsa_relpos_fwd(p("qk"), packed["ldqk"], p("vt"), packed["ldvt"], _lib.ptr(rh), _lib.ptr(rw), p("out"), packed["ldo"], case.NB,
                                    case.S if S is None else S, case.H, head_dim, scale, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (case.id, rc, _lib.last_error())
    plain = {k: v for k, v in _lib.routes().items() if v}
    sam = {k: v for k, v in _lib.sam_routes(reset=True).items() if v}
    assert plain == {} and sam == ({"attn_relpos": 1} if expect == 0 else {}), (plain, sam)
    bits = SC.out_window(t["out"].cpu().numpy().view(np.uint16), packed)
    if expect == 0:
        assert AC.finite_bits(bits).all(), case.id
    return bits


def run(case, inp=None, window=False):
    inp = SC.make_inputs(case) if inp is None else inp
    bits = launch(case, SC.pack(inp, case, window))
    return bits, AC.bf16_from_bits(bits).reshape(case.NB, case.T, case.H, 64)


def held(case, window=False):
    inp = SC.make_inputs(case)
    O, A, L = SC.oracle(inp, case)
    Lc = SC.components(inp, case)[1]
    assert Lc <= 2.0 * L, (case.id, L, Lc)                     # the precondition of the bound's constant, on the inputs that run
    bits, got = run(case, inp, window)
    r = SC.ratio(got, O, A, L)
    print(f"[sam-contract] {case.id}{' window' if window else ''}: ratio {r:.3f} (L = {L:.1f})")
    assert r <= 1.0, (case.id, r)
    return bits


@pytest.mark.parametrize("case", SC.GRID, ids=cid)
def test_grid(case):
    """S x NB x H: key tails of 4 (S = 2, 14), 17 (9) and 16 (20) keys, NB = 50 grids sharing global key tiles at every start residue."""
    held(case)


@pytest.mark.parametrize("case", [SC.Case(14, 3, 3, seed=40), SC.Case(9, 50, 1, seed=41), SC.Case(2, 3, 1, seed=42)], ids=cid)
def test_windows_inside_nan_filled_buffers(case):
    """Leading dimensions wider than the heads: Q | K as a window of a NaN-filled buffer with NaN rows behind it, V^T pad columns +-3.4e38,
    the output a window of a NaN-patterned buffer that stays untouched outside (asserted by out_window)."""
    held(case, window=True)


def test_global_shape():
    """S = 64: 4096 keys, every 64-key tile one grid row."""
    held(SC.GLOBAL)


@pytest.mark.parametrize("case", SC.BIAS30 + SC.GROWTH, ids=cid)
def test_bias_dominates_and_growth(case):
    """|bias| up to 30 over |scale q.k| ~ 1; staircases of 7.5 / 8.5 exp2 units per tile around the move threshold of 8; every logit at +-3000."""
    held(case)


@pytest.mark.parametrize("S", [9, 14])
@pytest.mark.parametrize("mode", ["h", "w", "hw"])
def test_index_exact(S, mode):
    """K = 0 and +-60 one-hot tables: every query's output is its predicted key's V row, bit for bit (swapped h / w, a transposed
    qh - kh or an off-by-one at the tile tail would pick another row)."""
    inp, want = SC.index_case(S, mode)
    case = SC.Case(S, 1, 1)
    bits, _ = run(case, inp)
    assert np.array_equal(bits.reshape(case.T, 64), AC.bf16_bits(want)), (S, mode)


def test_structure_bitwise():
    """A grid inside a batch equals the grid alone where both meet the same tile boundaries (g T % 64 == 0); permuting heads permutes blocks."""
    case = SC.Case(14, 17, 2, seed=50)                        # grid 16 starts at key 3136 = 49 * 64
    inp = SC.make_inputs(case)
    bits, _ = run(case, inp)
    alone = {k: v[16:17] for k, v in inp.items()}
    b1, _ = run(case._replace(NB=1), alone)
    assert np.array_equal(bits.reshape(17, case.T, 128)[16], b1.reshape(case.T, 128))
    case8 = SC.Case(8, 5, 2, seed=51)                          # T = 64: every grid is one whole tile
    inp8 = SC.make_inputs(case8)
    bits8, _ = run(case8, inp8)
    for g in (0, 3):
        bg, _ = run(case8._replace(NB=1), {k: v[g:g + 1] for k, v in inp8.items()})
        assert np.array_equal(bits8.reshape(5, 64, 128)[g], bg.reshape(64, 128))
    sw = {k: (v[:, :, ::-1] if k in ("q", "k", "v") else v[:, ::-1]).copy() for k, v in inp.items()}
    bsw, _ = run(case, sw)
    assert np.array_equal(bsw.reshape(-1, 2, 64)[:, ::-1], bits.reshape(-1, 2, 64))


def test_refusals_before_any_launch():
    case = SC.Case(8, 1, 2)
    packed = SC.pack(SC.make_inputs(case), case)
    lib = _lib.require_gpu()
    for kw, code, text in (({"S": 1}, -2, "S must be 2 .. 64"), ({"S": 65}, -2, "S must be 2 .. 64"), ({"head_dim": 128}, -2, "head_dim 64"),
                           ({"scale": 0.0}, -1, "scale must be > 0")):
        bits = launch(case, packed, expect=code, **kw)
        assert text in _lib.last_error() and (bits == AC.NAN_BITS).all(), kw
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    base = buf.data_ptr()
    ok = [base, 256, base, 128, base, base, base, 128, 1, 8, 2, 64, 0.125]
    for i, off, text in ((0, None, "null"), (2, None, "null"), (4, None, "null"), (5, None, "null"), (6, None, "null"), (0, 8, "16-byte"), (2, 8, "16-byte"),
                         (6, 4, "8-byte"), (4, 2, "4-byte"), (5, 2, "4-byte")):
        a = list(ok)
        a[i] = None if off is None else base + off
        _lib.routes(reset=True)
        assert lib.visrep_mhsa_relpos_fwd(*a, _lib.stream_ptr()) == -1 and text in _lib.last_error(), (i, off, _lib.last_error())
        assert not any(_lib.sam_routes().values())
    a = list(ok); a[3] = 64 + 1
    assert lib.visrep_mhsa_relpos_fwd(*a, _lib.stream_ptr()) == -2
    torch.cuda.synchronize()
    assert not buf.any()


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("S", [9, 14, 64])
def test_tables_against_float64_and_twin(S):
    NB, H = (1, 1) if S == 64 else (3, 2)
    rs = np.random.RandomState(100 + S)
    ld = 2 * H * 64 + 24                                       # Q taken from a qk buffer with ldqk > 2 H 64; everything else NaN
    q = AC.bf16_round(rs.standard_normal((NB * S * S, H * 64)))
    buf = np.full((NB * S * S, ld), AC.NAN_BITS, dtype=np.uint16)
    buf[:, :H * 64] = AC.bf16_bits(q)
    qk = torch.from_numpy(buf.view(np.int16)).view(torch.bfloat16)
    Rh, Rw = (torch.from_numpy(rs.standard_normal((2 * S - 1, 64)).astype(np.float32)) for _ in range(2))
    _lib.routes(reset=True)
    gh, gw = engine.relpos_tables(qk.to(DEV), Rh.to(DEV), Rw.to(DEV), NB, S, H)
    torch.cuda.synchronize()
    assert {k: v for k, v in _lib.sam_routes(reset=True).items() if v} == {"relpos_tables": 1}
    th, tw = engine.relpos_tables(qk, Rh, Rw, NB, S, H)
    assert torch.equal(gh.cpu(), th) and torch.equal(gw.cpu(), tw), "the kernel and its host twin run the same fmaf chain"
    wh, ww, bh, bw = SC.tables_oracle(q, Rh.double().numpy(), Rw.double().numpy(), NB, S, H)
    rh, rw = np.abs(gh.cpu().double().numpy() - wh) / bh, np.abs(gw.cpu().double().numpy() - ww) / bw
    print(f"[sam-tables] S = {S}: {rh.max():.3f} / {rw.max():.3f} of the gamma_64 bound")
    assert rh.max() <= 1.0 and rw.max() <= 1.0


# ------------------------------------------------------------------------------------------------ partition
@pytest.mark.parametrize("g", [14, 20, 64])
def test_partition_exact(g):
    """window_partition of the zero-padded map on PROJECTED tokens: exact copies, pad rows = the raw bias, nothing else written."""
    lib = _lib.require_gpu()
    B, w, d = 2, 14, 128
    rs = np.random.RandomState(g)
    M = B * g * g
    src = SC.window_rows(B, g, w)
    Mw = len(src)
    qk = AC.bf16_round(rs.standard_normal((M, 2 * d)))
    v = AC.bf16_round(rs.standard_normal((M, d)))
    bias = rs.standard_normal(3 * d).astype(np.float32) * 4
    ldvt, ldvw = AC.round_up(M, 64) + 64, AC.round_up(Mw, 64) + 64
    t_qk = torch.from_numpy(AC.bf16_bits(qk).view(np.int16)).to(DEV)
    t_vt = torch.from_numpy(AC.pack_vt(v, ldvt).view(np.int16)).to(DEV)
    t_b = torch.from_numpy(bias).to(DEV)
    guard = 64
    o_qk = torch.full((guard + Mw * 2 * d + guard,), AC.NAN_BITS, dtype=torch.int16, device=DEV)
    o_vt = torch.full((d, ldvw), AC.NAN_BITS, dtype=torch.int16, device=DEV)
    _lib.routes(reset=True)
    rc = lib.visrep_sam_window_partition(_lib.ptr(t_qk), 2 * d, _lib.ptr(t_vt), ldvt, _lib.ptr(t_b), C.c_void_p(o_qk.data_ptr() + 2 * guard), 2 * d,
                                         _lib.ptr(o_vt), ldvw, B, g, w, d, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    assert {k: v for k, v in _lib.sam_routes(reset=True).items() if v} == {"sam_partition": 1}
    bb = AC.bf16_bits(AC.bf16_round(bias.astype(np.float64)))
    got = o_qk.cpu().numpy().view(np.uint16)
    assert (got[:guard] == AC.NAN_BITS).all() and (got[-guard:] == AC.NAN_BITS).all()
    want = np.where(src[:, None] >= 0, AC.bf16_bits(qk)[np.maximum(src, 0)], bb[None, :2 * d])
    assert np.array_equal(got[guard:-guard].reshape(Mw, 2 * d), want)
    gv = o_vt.cpu().numpy().view(np.uint16)
    wv = np.where(src[:, None] >= 0, AC.bf16_bits(v)[np.maximum(src, 0)], bb[None, 2 * d:])
    cols = AC.perm16(np.arange(Mw))
    assert np.array_equal(gv[:, cols].T, wv)
    rest = np.ones(ldvw, dtype=bool); rest[cols] = False
    assert (gv[:, rest] == AC.NAN_BITS).all() and (src < 0).sum() == {14: 0, 20: B * (784 - 400), 64: B * (4900 - 4096)}[g]
    # the inverse drops the pad rows
    win = torch.from_numpy(AC.bf16_bits(AC.bf16_round(rs.standard_normal((Mw, d)))).view(np.int16)).to(DEV)
    out = torch.full((M * d + guard,), AC.NAN_BITS, dtype=torch.int16, device=DEV)
    assert lib.visrep_sam_window_unpartition(_lib.ptr(win), d, _lib.ptr(out), d, B, g, w, d, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint16)
    rows = np.empty(M, dtype=np.int64); rows[src[src >= 0]] = np.nonzero(src >= 0)[0]
    assert np.array_equal(o[:M * d].reshape(M, d), win.cpu().numpy().view(np.uint16)[rows]) and (o[M * d:] == AC.NAN_BITS).all()


# ------------------------------------------------------------------------------------------------ towers
TOWERS = {
    "tiny-g20": (SC.tiny_spec(), 3),
    "tiny-g14": (SC.tiny_spec(image_size=112), 3),
    "samb-g20": (SW.SamSpec("samb-2l", 320, 16, 768, 2, 12, 3072, 14, (1,), 256), 2),
    "samb-g64": (SW.SamSpec("samb-2l", 1024, 16, 768, 2, 12, 3072, 14, (1,), 256), 1),
}


def engine_states(spec, w, px):
    eng = engine.make_sam_engine(spec, w, DEV)
    _lib.routes(reset=True)
    states = [eng.forward(px.to(DEV), k).float().cpu() for k in range(spec.n_states)]
    torch.cuda.synchronize()
    return states, _lib.routes(), _lib.sam_routes(reset=True)


@pytest.mark.parametrize("weights", ["synthetic", "hostile"])
@pytest.mark.parametrize("name", list(TOWERS))
def test_tower_parity(name, weights):
    """e_hip / e_ref <= 2 for every one of the L + 2 states (e_ref: the same HF module in bf16 against its own fp32 run)."""
    spec, B = TOWERS[name]
    w = (SW.synthetic_weights if weights == "synthetic" else SW.hostile_weights)(spec, seed=1)
    px = SC.pixels_for(spec, B, seed=3)
    ref, e_ref = SC.tower_reference(spec, w, px, (name, weights))
    got, plain, sam = engine_states(spec, w, px)
    e_hip = [SC.rel_err(a, b) for a, b in zip(got, ref)]
    print(f"[sam-tower] {name} {weights}: e_hip / e_ref = {['%.2f' % (a / b) for a, b in zip(e_hip, e_ref)]}  e_ref = {['%.1e' % v for v in e_ref]}")
    for k, (a, b) in enumerate(zip(e_hip, e_ref)):
        assert a <= 2 * b, (name, weights, k, a, b)
    # routes: over the L + 2 forwards, state k runs min(k, L) layers - relpos attention in every one, the partition in windowed layers only
    L = spec.layers
    runs = [min(k, L) for k in range(spec.n_states)]
    n_attn = sum(runs)
    n_win = sum(sum(1 for l in range(r) if l not in spec.global_attn_indexes) for r in runs)
    assert sam["attn_relpos"] == n_attn and sam["relpos_tables"] == n_attn and sam["sam_partition"] == 2 * n_win and sam["sam_neck"] == 1, sam
    assert not any(plain[k] for k in ("attn", "attn_cls", "attn_prefix", "attn_96", "attn_wide")), plain


@pytest.mark.parametrize("name,B,budget", [("tiny-g20", 5, 2), ("samb-g20", 3, 1)], ids=["tiny-B5-by2", "samb-B3-by1"])
def test_chunked_equals_unchunked(name, B, budget):
    """visrep_sam_forward with a table budget of `budget` images per chunk (windowed and global layers, a last partial chunk) equals the
    unchunked run bit for bit, in the last block's state and in the neck map."""
    spec, _ = TOWERS[name]
    w = SW.hostile_weights(spec, seed=2)
    px = SC.pixels_for(spec, B, seed=5).to(DEV)
    eng = engine.make_sam_engine(spec, w, DEV)
    lib = _lib.require_gpu()
    whole = [eng.forward(px, k).clone() for k in (spec.layers, spec.layers + 1)]
    _lib.routes(reset=True)
    eng.forward(px, spec.layers)
    calls_whole = _lib.sam_routes(reset=True)["attn_relpos"]
    # the larger of the two per-image table sizes (windowed: grids * H * T * S * 4; global: H * T * S * 4), times the images per chunk
    nw = -(-spec.grid // spec.window)
    per_image = max(nw * nw * spec.heads * spec.window ** 3 * 4, spec.heads * spec.grid ** 3 * 4)
    old = lib.visrep_debug_sam_table_bytes(budget * per_image)
    try:
        parts = [eng.forward(px, k).clone() for k in (spec.layers, spec.layers + 1)]
        _lib.routes(reset=True)
        eng.forward(px, spec.layers)
        calls_parts = _lib.sam_routes(reset=True)["attn_relpos"]
    finally:
        lib.visrep_debug_sam_table_bytes(old)
    torch.cuda.synchronize()
    assert calls_whole == spec.layers and calls_parts >= spec.layers * -(-B // budget), (calls_whole, calls_parts)
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)


def test_dropped_bias_would_be_seen():
    """A-B proof: the tiny tower with rel_pos_* zeroed differs from the oracle by much more than 2 e_ref in every state behind layer 0."""
    spec, B = TOWERS["tiny-g20"]
    w = SW.synthetic_weights(spec, seed=1)
    px = SC.pixels_for(spec, B, seed=3)
    ref, e_ref = SC.tower_reference(spec, w, px, ("tiny-g20", "synthetic"))
    got, _, _ = engine_states(spec, SC.zero_rel(w), px)
    e = [SC.rel_err(a, b) for a, b in zip(got, ref)]
    print(f"[sam-tower] rel_pos zeroed: e / e_ref = {['%.1f' % (a / b) for a, b in zip(e, e_ref)]}")
    assert all(a > 10 * b for a, b in zip(e[1:], e_ref[1:]))


def test_plugin():
    from law_of_vision_representation_in_mllms_amd.llava.model.multimodal_encoder import builder
    args = dict(mm_vision_tower="facebook/sam-vit-base", synthetic_weights=True, device=DEV, mm_vision_select_feature="patch")
    t = builder.build_sam_vision_tower(SimpleNamespace(**args, mm_vision_select_layer=-1))
    px = torch.randn(1, 3, 1024, 1024)
    f = t(px.to(DEV))
    assert tuple(f.shape) == (1, 4096, 256) == (1, t.num_patches, t.hidden_size) and torch.isfinite(f.float()).all()
    t2 = builder.build_sam_vision_tower(SimpleNamespace(**args, mm_vision_select_layer=-2))
    f2 = t2(px.to(DEV))
    assert tuple(f2.shape) == (1, 4096, 768) == (1, t2.num_patches, t2.hidden_size) and torch.isfinite(f2.float()).all()
    assert torch.equal(f2, t2.vision_tower.engine.forward(px.to(DEV), 12).to(f2.dtype)), "-2 is the last block's output"
    with pytest.raises(ValueError, match="Unexpected select feature"):
        builder.build_sam_vision_tower(SimpleNamespace(**dict(args, mm_vision_select_feature="cls_patch"), mm_vision_select_layer=-1))
    with pytest.raises(ValueError, match="vit_img_size"):
        builder.build_sam_vision_tower(SimpleNamespace(**args, mm_vision_select_layer=-1, vit_img_size=512))
