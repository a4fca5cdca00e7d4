"""CPU proofs of the convolution contract pieces (tests/_conv_cases.py): the oracle against F.conv2d in float64, the index-exact builder's
conditions, the windows and the isolation buffers, the dispatcher's plan for every table case, the SiLU formula inside its allowance, a CPU fp32
emulation of the convolution inside the arithmetic bound (worst err / bound per route printed), and the mutations: the same emulation with one
defect each must be rejected by the per-element check, and by the exact check where it applies."""
import math
import os
import sys
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _conv_cases as CC  # noqa: E402
import _gemm_cases as GC  # noqa: E402


def ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------------------------------------ oracle
@pytest.mark.parametrize("geom", CC.GEOMS + ((1, 1, 0), (2, 0, 1)), ids=lambda g: "s%dp%du%d" % g)
@pytest.mark.parametrize("shape", [(2, 5, 7, 8, 16), (1, 13, 10, 16, 8), (1, 6, 6, 8, 8), (2, 16, 16, 8, 8)], ids=lambda s: "x".join(map(str, s)))
def test_oracle_agrees_with_conv2d(shape, geom):
    """Nine shifted slices == F.conv2d in float64 (NCHW, explicit F.pad / F.interpolate) at every (stride, pad_mode, up); Ho / Wo at odd and even sizes."""
    B, H, W, C, Co = shape
    s, p, u = geom
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    w = torch.randn(Co, 3, 3, C, generator=g, dtype=torch.float64)
    xn = x.permute(0, 3, 1, 2)
    if u:
        xn = F.interpolate(xn, scale_factor=2, mode="nearest")
    want = F.conv2d(F.pad(xn, (0, 1, 0, 1)), w.permute(0, 3, 1, 2), stride=s) if p else F.conv2d(xn, w.permute(0, 3, 1, 2), stride=s, padding=1)
    Ho, Wo = CC.out_hw(H, W, s, p, u)
    assert want.shape == (B, Co, Ho, Wo)
    got = CC.conv64(x, w, s, p, u).view(B, Ho, Wo, Co).permute(0, 3, 1, 2)
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()
    # the gather oracle is the same slices without the product: it rebuilds the convolution exactly
    cols = CC.im2col_index_oracle(x, s, p, u, 9 * C + 8)
    assert (cols[:, 9 * C:] == 0).all()
    assert (cols[:, :9 * C] @ w.reshape(Co, -1).t() - CC.conv64(x, w, s, p, u)).abs().max() <= 1e-12 * want.abs().max()


def test_out_hw_formulas():
    assert CC.out_hw(5, 7, 1, 0, 0) == (5, 7) and CC.out_hw(5, 7, 2, 0, 0) == (3, 4) and CC.out_hw(5, 7, 2, 1, 0) == (2, 3) and CC.out_hw(5, 7, 1, 0, 1) == (10, 14)
    assert CC.out_hw(13, 10, 2, 0, 0) == (7, 5) and CC.out_hw(13, 10, 2, 1, 0) == (6, 5) and CC.out_hw(257, 257, 2, 1, 0) == (128, 128)


def test_bf16_round64_is_round_to_nearest_even():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(200000, generator=g, dtype=torch.float64) * torch.exp2(torch.randint(-20, 20, (200000,), generator=g).double())
    assert torch.equal(CC.bf16_round64(v.float().double()), v.float().to(torch.bfloat16).double())       # fp32-representable: torch's own rounding
    ties = torch.tensor([1.00390625, 1.01171875, -3.0234375, 0.0, 256.0, 257.0, 259.0])                # 1 + 2^-8 (down to even), 1 + 3 * 2^-8 (up), ...
    assert CC.bf16_round64(ties.double()).tolist() == [1.0, 1.015625, -3.03125, 0.0, 256.0, 256.0, 260.0]
    assert CC.ulp_bf16(torch.tensor([1.0, 1.9, 2.0, 0.75], dtype=torch.float64)).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8]


def test_silu_formula_is_inside_its_allowance():
    """conv3x3_halo's o * rcp(1 + exp2(o * -log2 e)) in fp32 on a dense grid against float64 (torch's fp32 exp2 / reciprocal are within 1 ulp, as
    v_exp_f32 / v_rcp_f32)."""
    x = torch.cat([torch.linspace(-100.0, 100.0, 2000001), torch.linspace(-1.0, 1.0, 200001), torch.tensor([0.0, -126.0, 88.0, -88.0])]).float()
    want = x.double() * torch.sigmoid(x.double())
    err = (CC.silu_device_formula_fp32(x).double() - want).abs()
    allow = CC.silu_allowance(x.double())
    worst = (err / allow).max().item()
    print(f"[conv-cases] SiLU device formula: worst err / allowance {worst:.3f}")
    assert (err <= allow).all() and worst > 0.01
    d = torch.linspace(-20.0, 20.0, 400001, dtype=torch.float64)                                       # Lipschitz constant of t sigmoid(t)
    s = torch.sigmoid(d)
    assert (s * (1 + d * (1 - s))).abs().max() < 1.1


# ------------------------------------------------------------------------------------------------ exact builder
def exact_want(case):
    d, gn, _ = CC.inputs_for(case, "exact")
    s, p, u = case.geom
    X = d["x"].double()
    if gn is not None:
        X, flip = CC.gn_operand64(X, gn)
        assert (flip == 0).all()                                # integers: nowhere near a tie
    want = CC.conv64(X, d["w"].double(), s, p, u) + d["bias"].double()
    if case.kind == "resid":
        want = want + d["resid"].double()
    return d, X, want


SMALL = [c for c in CC.ALL_CASES if c.M * c.Cout * 9 * c.C <= 8e9 and (c.route == "halo" or c.M <= 4096)]


@pytest.mark.parametrize("case", SMALL, ids=ids(SMALL))
def test_exact_inputs_stay_exact(case):
    """Integers, one nonzero channel per pixel, every output an integer of magnitude <= 254, float64 == int64 arithmetic; the reference's bound
    machinery agrees (want identical)."""
    d, X, want = exact_want(case)
    x = d["x"]
    assert ((x != 0).sum(dim=3) == 1).all() and set(x.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    w = d["w"]
    assert w.abs().max() <= 7 and torch.equal(w, w.round())
    t9 = w.reshape(case.Cout, 9, case.C)
    assert all((t9[:, i] != t9[:, j]).all() for i in range(9) for j in range(i))                       # no two taps agree, hence no ky / kx transpose
    assert d["bias"].abs().max() <= 64 and d["resid"].abs().max() <= 64 and torch.equal(d["resid"], d["resid"].round())
    assert torch.equal(X, X.round()) and torch.equal(want, want.round()) and want.abs().max() <= 254, want.abs().max()
    s, p, u = case.geom
    if case.M * case.Cout * 9 * case.C <= 3e8:                   # int64 products have no BLAS: the small cases
        cols = CC.im2col_index_oracle(X.to(torch.int64), s, p, u, 9 * case.C)
        w64 = w.to(torch.int64).reshape(case.Cout, -1)
        i64 = cols @ w64.t() + d["bias"].to(torch.int64) + (d["resid"].to(torch.int64) if case.kind == "resid" else 0)
        assert torch.equal(want.to(torch.int64), i64)
    if case.gn:
        tab = d["table"]
        assert (tab[..., 1] != 0).all() and torch.equal(tab[..., 1], tab[..., 1].round())
        assert set(tab[..., 0].unique().tolist()) <= {1.0, -1.0, 2.0, -2.0, 0.5}
        # a kernel that normalises the zero padding adds sum_c shift[c] w[co, tap, c] = w[co, tap, 0] for every padded tap: nonzero somewhere on every border
        leak = (tab[0, :, 1][None, None, :] * t9).sum(2)
        assert torch.equal(leak, t9[:, :, 0]) and (leak != 0).any(0).all()
    if case.route == "c8":
        assert (x[..., 3:] == 0).all() and (w[..., 3:] != 0).any()


def test_exact_magnitude_limit_holds_by_construction():
    """Without the fused norm the limit needs no computation: 9 taps x |x| <= 2 x |w| <= 7 = 126, + 64 + 64."""
    assert 9 * 2 * 7 + 64 + 64 == 254
    for case in CC.ALL_CASES:
        assert case.gn is None or case in SMALL, case.id          # every fused-norm case is computed by test_exact_inputs_stay_exact


def test_exact_inputs_reach_every_halo_slot_and_border():
    """Every (halo x-position 0 .. 17, 16-byte channel chunk 0 .. 15) pair receives a nonzero somewhere in the table's halo shapes, and every tap is
    exercised at every border and corner: in-image taps multiply a nonzero pixel with a nonzero weight, out-of-image taps would (the pixel a
    clamping or wrapping gather reads there has a nonzero weight under it)."""
    seen = torch.zeros(18, 16, dtype=torch.bool)
    for B, H, W in {(c.B, c.H, c.W) for c in CC.CASES_HALO}:
        ch = CC.exact_channel(B, H, W, 128)
        xs = torch.arange(W)[None, None, :].expand(B, H, W)
        for hx_of, ok in ((xs % 16 + 1, torch.ones_like(xs, dtype=torch.bool)), (torch.zeros_like(xs), (xs % 16 == 15) & (xs + 1 < W)),
                          (torch.full_like(xs, 17), (xs % 16 == 0) & (xs > 0))):
            seen[hx_of[ok], (ch >> 3)[ok]] = True
    assert seen.all(), (~seen).nonzero().tolist()
    for case in (CC.CASES_HALO[0], CC.CASES_128[0], CC.CASES_C8[0]):
        d, _, _ = CC.inputs_for(case, "exact")
        x, w = d["x"], d["w"]
        B, H, W, C = x.shape
        ch = CC.exact_channel(B, H, W, C, 3 if case.route == "c8" else None)
        classes = {"top": (0, range(1, W - 1)), "bottom": (H - 1, range(1, W - 1)), "left": (range(1, H - 1), 0), "right": (range(1, H - 1), W - 1),
                   "tl": (0, 0), "tr": (0, W - 1), "bl": (H - 1, 0), "br": (H - 1, W - 1)}
        for name, (ys, xs_) in classes.items():
            ys = [ys] if isinstance(ys, int) else list(ys)
            xs_ = [xs_] if isinstance(xs_, int) else list(xs_)
            for ky in range(3):
                for kx in range(3):
                    hit = False
                    for y in ys:
                        for xx in xs_:
                            cy, cx = min(max(y + ky - 1, 0), H - 1), min(max(xx + kx - 1, 0), W - 1)
                            hit = hit or bool((w[:, ky, kx, ch[0, cy, cx]] != 0).any())
                    assert hit, (case.id, name, ky, kx)


# ------------------------------------------------------------------------------------------------ windows, isolation, table
def test_windows_and_isolation():
    for case in CC.ALL_CASES:
        ldc, col0 = CC.window_of(case)
        dtype = torch.float32 if case.kind == "f32" else torch.bfloat16
        assert (case.win == "f4") <= (case.kind == "f32") and (case.kind == "f32") <= (case.win in ("f4", "c"))
        off = GC.c_offset_bytes(case.M, case.Cout, ldc, col0, dtype)
        if case.route == "halo":
            assert ldc % 8 == 0 and off % 16 == 0, case.id      # the halo entry refuses anything else (refusals are tested on the GPU)
        if case.route == "c8":
            assert ldc % 8 == 0 and off % 8 == 0, case.id
        assert ldc % 4 == 0 and off % (16 if case.kind == "f32" else 8) == 0, case.id
    buf, view = CC.make_window(70, 64, 80, 8, torch.bfloat16)
    assert CC.stray_writes(buf, 70, 64, 8) == 0
    view.fill_(1.0)
    assert CC.stray_writes(buf, 70, 64, 8) == 0 and not torch.isnan(view.float()).any()
    buf[0, 3] = 0.0
    buf[71, 79] = float("nan")                                  # a NaN that is not the sentinel's bit pattern counts too
    assert CC.stray_writes(buf, 70, 64, 8) == 2
    tok = torch.ones(2 * 5 * 7, 64, dtype=torch.bfloat16)
    ibuf, iview = CC.isolate(tok, (7 + 2) * 64)
    g = CC.round_up(9 * 64, 64)
    assert ibuf.numel() == 2 * g + tok.numel() and iview.data_ptr() % 128 == ibuf.data_ptr() % 128 and torch.equal(iview, tok)
    assert torch.isnan(ibuf[:g].float()).all() and torch.isnan(ibuf[-g:].float()).all()
    w = CC.pack_weights(torch.ones(128, 3, 3, 8), 104, zero_to=96)
    assert (w[:, :72] == 1).all() and (w[:, 72:96] == 0).all() and torch.isnan(w[:, 96:].float()).all()
    w = CC.pack_weights(torch.ones(64, 3, 3, 64), 9 * 64 + 8)
    assert torch.isnan(w[:, 576:].float()).all() and not torch.isnan(w[:, :576].float()).any()


def test_case_table_covers_what_it_claims():
    ids_ = [c.id for c in CC.ALL_CASES]
    assert len(set(ids_)) == len(ids_)
    c128 = CC.CASES_128
    assert {(c.B, c.H, c.W, c.Cout) for c in c128} == set(CC.SHAPES_128) and {c.M for c in c128 if c.geom == (1, 0, 0)} == {70, 243, 130}
    assert {(c.kind, c.variant) for c in c128} == {(k, v) for k in CC.KIND_OF_EPI for v in (1, 5)}
    assert {((c.B, c.H, c.W), c.geom) for c in c128} == {(s[:3], g) for s in CC.SHAPES_128 for g in CC.GEOMS}
    assert {c.win for c in c128} == {"c", "al", "a8", "l4", "f4"}
    sk = CC.CASES_SPLITK
    assert {c.C for c in sk} == {128, 256} and {c.kind for c in sk} == set(CC.KIND_OF_EPI) and {c.geom for c in sk} == {(1, 0, 0), (2, 1, 0)}
    assert {(c.B, c.H, c.W) for c in sk} == {(2, 6, 6), (1, 12, 20)}
    for sh in CC.SHAPES_128:                                    # each shape meets each epilogue
        assert {c.kind for c in c128 if (c.B, c.H, c.W, c.Cout) == sh} == set(CC.KIND_OF_EPI), sh
    halo = CC.CASES_HALO                                        # the full cross, nothing rotated
    cross = {(sh, k, tab, kind) for sh in CC.SHAPES_HALO + ((3, 80, 80),) for k in CC.HALO_KERNELS for tab in CC.HALO_TABLES for kind in ("bias", "resid")}
    assert len(halo) == len(cross) == 90 and {((c.B, c.H, c.W), (c.Cout, c.tile), (c.gn, c.silu), c.kind) for c in halo} == cross
    assert all(c.groups == 32 for c in halo) and {c.win for c in halo} == {"al", "c"} and all((c.cus == 64) == (c.H == 80) for c in halo)
    keys = [CC.data_key(c) for c in CC.ALL_CASES]               # cases that share operands are neighbours (one float64 accumulation on the GPU)
    assert all(keys.index(k) + keys.count(k) - 1 == len(keys) - 1 - keys[::-1].index(k) for k in set(keys))
    assert len({CC.seed_of(c) for c in CC.ALL_CASES}) == len(set(keys))
    assert {(c.B, c.H, c.W) for c in CC.CASES_C8} == {(1, 4, 16), (2, 8, 16), (3, 4, 32), (1, 16, 48)} and {bool(c.groups) for c in CC.CASES_C8} == {True, False}
    assert len(CC.IM2COL_CASES) == 32


@pytest.mark.parametrize("case", CC.ALL_CASES, ids=ids(CC.ALL_CASES))
def test_route_plan(case):
    """The dispatcher's rule restated (csrc/gemm_bf16.hip) gives every case the route it names at the CU count it runs at."""
    cus = case.cus or 256
    assert CC.route_plan(case, cus, gn_entry=case.route == "128gn") == CC.expected_routes(case), case.id
    if case.route == "128gn":                                   # the plain call it is compared with runs the same kernel without the sums
        assert CC.route_plan(case, cus) == CC.expected_routes(CC.Case("128", *[getattr(case, f) for f in ("B", "H", "W", "C", "Cout")])), case.id
    if case.route == "splitk":
        S = CC.split_k_slices(case.M, case.Cout, 9 * case.C, cus)
        assert 2 <= S <= 9 and S - 1 <= 8 and 9 * case.C <= 2304, (case.id, S)      # the K + 8 factor counts the reduction's additions
    if case.route == "halo":
        assert case.C == 128 and case.H % 16 == 0 and case.W % 16 == 0 and (case.tile == 16 or case.Cout == 128)
        if case.cus:
            tiles = case.B * (case.H // case.tile) * (case.W // 16)
            assert tiles > case.cus * (1 if case.tile == 16 else 2), case.id      # a workgroup walks more than one tile
    if case.route == "c8":
        assert case.W % 16 == 0 and (case.H * case.W) % (128 if case.groups else 64) == 0


def test_route_plan_of_the_64_cu_shapes():
    c = {x.id: x for x in CC.CASES_256}
    whole = CC.Case("256", 2, 128, 128, 64, 256, cus=64)
    assert whole.M == 32768 and CC.route_plan(whole, 64)["conv_256"] == 1 and CC.route_plan(whole, 256) == CC.expected_routes(CC.Case("128", 2, 128, 128, 64, 256))
    rag = CC.Case("256tail", 1, 182, 182, 64, 256, "resid", cus=64)
    assert rag.M == 33124 and rag.M % 256 == 100 and -(-rag.M // 256) == 130
    assert CC.route_plan(rag, 64) == CC.expected_routes(rag) and CC.route_plan(rag, 256)["conv_128"] == 1
    odd = CC.Case("256", 2, 257, 257, 64, 256, geom=(2, 1, 0), cus=64)
    assert odd.M == 32768 and CC.route_plan(odd, 64)["conv_256"] == 1
    assert CC.route_plan(CC.Case("256", 2, 128, 128, 64, 256, "f32", cus=64), 64)["conv_128"] == 1      # the 256 x 256 kernel has no F32 convolution
    assert len(c) == len(CC.CASES_256)


# ------------------------------------------------------------------------------------------------ CPU fp32 emulation and its mutations
def gather_index(case, mutation=None):
    """(b, iy, ix, valid) index tensors [M, 9] of the gather, written from the definition with explicit index arithmetic (so that a defect can be put in)."""
    s, p, u = case.geom
    H, W = case.H, case.W
    Ho, Wo = CC.out_hw(H, W, s, p, u)
    pad = 1 if p == 0 else 0
    if mutation == "pad_symmetric" and p == 1:
        pad = 1
    m = torch.arange(case.B * Ho * Wo)
    b, pix = m // (Ho * Wo), m % (Ho * Wo)
    oy, ox = pix // Wo, pix % Wo
    t = torch.arange(9)
    ky, kx = t // 3, t % 3
    iy = oy[:, None] * s + ky[None, :] - pad
    ix = ox[:, None] * s + kx[None, :] - pad
    Hl, Wl = H << u, W << u
    valid = (iy >= 0) & (iy < Hl) & (ix >= 0) & (ix < Wl)
    if mutation == "clamp":
        iy, ix, valid = iy.clamp(0, Hl - 1), ix.clamp(0, Wl - 1), torch.ones_like(valid)
    if mutation == "wrap":                                      # only the row bound is tested: x = -1 reads the previous pixel row's last pixel
        flat = (iy * Wl + ix).clamp(0, Hl * Wl - 1)
        valid = (iy >= 0) & (iy < Hl)
        iy, ix = flat // Wl, flat % Wl
    if u:
        iy, ix = ((iy + 1) >> 1, (ix + 1) >> 1) if mutation == "up_ceil" else (iy >> 1, ix >> 1)
        iy, ix = iy.clamp(max=H - 1), ix.clamp(max=W - 1)
    iy, ix = iy.clamp(0, H - 1), ix.clamp(0, W - 1)
    return b[:, None].expand_as(iy), iy, ix, valid


def emulate(case, d, gn, mutation=None, lose=None):
    """fp32 emulation: operand (fused norm in fp32 as the device forms it), Python gather, float32 matmul, bias (+ residual) in fp32.  Returns the
    UNROUNDED fp32 result [M, Cout].  mutation: one defect (see the test below); lose = (row, tap): that output row loses that tap."""
    x = d["x"].float()
    pad_value = None
    if gn is not None:
        tab, silu = gn
        sc, sh = tab[..., 0][:, None, None, :], tab[..., 1][:, None, None, :]
        h = (x.double() * sc.double() + sh.double()).float()    # fma: one rounding
        hp = sh.expand(case.B, 1, 1, case.C).clone().float()
        if silu:
            h, hp = CC.silu_device_formula_fp32(h), CC.silu_device_formula_fp32(hp)
        x = h.to(torch.bfloat16).float()
        pad_value = hp.to(torch.bfloat16).float()               # what a padding pixel becomes if it is normalised (x = 0 -> shift)
    b, iy, ix, valid = gather_index(case, mutation)
    cols = x[b, iy, ix, :]                                      # [M, 9, C]
    if mutation == "pad_before_norm":
        cols = torch.where(valid[..., None], cols, pad_value[b[:, 0], 0, 0, :][:, None, :].expand_as(cols))
    else:
        cols = cols * valid[..., None]
    if lose is not None:
        cols[lose[0], lose[1]] = 0
    w = d["w"].float().reshape(case.Cout, 9, case.C)
    if mutation == "transpose":
        w = d["w"].float().transpose(1, 2).reshape(case.Cout, 9, case.C)
    if mutation == "chunk_swap":                                # one 16-byte weight chunk of one tap swapped with its swizzle neighbour (chunk ^ 1)
        w = w.clone()
        w[:, 4, 8:16], w[:, 4, 0:8] = w[:, 4, 0:8].clone(), w[:, 4, 8:16].clone()
    z = cols.reshape(cols.shape[0], -1) @ w.reshape(case.Cout, -1).t() + d["bias"].float()
    if case.kind == "resid":
        z = d["resid"].float() + z
    return z


def rounded(case, z):
    return z.double() if case.kind == "f32" else z.to(torch.bfloat16).double()


EMU = ([c for c in SMALL if c.route != "halo" and c.M <= 4096][::2] + [c for c in CC.CASES_HALO if c.B * c.H * c.W <= 512][::3] +
       [next(c for c in CC.CASES_256 if c.route == r) for r in ("256", "256tail")])


def test_fp32_emulation_stays_inside_the_arithmetic_bound():
    """Every route: the 256 x 256 kernel on its whole-rounds shape and its head-plus-tail shape too (the arithmetic is the 128 x 128 route's at 32768 rows)."""
    worst, widened, near = defaultdict(float), defaultdict(float), defaultdict(float)
    for case in dict.fromkeys(EMU):
        for mode in ("bound", "exact"):
            d, gn, _ = CC.inputs_for(case, mode)
            rep = {}
            want, bound = CC.reference_for(case, d, gn, report=rep)
            z = emulate(case, d, gn)
            if mode == "exact":
                assert torch.equal(rounded(case, z), want), case.id
                continue
            ab = CC.arithmetic_bound(case.kind, want, bound)
            r = ((z.double() - want).abs() / ab).max().item()
            key = case.route + (" +gn" if gn else "")
            worst[key] = max(worst[key], r)
            widened[key] = max(widened[key], rep.get("widened", 0.0))
            near[key] = max(near[key], rep.get("operands", 0.0))
            assert r <= 1.0, (case.id, r)
            assert ((rounded(case, z) - want).abs() <= bound).all(), case.id
    for k in sorted(worst):
        print(f"[conv-cases] fp32 emulation, route {k:10s}: worst err / arithmetic bound {worst[k]:.4f}; outputs touched by the tie widening {100 * widened[k]:.2f} % "
              f"({100 * near[k]:.4f} % of the operands lie near a tie)")
    assert set(worst) >= {"128", "128gn", "splitk", "256", "256tail", "c8", "halo", "halo +gn"}
    assert 0 < max(near.values()) < 0.005                       # the widening is an exception (an output sums 1152 operands), not a blanket


def _first(group, **kw):
    return next(c for c in group if all(getattr(c, k) == v for k, v in kw.items()))


MUTATIONS = [
    ("transpose", _first(CC.CASES_128, geom=(1, 0, 0))), ("transpose", _first(CC.CASES_HALO, gn="tab", silu=1)),
    ("clamp", _first(CC.CASES_128, geom=(1, 0, 0))), ("clamp", _first(CC.CASES_128, geom=(2, 1, 0), W=10)), ("clamp", _first(CC.CASES_C8)),
    ("clamp", _first(CC.CASES_HALO, gn="tab", silu=1)),
    ("wrap", _first(CC.CASES_128, geom=(1, 0, 0))), ("wrap", _first(CC.CASES_C8)), ("wrap", _first(CC.CASES_HALO, gn=None)),
    ("pad_before_norm", _first(CC.CASES_HALO, gn="tab", silu=1)), ("pad_before_norm", _first(CC.CASES_HALO, gn="tab", silu=0)),
    ("pad_symmetric", _first(CC.CASES_128, geom=(2, 1, 0))), ("pad_symmetric", _first(CC.CASES_SPLITK, geom=(2, 1, 0))),
    ("up_ceil", _first(CC.CASES_128, geom=(1, 0, 1))),
    ("chunk_swap", _first(CC.CASES_128, geom=(1, 0, 0))), ("chunk_swap", _first(CC.CASES_HALO, gn="tab", silu=1)), ("chunk_swap", _first(CC.CASES_HALO, gn=None)),
]


@pytest.mark.parametrize("mutation,case", MUTATIONS, ids=[f"{m}-{c.id}" for m, c in MUTATIONS])
def test_mutations_are_rejected(mutation, case):
    """One defect each; the per-element check must reject it in bound mode (the SiLU tie widening included) and the exact check in exact mode."""
    for mode in ("bound", "exact"):
        d, gn, _ = CC.inputs_for(case, mode)
        want, bound = CC.reference_for(case, d, gn)
        good, bad = rounded(case, emulate(case, d, gn)), rounded(case, emulate(case, d, gn, mutation))
        assert ((good - want).abs() <= bound).all()
        n_bad = int(((bad - want).abs() > bound).sum())
        l2 = ((bad - want).norm() / want.norm()).item()
        print(f"[conv-cases] mutation {mutation:16s} {case.id} [{mode}]: {n_bad} elements outside the bound, exact equal: {torch.equal(bad, want)}, rel L2 {l2:.2e}")
        if mode == "bound":
            assert n_bad > 0, (mutation, case.id)
        else:
            assert torch.equal(good, want) and not torch.equal(bad, want), (mutation, case.id)


def test_one_lost_corner_tap_passes_the_old_bar_and_fails_this_one():
    """The documented reason for this suite: one corner pixel of one image of a 4 x 128 x 128, 64 -> 128 convolution loses one tap.  The relative L2
    norm stays below the 5e-3 the older tests ask for; the per-element bound and the exact check both reject it."""
    case = CC.Case("128", 4, 128, 128, 64, 128)
    row = 2 * 128 * 128 + 127 * 128 + 127                       # image 2, bottom right corner
    for mode in ("bound", "exact"):
        build = CC.exact_inputs if mode == "exact" else CC.random_inputs
        d = build(4, 128, 128, 64, 128, 77)
        want, bound = CC.conv_reference("bias", d["x"], d["w"], d["bias"])
        good, bad = rounded(case, emulate(case, d, None)), rounded(case, emulate(case, d, None, lose=(row, 0)))
        l2_good, l2 = ((good - want).norm() / want.norm()).item(), ((bad - want).norm() / want.norm()).item()
        out = (bad - want).abs() > bound
        print(f"[conv-cases] lost corner tap [{mode}]: rel L2 {l2:.3e} (intact: {l2_good:.3e}), {int(out.sum())} elements outside the bound, all in row {row}")
        assert ((good - want).abs() <= bound).all()
        assert l2 < 5e-3 and out.any() and out.nonzero()[:, 0].unique().tolist() == [row]
        if mode == "exact":
            assert torch.equal(good, want) and not torch.equal(bad, want)
