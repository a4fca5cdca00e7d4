"""InternViT on the GPU: the RMS row kernels (rms_rows, rms_stats_rows) and the QK-norm pass (qk_rmsnorm_rows) through ctypes against float64
and the bounds derived in tests/_internvit_cases.py, RMS statistics out of the residual GEMMs on each of their routes, tower parity on all
engines against the real transformers module, the pre-scaled-Q constant's place, full-width routes, the plug-in tower and the unchanged
launches of towers that leave the new config fields zero.  `[internvit]` lines (pytest -s) print every figure before it is asserted."""
import ctypes as C
import math
import os
import sys
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _internvit_cases as IC  # noqa: E402

from law_of_vision_representation_in_mllms_amd import _lib, engine  # noqa: E402
from law_of_vision_representation_in_mllms_amd import vit_weights as VW  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bf = lambda t: t.to(torch.bfloat16).float()
SENTINEL = 0x5A5B                                                # a finite bf16 pattern (about 1.5e13) no kernel here produces


def dev_bits(a):
    return torch.from_numpy(IC.bf16_bits(a)).to(DEV)


def routed(fn):
    torch.cuda.synchronize()
    _lib.routes(reset=True)
    rc = fn()
    torch.cuda.synchronize()
    r = _lib.routes(reset=True)
    assert rc == 0, _lib.last_error()
    return {k: v for k, v in r.items() if v}


# ------------------------------------------------------------------------------------------------ 1. RMS row kernels
@pytest.mark.parametrize("rows", IC.RMS_ROWS)
@pytest.mark.parametrize("d", IC.RMS_DS)
def test_rmsnorm_and_stats_against_float64(d, rows):
    lib = _lib.require_gpu()
    x, g = IC.rms_rows_input(rows, d, seed=d + rows)
    rstd, y = IC.rms_oracle(x, g)
    ldx, ldy = d + 24, d + 8
    xb = torch.full((rows, ldx), SENTINEL, dtype=torch.int16, device=DEV)
    xb[:, :d] = dev_bits(x)
    yb = torch.full((rows, ldy), SENTINEL, dtype=torch.int16, device=DEV)
    gt = torch.from_numpy(g).to(DEV)
    rt = torch.full((rows + 2, 2), float("nan"), device=DEV)
    r = routed(lambda: lib.visrep_rmsnorm(_lib.ptr(xb), ldx, _lib.ptr(gt), _lib.ptr(yb), ldy, rows, d, IC.EPS, _lib.stream_ptr()))
    assert r == {"rms": 1}, r
    r = routed(lambda: lib.visrep_rmsnorm_stats(_lib.ptr(xb), ldx, _lib.ptr(rt), rows, d, IC.EPS, _lib.stream_ptr()))
    assert r == {"rms": 1, "stats_rows": 1}, r
    out = yb.cpu().numpy()
    assert (out[:, d:] == np.int16(SENTINEL)).all() and bool(torch.isnan(rt[rows:]).all())
    got = IC.from_bits(out[:, :d])
    ratio = float((np.abs(got - y) / (np.abs(y) * IC.out_rel(d) + 1e-38)).max())
    rt = rt[:rows].double().cpu().numpy()
    sratio = float((np.abs(rt[:, 0] - rstd) / (rstd * IC.rstd_rel(d))).max())
    print(f"[internvit] rmsnorm d {d} rows {rows}: worst |err| / bound {ratio:.3f}, rstd {sratio:.3f}")
    assert np.isfinite(got).all() and ratio <= 1.0, (d, rows, ratio)
    assert sratio <= 1.0 and not rt[:, 1].any() and not np.signbit(rt[:, 1]).any(), (d, rows, sratio)
    if rows > 1:                                                 # the all-zero row: rstd = eps^-0.5, outputs exactly zero
        assert abs(rt[-1, 0] - IC.EPS ** -0.5) <= IC.EPS ** -0.5 * IC.rstd_rel(d) and not got[-1].any()
    # in place
    r = routed(lambda: lib.visrep_rmsnorm(_lib.ptr(xb), ldx, _lib.ptr(gt), _lib.ptr(xb), ldx, rows, d, IC.EPS, _lib.stream_ptr()))
    assert torch.equal(xb[:, :d], yb[:, :d]) and bool((xb[:, d:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 2. statistics from the residual GEMMs
def resid_rms_stats(M, N, K, seed):
    """(routes, rt, rt of the read-only pass over the written rows, the written rows, the rows plain EPI_RESID writes for the same problem)"""
    lib = _lib.require_gpu()
    engine.ensure_scratch(DEV)
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16).to(DEV)
    bias, ls = torch.randn(N, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
    x0 = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)
    x, plain = x0.clone(), x0.clone()
    rt = torch.full((M, 2), float("nan"), device=DEV)
    part = torch.zeros(((M + 127) // 128 * 128) * (N // 64), 2, device=DEV)
    r = routed(lambda: lib.visrep_gemm_bf16_resid_rms_stats(_lib.ptr(a), K, _lib.ptr(w), K, _lib.ptr(bias), _lib.ptr(x), N, M, N, K, _lib.ptr(x), _lib.ptr(ls),
                                                          _lib.ptr(rt), _lib.ptr(part), IC.EPS, _lib.stream_ptr()))
    want = torch.full((M, 2), float("nan"), device=DEV)
    assert lib.visrep_rmsnorm_stats(_lib.ptr(x), N, _lib.ptr(want), M, N, IC.EPS, _lib.stream_ptr()) == 0
    # the same residual GEMM without statistics: the kernels of before (splitk_reduce for the split-K shape), the same decomposition and summation order
    rp = routed(lambda: lib.visrep_gemm_bf16(_lib.ptr(a), K, _lib.ptr(w), K, _lib.ptr(bias), _lib.ptr(plain), N, M, N, K, _lib.EPI_RESID, 0, _lib.ptr(plain),
                                             _lib.ptr(ls), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert {k: v for k, v in r.items() if k.startswith(("gemm", "splitk"))} == rp, (r, rp)
    ad, wd, bd, ld, xd = (t.double().cpu() for t in (a, w, bias, ls, x0))
    oracle = xd + ld * (ad @ wd.T + bd)
    # one bf16 rounding of the result (2^-8 relative) + the fp32 evaluation: K products summed in any order, bias, LayerScale and residual adds -
    # (K + 4) u relative to the sum of the magnitudes of everything that is added
    bound = oracle.abs() * 2.0 ** -8 + (K + 4) * IC.U * (xd.abs() + ld.abs() * (ad.abs() @ wd.abs().T + bd.abs())) * (1 + 2.0 ** -8)
    return r, rt.double().cpu(), want.double().cpu(), x, plain, (oracle, bound)


# (N, K) -> the launches the dispatcher makes: whole 256-column tiles leave partial sums in the epilogue (4 slots at N = 256, 48 at N = 3072: the
# finalize kernel's slot loop at an InternViT-like width); N = 1024 with a deep K is split-K, whose reduction (splitk_reduce_rms) writes the rows AND
# the statistics; N = 3200 is no multiple of 256, runs on the 128 x 128 kernel and falls back to the read-only pass - the epilogue-partials route
# cannot be reached at that width, so there only the route and the rows carry information
STAT_ROUTES = {(256, 256): {"gemm_256": 1, "stats_epilogue": 1, "rms": 1}, (3072, 256): {"gemm_256": 1, "stats_epilogue": 1, "rms": 1},
               (1024, 1024): {"splitk": 1, "stats_reduce": 1, "rms": 1}, (3200, 256): {"gemm_128": 1, "stats_rows": 1, "rms": 1}}


@pytest.mark.parametrize("M", [130, 300])
@pytest.mark.parametrize("N,K", sorted(STAT_ROUTES))
def test_rms_statistics_from_the_residual_gemm(N, K, M):
    r, rt, want, x, plain, oracle = resid_rms_stats(M, N, K, seed=N + M)
    assert r == STAT_ROUTES[(N, K)], r
    ratio = float(((rt[:, 0] - want[:, 0]).abs() / (want[:, 0] * IC.order_rel(N))).max())
    # the written rows: bit for bit those of the plain residual GEMM, and within the derived bound of the float64 result
    err = float(((x.double().cpu() - oracle[0]).abs() / oracle[1]).max())
    print(f"[internvit] resid stats N {N} K {K} M {M}: {r}, worst |rstd - pass| / bound {ratio:.3f}; rows vs float64: worst |err| / bound {err:.3f}")
    assert torch.equal(x, plain), int((x != plain).sum())
    assert err <= 1.0, err
    assert bool(torch.isfinite(rt).all()) and ratio <= 1.0, ratio
    assert not rt[:, 1].any() and not np.signbit(rt[:, 1].numpy()).any()


# ------------------------------------------------------------------------------------------------ 3. QK normalisation
def qk_launch(inp, rows, heads, hd, hp, edit=None):
    lib = _lib.require_gpu()
    da = heads * hp
    ldqk = 2 * da + 24
    buf = torch.full((rows + 2, ldqk), SENTINEL, dtype=torch.int16, device=DEV)
    buf[1:rows + 1, :2 * da] = dev_bits(inp["qk"].reshape(rows, 2 * da))
    if edit is not None:
        edit(buf)
    before = buf.clone()
    qg, kg = torch.from_numpy(inp["qg"].reshape(-1)).to(DEV), torch.from_numpy(inp["kg"].reshape(-1)).to(DEV)
    r = routed(lambda: lib.visrep_qk_rmsnorm(C.c_void_p(buf.data_ptr() + 2 * ldqk), ldqk, da, heads * hd, _lib.ptr(qg), _lib.ptr(kg), rows, IC.EPS, _lib.stream_ptr()))
    assert r == {"qk_norm": 1}, r
    out = buf.cpu().numpy()
    frame = np.ones(out.shape, dtype=bool)
    frame[1:rows + 1, :2 * da] = False
    assert (out[frame] == before.cpu().numpy()[frame]).all()                       # nothing outside the 2 da columns of the `rows` rows
    return out[1:rows + 1, :2 * da].reshape(rows, 2, heads, hp)


@pytest.mark.parametrize("rows", IC.QK_ROWS)
@pytest.mark.parametrize("heads,hd,hp", IC.QK_GEOMETRIES, ids=[f"{h}x{a}p{b}" for h, a, b in IC.QK_GEOMETRIES])
def test_qk_rmsnorm_contract(heads, hd, hp, rows):
    inp = IC.qk_input(rows, heads, hd, hp, seed=heads * hd + rows)
    want = IC.qk_oracle(inp, hd)
    bits = qk_launch(inp, rows, heads, hd, hp)
    got = IC.from_bits(bits)
    ratio = float((np.abs(got - want) / (np.abs(want) * IC.out_rel(heads * hp) + 1e-38)).max())
    print(f"[internvit] qk_rmsnorm {heads} x {hd} (pad {hp}) rows {rows}: worst |err| / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
    assert not bits[..., hd:].any()                                                 # padded columns stay exactly zero (bit pattern +0)
    if rows > 1:                                                                    # rows are independent: changing row i changes only row i
        i = rows // 2

        def edit(buf):
            buf[1 + i, :heads * hp] = dev_bits(inp["qk"][i, 0].reshape(-1) * 3.0 + 0.5 * (inp["qg"].reshape(-1) != 0))
        other = qk_launch(inp, rows, heads, hd, hp, edit)
        same = np.ones(rows, dtype=bool)
        same[i] = False
        assert np.array_equal(other[same], bits[same]) and not np.array_equal(other[i, 0], bits[i, 0])
        assert np.array_equal(other[i, 1], bits[i, 1])                              # and the K half of the row does not see its Q half


@pytest.mark.parametrize("name,over,rc,msg", IC.QK_REFUSALS, ids=[r[0] for r in IC.QK_REFUSALS])
def test_qk_rmsnorm_refusals(name, over, rc, msg):
    lib = _lib.require_gpu()
    buf = torch.full((1 << 16,), -1, dtype=torch.int16, device=DEV)
    _lib.routes(reset=True)
    assert lib.visrep_qk_rmsnorm(*IC.qk_refusal_args(over, buf.data_ptr()), _lib.stream_ptr()) == rc, _lib.last_error()
    assert msg in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    assert not any(_lib.routes(reset=True).values()) and bool((buf == -1).all())


# ------------------------------------------------------------------------------------------------ 4. tower parity
GEOMETRIES = {"T17-2x64": dict(heads=(2, 64), image=28, patch=7), "T65-2x64": dict(heads=(2, 64), image=112, patch=14),
              "T17-8x80": dict(heads=(8, 80), image=28, patch=7)}
ATTN = ("attn", "attn_cls", "attn_prefix", "attn_96", "attn_wide")


def forward_routes(eng, px, n):
    _lib.routes(reset=True)
    out = eng.forward(px, n_layers=n)
    torch.cuda.synchronize()
    return out, _lib.routes(reset=True)


def oracle_pair(spec, w, px, n):
    """(hidden_states[n] of the transformers module in fp32, the module's own bf16 error against it) on the same weights."""
    model = IC.hf_from_packed(spec, w)
    want = IC.hf_hidden(model, px, n)
    return want, IC.rel(IC.hf_hidden(model, px, n, torch.bfloat16), want), model


@pytest.mark.parametrize("kind", ["synthetic", "hostile"])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
@pytest.mark.parametrize("qk", [False, True], ids=["noqk", "qk"])
@pytest.mark.parametrize("norm", ["layernorm", "rmsnorm"])
def test_tiny_tower_parity(norm, qk, geo, kind, monkeypatch):
    spec = IC.internvit_tiny_spec(norm, qk, **GEOMETRIES[geo])
    w = VW.hostile_weights(spec, seed=6, profile="all") if kind == "hostile" else VW.synthetic_weights(spec, seed=6, qk_gains=True)
    px = bf(torch.randn(3, 3, spec.image_size, spec.image_size, generator=torch.Generator().manual_seed(spec.tokens)))
    want, e_ref, _ = oracle_pair(spec, w, px, 3)
    route = "attn_cls" if geo == "T65-2x64" else "attn_96" if geo == "T17-8x80" else "attn"
    for fuse in ("1", "0"):
        monkeypatch.setenv("VISREP_FUSE_LN", fuse)
        eng = engine.VitEngine(spec, w, DEV)
        got, r = forward_routes(eng, px.to(DEV), 3)
        e = IC.rel(got, want)
        print(f"[internvit] bf16 {norm} qk={qk} {geo} {kind} fuse_ln={fuse}: e_hip {e:.3e} e_ref {e_ref:.3e} ratio {e / e_ref:.2f} {({k: v for k, v in r.items() if v})}")
        assert {k: r[k] for k in ATTN if r[k]} == {route: 3}, r
        assert r["qk_norm"] == (3 if qk else 0)
        if norm == "rmsnorm":
            assert r["rms"] > 0 and (r["stats_rows"] + r["stats_epilogue"] + r["stats_reduce"] == (6 if fuse == "1" else 0)), r
        else:
            assert r["rms"] == 0, r
        assert e <= 2 * e_ref, (norm, qk, geo, kind, fuse, e, e_ref)
    monkeypatch.delenv("VISREP_FUSE_LN")
    e32 = IC.rel(engine.VitEngineF32(spec, w, DEV).forward(px.to(DEV), n_layers=3), want)
    ecpu = IC.rel(engine.VitEngineCPU(spec, w).forward(px, n_layers=3), want)
    print(f"[internvit] fp32 {norm} qk={qk} {geo} {kind}: engine {e32:.3e} host twin {ecpu:.3e}")
    assert e32 < 5e-6 and ecpu < 1e-5, (e32, ecpu)


@pytest.mark.parametrize("kind", ["synthetic", "hostile"])
def test_d1024_rms_tower_takes_its_statistics_from_the_split_k_reduction(kind):
    """d = 1024, K = 1024 and few rows: out-proj and fc2 are split-K pairs whose reduction (splitk_reduce_rms) writes the residual stream and
    the RMS statistics the next folded GEMM reads."""
    spec = IC.internvit_tiny_spec("rmsnorm", True, heads=(16, 64), image=28, patch=7, mlp=1024, layers=2)
    w = VW.hostile_weights(spec, seed=8, profile="all") if kind == "hostile" else VW.synthetic_weights(spec, seed=8, qk_gains=True)
    px = bf(torch.randn(3, 3, 28, 28, generator=torch.Generator().manual_seed(8)))
    want, e_ref, _ = oracle_pair(spec, w, px, 2)
    got, r = forward_routes(engine.VitEngine(spec, w, DEV), px.to(DEV), 2)
    e = IC.rel(got, want)
    print(f"[internvit] bf16 d 1024 rmsnorm {kind}: e_hip {e:.3e} e_ref {e_ref:.3e} ratio {e / e_ref:.2f} {({k: v for k, v in r.items() if v})}")
    assert r["stats_reduce"] == 3 and r["stats_rows"] == 1 and r["stats_epilogue"] == 0 and r["rms"] == 4 and r["qk_norm"] == 2, r
    assert e <= 2 * e_ref, (e, e_ref)


@pytest.mark.parametrize("cell", [c for c in IC.HOST_MATRIX if c[3] == (2, 72)], ids=lambda c: IC.matrix_id(c))
def test_fp32_engine_on_the_72_wide_heads_of_the_host_matrix(cell):
    norm, qk, bias, heads = cell
    model = IC.hf_model(seed=21, norm_type=norm, qk=qk, bias=bias, heads=heads)
    spec = VW.spec_from_hf_config(model.config, "x")
    w = VW.pack_hf_state_dict(model.state_dict(), spec)
    px = torch.randn(2, 3, 28, 28, generator=torch.Generator().manual_seed(5))
    eng = engine.VitEngineF32(spec, w, DEV)
    assert eng.gemm == "native"
    e = IC.rel(eng.forward(px.to(DEV), n_layers=3), IC.hf_hidden(model, px, 3))
    print(f"[internvit] fp32 engine {IC.matrix_id(cell)}: {e:.3e}")
    assert e < 5e-6, e


def test_split_fp32_route_declines_internvit_towers():
    spec = IC.internvit_tiny_spec("rmsnorm", True, heads=(4, 64), mlp=512)
    eng = engine.VitEngineF32(spec, VW.synthetic_weights(spec, seed=2), DEV)
    assert eng.gemm == "native"
    with pytest.raises(ValueError, match="split-bf16"):
        engine.VitEngineF32(spec, VW.synthetic_weights(spec, seed=2), DEV, gemm="split")
    plain = replace(spec, norm="layernorm", qk_norm=False)
    assert engine.VitEngineF32(plain, VW.synthetic_weights(plain, seed=2), DEV).gemm == "split"


# ------------------------------------------------------------------------------------------------ 5. where the pre-scaled-Q constant lives
def test_scale_fold_goes_into_qn_g(monkeypatch):
    spec = IC.internvit_tiny_spec("rmsnorm", True, **GEOMETRIES["T65-2x64"])
    w = VW.synthetic_weights(spec, seed=4, qk_gains=True)
    px = bf(torch.randn(3, 3, 112, 112, generator=torch.Generator().manual_seed(4)))
    want, e_ref, model = oracle_pair(spec, w, px, 3)
    outs = {}
    for mode, route in (("0", "attn"), ("2", "attn_cls")):
        monkeypatch.setenv("VISREP_Q_PRESCALE", mode)
        outs[mode], r = forward_routes(engine.VitEngine(spec, w, DEV), px.to(DEV), 3)
        assert r[route] == 3 and r["qk_norm"] == 3, r
    e0, e2, e02 = IC.rel(outs["0"], want), IC.rel(outs["2"], want), IC.rel(outs["2"], outs["0"])
    # The wrong packing, computed on the host: the constant c = head_dim^-0.5 log2(e) left in the Q rows of wqkv / bqkv (q_proj's weight and
    # bias times c - the norm behind the projection divides it out again, up to its eps term, which this keeps), and the attention kernel - told
    # that Q is pre-scaled - exponentiating the raw scores in base 2: softmax scale ln 2 where head_dim^-0.5 was meant.
    c = 64 ** -0.5 * 1.4426950408889634
    with torch.no_grad():
        for layer in model.encoder.layer:
            layer.attention.q_proj.weight.mul_(c)
            layer.attention.q_proj.bias.mul_(c)
            layer.attention.scale = math.log(2.0)
    e_wrong = IC.rel(IC.hf_hidden(model, px, 3), want)
    print(f"[internvit] scale fold: mode 0 {e0:.3e} mode 2 {e2:.3e} apart {e02:.3e}; bound {2 * e_ref:.3e}; constant left in wqkv {e_wrong:.3e}")
    assert e0 <= 2 * e_ref and e2 <= 2 * e_ref and e02 <= 2 * e_ref
    assert e_wrong > 2 * e_ref


# ------------------------------------------------------------------------------------------------ 6. full width, two layers, B = 2
def fast_weights(spec, seed, n_layers=2):
    os.environ["VISREP_FAST_SYNTHETIC"] = "1"
    try:
        return VW.synthetic_weights(spec, seed=seed, n_layers=n_layers, qk_gains=True)
    finally:
        os.environ.pop("VISREP_FAST_SYNTHETIC")


def test_internvit_6b_shape_routes():
    spec = VW.SPECS["OpenGVLab/InternViT-6B-448px-V2_5"]
    w = fast_weights(spec, 9)
    px = torch.randn(2, 3, 448, 448, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16).to(DEV)
    eng = engine.VitEngine(spec, w, DEV)
    assert (eng.head_dim, eng.head_pad, eng._q_mode) == (128, 128, 0)
    got, r = forward_routes(eng, px, 2)
    print(f"[internvit] 6B shape, 2 layers: {({k: v for k, v in r.items() if v})}")
    assert got.shape == (2, 1025, 3200) and bool(torch.isfinite(got.float()).all())
    assert {k: r[k] for k in ATTN} == dict(attn=2, attn_cls=0, attn_prefix=0, attn_96=0, attn_wide=0) and r["qk_norm"] == 2
    # d = 3200 is no multiple of the 256-column tile: out-proj and fc2 run on the 128 x 128 kernel, whose rows get the read-only RMS pass;
    # layer 0's first norm is that pass too: 1 + 3 statistics launches for two layers, all in their RMS form
    assert r["stats_rows"] == 4 and r["stats_epilogue"] == 0 and r["stats_reduce"] == 0 and r["rms"] == 4, r
    want = engine.VitEngineF32(spec, w, DEV).forward(px.float(), n_layers=2)
    e = IC.rel(got, want)
    print(f"[internvit] 6B shape vs fp32 engine: {e:.3e}")
    assert e < 2e-2, e


def test_internvit_300m_shape_takes_the_launches_of_a_dinov2_large_like_tower():
    spec = VW.SPECS["OpenGVLab/InternViT-300M-448px-V2_5"]
    twin = VW.tiny_spec("dinov2", image_size=448, patch=14, d=1024, heads=16, mlp=4096, layers=24)
    px = torch.randn(2, 3, 448, 448, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).to(DEV)
    w = fast_weights(spec, 10)
    got, r = forward_routes(engine.VitEngine(spec, w, DEV), px, 2)
    _, r2 = forward_routes(engine.VitEngine(twin, fast_weights(twin, 10), DEV), px, 2)
    print(f"[internvit] 300M shape, 2 layers: {({k: v for k, v in r.items() if v})}")
    assert r["attn_cls"] == 2 and r["attn"] == 0 and r["rms"] == 0 and r["qk_norm"] == 0 and r == r2, (r, r2)
    e = IC.rel(got, engine.VitEngineF32(spec, w, DEV).forward(px.float(), n_layers=2))
    assert e < 2e-2, e


# ------------------------------------------------------------------------------------------------ 7. plug-in tower
def test_plugin_tower_equals_the_engine_bit_for_bit(tmp_path):
    from law_of_vision_representation_in_mllms_amd.llava.model.multimodal_encoder.builder import build_internvit_vision_tower
    model = IC.hf_model(seed=13, norm_type="rms_norm", qk=True, bias=False, heads=(2, 64), image=112, patch=14)
    path = str(tmp_path / "internvl")
    IC.save_checkpoint(model, path, wrap=True)
    spec = VW.spec_from_hf_config(model.config, path)
    direct = engine.VitEngine(spec, VW.pack_hf_state_dict(model.state_dict(), spec), DEV)
    px = bf(torch.randn(3, 3, 112, 112, generator=torch.Generator().manual_seed(2))).to(DEV).to(torch.bfloat16)
    for feature, layer in (("patch", -2), ("cls_patch", -1)):
        cfg = SimpleNamespace(mm_vision_tower=path, vision_tower=path, mm_vision_select_layer=layer, mm_vision_select_feature=feature, device=DEV,
                              tower_precision="bf16")
        tower = build_internvit_vision_tower(cfg)
        assert tower.spec == spec
        want = direct.forward(px, n_layers=3 + 1 + layer)
        got = tower(px)
        assert torch.equal(got, want[:, 1:] if feature == "patch" else want)
    e = IC.rel(got, IC.hf_hidden(model, px.float().cpu(), -1))
    print(f"[internvit] plug-in tower vs transformers: {e:.3e}")
    assert e < 5e-2


# ------------------------------------------------------------------------------------------------ 8. zeroed new fields = the launches of before
@pytest.mark.parametrize("family,reg", [("clip", 0), ("dinov2", 4)])
def test_zeroed_new_fields_change_nothing(family, reg):
    spec = VW.tiny_spec(family, image_size=112, patch=14, d=128, heads=2, mlp=512, registers=reg)
    eng = engine.VitEngine(spec, VW.synthetic_weights(spec, seed=5), DEV)
    px = torch.randn(2, 3, 112, 112, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(DEV)
    a, ra = forward_routes(eng, px, 3)
    # the configuration and layer table as a caller written against the 640 header fills them: the sixteen old fields, the rest zero bytes
    old = _lib.VitConfig(spec.image_size, spec.patch, spec.d, spec.heads, eng.mlp_pad, 3, spec.tokens, int(spec.has_cls), int(spec.pre_ln),
                         _lib.ACT[spec.act], eng.kpad, float(spec.eps), eng._q_mode, eng.head_dim, eng.head_pad, spec.registers)
    assert bytes(old) == bytes(eng._cfg) and (old.norm, old.qk_norm) == (0, 0)
    assert all(eng._layers[i].qn_g is None and eng._layers[i].kn_g is None for i in range(3))
    eng._cfg = old
    b, rb = forward_routes(eng, px, 3)
    assert torch.equal(a, b) and ra == rb
    assert ra["rms"] == 0 and ra["qk_norm"] == 0 and ra["attn_prefix" if reg else "attn_cls"] == 3
    # one read-only statistics pass (layer 0's first norm), every other norm from the residual GEMMs, as since the fold was built
    assert ra["stats_rows"] + ra["stats_epilogue"] + ra["stats_reduce"] == 6, ra
