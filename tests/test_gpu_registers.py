"""DINOv2 with registers on the GPU: the prefix-key image-aligned attention kernel (attn_fwd_prefix, visrep_mhsa_prefix_fwd) through ctypes
against the float64 oracle and the derived bound of tests/_attention_cases.py, its equality with attn_fwd_cls at one side key, isolation,
refusals, route counters, and register towers on all three engines and through the plug-in tower.  Cases, packers and the tower oracle are in
tests/_register_cases.py (checked without a GPU by tests/test_host_registers.py).  `[prefix]` lines (pytest -s) print every ratio / error
before it is asserted."""
import ctypes as C
import os
import sys
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _attention_cases as AC  # noqa: E402
import _register_cases as RC  # noqa: E402

from law_of_vision_representation_in_mllms_amd import _lib, ascore_ops, engine  # noqa: E402
from law_of_vision_representation_in_mllms_amd import vit_weights as VW  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bf = lambda t: t.to(torch.bfloat16).float()


# ------------------------------------------------------------------------------------------------ 5. kernel contract
def launch(pc, packed, finite=True):
    lib = _lib.require_gpu()
    t = {n: torch.from_numpy(a.view(np.int16).copy()).to(DEV) for n, (a, _) in packed["bufs"].items()}
    p = lambda n: C.c_void_p(t[n].data_ptr() + 2 * packed["bufs"][n][1])
    d = packed["dims"]
    torch.cuda.synchronize()
    _lib.routes(reset=True)
    rc = lib.visrep_mhsa_prefix_fwd(p("q"), d["ldq"], p("vt"), d["ldvt"], p("vpre"), d["ldvp"], p("out"), d["ldo"], pc.B, pc.T, pc.NP, pc.H, 64,
                                    _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (pc.id, _lib.last_error())
    r = _lib.routes(reset=True)
    assert {k: v for k, v in r.items() if v} == {"attn_prefix": 1}, (pc.id, r)
    bits = AC.out_window(t["out"].cpu().numpy().view(np.uint16), packed)
    if finite:
        assert AC.finite_bits(bits).all(), f"{pc.id}: {int((~AC.finite_bits(bits)).sum())} non-finite outputs"
    return bits


def run(pc, layout="tight", inp=None, hostile=True, edit=None, finite=True):
    inp = RC.make_inputs(pc) if inp is None else inp
    packed = RC.pack(inp, pc, layout, hostile)
    if edit is not None:
        edit(packed)
    return launch(pc, packed, finite)


@pytest.mark.parametrize("pc", RC.KERNEL_CASES, ids=[c.id for c in RC.KERNEL_CASES])
def test_kernel_contract(pc):
    inp = RC.make_inputs(pc)
    O, A, L = RC.oracle(inp, pc)
    for lay in RC.LAYOUTS:
        got = AC.bf16_from_bits(run(pc, lay, inp)).reshape(pc.B, pc.T, pc.H, 64)
        r = AC.ratio(got, O, A, L)
        print(f"[prefix] {pc.id} {lay}: ratio {r:.3f} (L = {L:.1f})")
        assert r <= 1.0, (pc.id, lay, r)


# ------------------------------------------------------------------------------------------------ 6. one side key = attn_fwd_cls
@pytest.mark.parametrize("T", [65, 129])
def test_one_side_key_equals_the_cls_kernel_bit_for_bit(T):
    lib = _lib.require_gpu()
    pc = RC.PCase(1, T, 3, 2, seed=77 + T)
    inp = RC.make_inputs(pc)
    for lay in ("tight", "window"):
        packed = RC.pack(inp, pc, lay)
        a = launch(pc, packed)
        t = {n: torch.from_numpy(arr.view(np.int16).copy()).to(DEV) for n, (arr, _) in packed["bufs"].items()}
        p = lambda n: C.c_void_p(t[n].data_ptr() + 2 * packed["bufs"][n][1])
        d = packed["dims"]
        _lib.routes(reset=True)
        rc = lib.visrep_mhsa_cls_fwd(p("q"), d["ldq"], p("vt"), d["ldvt"], p("vpre"), d["ldvp"], p("out"), d["ldo"], pc.B, T, pc.H, 64, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and _lib.routes(reset=True)["attn_cls"] == 1
        b = AC.out_window(t["out"].cpu().numpy().view(np.uint16), packed)
        assert np.array_equal(a, b), (T, lay, int((a != b).sum()))


# ------------------------------------------------------------------------------------------------ 7. isolation
def test_image_alone_equals_image_among_nan_neighbours():
    pc = RC.PCase(5, 133, 3, 2, seed=91)
    inp = RC.make_inputs(pc)
    one = {n: inp[n][1:2] for n in ("q", "k", "v")}
    alone = run(pc._replace(B=1), "tight", one).reshape(pc.T, -1)

    def poison(packed):
        T, NP, P = pc.T, pc.NP, pc.T - pc.NP
        qb, vt, vp = packed["bufs"]["q"][0], packed["bufs"]["vt"][0], packed["bufs"]["vpre"][0]
        for b in (0, 2):
            qb[b * T:(b + 1) * T] = AC.NAN_BITS                 # Q and K rows of the other images
            vt[:, b * P:(b + 1) * P] = AC.NAN_BITS              # their V^T columns (image-aligned: whole 64-column blocks)
            vp[b * NP:(b + 1) * NP] = AC.NAN_BITS               # their prefix V rows
    got = run(pc, "tight", inp, edit=poison, finite=False).reshape(pc.B, pc.T, -1)
    assert np.array_equal(got[1], alone)
    assert not AC.finite_bits(got[0]).any() and not AC.finite_bits(got[2]).any()


def test_head_permutation_and_narrow_store():
    pc = RC.PCase(5, 133, 2, 3, seed=92)
    inp = RC.make_inputs(pc)
    perm = [2, 0, 1]
    pin = {n: np.ascontiguousarray(inp[n][:, :, perm]) for n in ("q", "k", "v")}
    a = run(pc, "tight", inp)
    assert np.array_equal(a.reshape(-1, 3, 64)[:, perm], run(pc, "tight", pin).reshape(-1, 3, 64))
    for lay in ("window", "narrow_a", "narrow_b"):
        assert np.array_equal(a, run(pc, lay, inp)), lay


# ------------------------------------------------------------------------------------------------ 8. refusals
@pytest.mark.parametrize("name,over,rc,msg", RC.REFUSALS, ids=[r[0] for r in RC.REFUSALS])
def test_refusals(name, over, rc, msg):
    lib = _lib.require_gpu()
    buf = torch.full((1 << 16,), -1, dtype=torch.int16, device=DEV)
    _lib.routes(reset=True)
    assert lib.visrep_mhsa_prefix_fwd(*RC.refusal_args(over, buf.data_ptr()), _lib.stream_ptr()) == rc, _lib.last_error()
    assert msg in _lib.last_error(), _lib.last_error()
    torch.cuda.synchronize()
    assert not any(_lib.routes(reset=True).values())
    assert bool((buf == -1).all())


def test_supported_query():
    lib = _lib.load()
    ok = lambda T, NP: bool(lib.visrep_mhsa_prefix_supported(T, NP))
    assert ok(261, 5) and ok(581, 5) and ok(65, 1) and ok(72, 8)
    assert not ok(73, 9) and not ok(64, 0) and not ok(21, 5) and not ok(5, 5) and not ok(149, 5)
    assert engine.mhsa_prefix_supported(69, 5)


# ------------------------------------------------------------------------------------------------ 9. / 10. towers: routes and parity
def attn_routes(eng, px, n):
    _lib.routes(reset=True)
    out = eng.forward(px, n_layers=n)
    torch.cuda.synchronize()
    r = _lib.routes(reset=True)
    return out, {k: r[k] for k in ("attn", "attn_cls", "attn_prefix", "attn_96", "attn_wide")}


def bf16_rule(got, spec, w, px, n, tag):
    want = RC.hidden_states(spec, w, px.float(), n_layers=n)[n]
    e_ref = RC.rel(RC.hidden_states(spec, w, px.float(), n_layers=n, dtype=torch.bfloat16)[n], want)
    e_hip = RC.rel(got, want)
    print(f"[prefix] {tag}: e_hip {e_hip:.3e} e_ref {e_ref:.3e}")
    assert e_hip < max(1.5 * e_ref, 2e-2), (tag, e_hip, e_ref)


def test_route_counters(monkeypatch):
    spec8, spec4 = RC.register_tiny_spec(), RC.register_tiny_spec(image_size=56)
    w8, w4 = VW.synthetic_weights(spec8, seed=5), VW.synthetic_weights(spec4, seed=5)
    px8 = torch.randn(2, 3, 112, 112, device=DEV, dtype=torch.bfloat16)
    px4 = torch.randn(2, 3, 56, 56, device=DEV, dtype=torch.bfloat16)
    zero = dict(attn=0, attn_cls=0, attn_prefix=0, attn_96=0, attn_wide=0)
    assert attn_routes(engine.VitEngine(spec8, w8, DEV), px8, 3)[1] == dict(zero, attn_prefix=3)
    assert attn_routes(engine.VitEngine(spec4, w4, DEV), px4, 3)[1] == dict(zero, attn=3)
    plain = VW.tiny_spec("dinov2", image_size=112, patch=14, d=128, heads=2, mlp=512)
    assert attn_routes(engine.VitEngine(plain, VW.synthetic_weights(plain, seed=5), DEV), px8, 3)[1] == dict(zero, attn_cls=3)
    monkeypatch.setenv("VISREP_Q_PRESCALE", "1")
    assert attn_routes(engine.VitEngine(spec8, w8, DEV), px8, 3)[1] == dict(zero, attn=3)


@pytest.mark.parametrize("hostile", [None, "all"], ids=["synthetic", "hostile"])
@pytest.mark.parametrize("act", ["gelu", "swiglu"])
@pytest.mark.parametrize("size", [112, 56], ids=["grid8", "grid4"])
def test_tiny_register_tower_parity(size, act, hostile, monkeypatch):
    spec = RC.register_tiny_spec(act, size)
    w = VW.hostile_weights(spec, seed=6, profile=hostile) if hostile else VW.synthetic_weights(spec, seed=6)
    px = bf(torch.randn(3, 3, size, size, generator=torch.Generator().manual_seed(size)))
    want_route = "attn_prefix" if size == 112 else "attn"
    got, r = attn_routes(engine.VitEngine(spec, w, DEV), px.to(DEV), 3)
    assert r[want_route] == 3 and sum(r.values()) == 3, r
    bf16_rule(got, spec, w, px, 3, f"bf16 {spec.tokens} {act} {hostile} {want_route}")
    if size == 112:                                              # the general route of the same tower meets the same bar
        monkeypatch.setenv("VISREP_Q_PRESCALE", "1")
        got1, r1 = attn_routes(engine.VitEngine(spec, w, DEV), px.to(DEV), 3)
        monkeypatch.delenv("VISREP_Q_PRESCALE")
        assert r1["attn"] == 3 and r1["attn_prefix"] == 0, r1
        bf16_rule(got1, spec, w, px, 3, f"bf16 {spec.tokens} {act} {hostile} attn")
    hs = RC.hidden_states(spec, w, px)
    for name, eng in (("native", engine.VitEngineF32(spec, w, DEV, gemm="native")),):
        e = RC.rel(eng.forward(px.to(DEV), n_layers=3), hs[3])
        print(f"[prefix] fp32 {name} {spec.tokens} {act} {hostile}: {e:.3e}")
        assert e < 5e-6, (name, e)
    assert RC.rel(engine.VitEngineCPU(spec, w).forward(px, n_layers=3), hs[3]) < 1e-5


@pytest.mark.parametrize("products", [6, 3])
def test_split_fp32_register_tower(products):
    """The split-bf16 fp32 route needs d, mlp % 256 and heads of 64: the register spec at d 256."""
    spec = VW.tiny_spec("dinov2", image_size=112, patch=14, d=256, heads=4, mlp=512, layers=2, registers=4)
    w = VW.synthetic_weights(spec, seed=8)
    px = torch.randn(2, 3, 112, 112, generator=torch.Generator().manual_seed(8))
    eng = engine.VitEngineF32(spec, w, DEV, gemm="split", products=products)
    assert eng.gemm == "split"
    e = RC.rel(eng.forward(px.to(DEV), n_layers=2), RC.hidden_states(spec, w, px)[2])
    print(f"[prefix] fp32 split x{products}: {e:.3e}")
    assert e < 5e-6, e


def test_resolution_change_against_transformers(tmp_path):
    """weights_at_resolution grid 8 -> grid 12 (T = 149: the general route) against transformers' own interpolation at 168 px."""
    pytest.importorskip("transformers")
    model = RC.hf_register_model(seed=12)
    spec = VW.spec_from_hf_config(model.config, "reg", crop_size=112)
    w = VW.pack_hf_state_dict(model.state_dict(), spec)
    s12, w12 = VW.weights_at_resolution(spec, w, 168)
    px = bf(torch.randn(2, 3, 168, 168, generator=torch.Generator().manual_seed(12)))
    want = RC.hf_hidden(model, px, layer=-1)
    got, r = attn_routes(engine.VitEngine(s12, w12, DEV), px.to(DEV), 3)
    assert r["attn"] == 3 and r["attn_prefix"] == 0, r
    e_ref = RC.rel(RC.hidden_states(s12, w12, px, dtype=torch.bfloat16)[3], want)
    e = RC.rel(got, want)
    print(f"[prefix] grid 12 vs transformers: e_hip {e:.3e} e_ref {e_ref:.3e}")
    assert e < max(1.5 * e_ref, 2e-2)
    assert RC.rel(engine.VitEngineF32(s12, w12, DEV).forward(px.to(DEV), n_layers=3), want) < 1e-5


# ------------------------------------------------------------------------------------------------ 11. full width, once
def test_register_large_at_full_width():
    spec = VW.SPECS["facebook/dinov2-with-registers-large"]
    os.environ["VISREP_FAST_SYNTHETIC"] = "1"
    try:
        w = VW.synthetic_weights(spec, seed=9, n_layers=2)
    finally:
        os.environ.pop("VISREP_FAST_SYNTHETIC")
    px = bf(torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(4)))
    eng = engine.VitEngine(spec, w, DEV)
    got, r = attn_routes(eng, px.to(DEV), 2)
    assert got.shape == (2, 261, 1024) and r == dict(attn=0, attn_cls=0, attn_prefix=2, attn_96=0, attn_wide=0), r
    want = engine.VitEngineF32(spec, w, DEV).forward(px.to(DEV), n_layers=2)
    e = RC.rel(got, want)
    print(f"[prefix] register-large 2 layers vs fp32 engine: {e:.3e}")
    assert e < 2e-2, e
    pxd = px.to(DEV).to(torch.bfloat16)
    out = torch.empty(2, 261, 1024, dtype=torch.bfloat16, device=DEV)
    eager = eng.forward(pxd, n_layers=2).clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.forward(pxd, n_layers=2, out=out)                    # warm the workspace outside the capture
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            eng.forward(pxd, n_layers=2, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ------------------------------------------------------------------------------------------------ 12. plug-in path
def test_plugin_tower_from_a_transformers_checkpoint(tmp_path):
    pytest.importorskip("transformers")
    from law_of_vision_representation_in_mllms_amd.llava.model.multimodal_encoder.builder import build_dinov2_vision_tower
    model = RC.hf_register_model(seed=3)
    path = str(tmp_path / "reg-112")
    RC.save_checkpoint(model, path, 112)
    px = bf(torch.randn(4, 3, 112, 112, generator=torch.Generator().manual_seed(112)))
    stack = {}
    for feature, rows in (("patch", 64), ("cls_patch", 65)):
        cfg = lambda dev: SimpleNamespace(mm_vision_tower=path, vision_tower=path, mm_vision_select_layer=-2, mm_vision_select_feature=feature,
                                          device=dev, tower_precision="bf16" if dev != "cpu" else "fp32")
        gpu, host = build_dinov2_vision_tower(cfg(DEV)), build_dinov2_vision_tower(cfg("cpu"))
        assert gpu.spec.registers == 4 and gpu.num_patches == 64
        got, ref = gpu(px.to(DEV).to(torch.bfloat16)), host(px)
        assert got.shape == ref.shape == (4, rows, 128)
        e = RC.rel(got, ref)
        print(f"[prefix] plug-in {feature}: {e:.3e}")
        assert e < 2e-2, (feature, e)
        stack[feature] = got
    assert torch.equal(stack["cls_patch"][:, 1:], stack["patch"])
    a = ascore_ops.max_cos_mean(stack["patch"][:2].float(), stack["patch"][2:].float())
    assert a.shape == (2,) and bool(torch.isfinite(a).all())
