"""SwiGLU-FFN towers on the GPU: the kernel contract of visrep_gemm_bf16_gated on every route of the dispatcher, the composed forward on
every engine, DINOv2-giant at full width, the plug-in path from a checkpoint directory.  References and bounds: tests/_swiglu_cases.py."""
import json
import os
import sys
from dataclasses import replace
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _swiglu_cases as SC  # noqa: E402

from law_of_vision_representation_in_mllms_amd import _lib, engine  # noqa: E402
from law_of_vision_representation_in_mllms_amd import vit_weights as VW  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GIANT = "facebook/dinov2-giant"


def bf(x):
    return x.to(torch.bfloat16)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


def fast_weights(spec, seed, n_layers, hostile=None):
    os.environ["VISREP_FAST_SYNTHETIC"] = "1"
    try:
        return VW.hostile_weights(spec, seed=seed, n_layers=n_layers, profile=hostile) if hostile else VW.synthetic_weights(spec, seed=seed, n_layers=n_layers)
    finally:
        os.environ.pop("VISREP_FAST_SYNTHETIC", None)


# ------------------------------------------------------------------------------------------------ kernel contract
def run_gated(M, mp, K, ln=False, seed=0, window=None, bias=True):
    """One visrep_gemm_bf16_gated problem against float64 on the same bf16-rounded operands; returns the routes it took.
    window = (ldc, col0): C is a column window of a NaN-filled [M + 2, ldc] buffer; everything outside rows [0, M) x the window must stay NaN."""
    g = torch.Generator().manual_seed(seed)
    a = bf(torch.randn(M, K, generator=g))
    w = bf(torch.randn(2 * mp, K, generator=g) * 0.25)
    b = torch.randn(2 * mp, generator=g) if bias else None
    lnp = None
    if ln:
        rt = torch.stack([torch.rand(M, generator=g) * 1.5 + 0.5, torch.randn(M, generator=g)], dim=1)
        lnp = (rt, torch.randn(2 * mp, generator=g))
    want, bound = SC.gated_reference(a.float(), w.float(), b, lnp)
    ldc, col0 = window or (mp, 0)
    buf = torch.full((M + 2, ldc), float("nan"), dtype=torch.bfloat16, device=DEV)
    out = buf[1:M + 1, col0:col0 + mp]
    rt_dev = None
    if ln:
        rt_dev = torch.zeros((M + 127) // 128 * 128 + 8, 2, device=DEV)
        rt_dev[:M] = lnp[0].to(DEV)
    engine.ensure_scratch(torch.device(DEV))
    torch.cuda.synchronize()
    _lib.routes(reset=True)
    engine.gemm_gated(a.to(DEV), SC.interleave(w, mp).contiguous().to(DEV), None if b is None else SC.interleave(b, mp).contiguous().to(DEV),
                      rt_dev, SC.interleave(lnp[1], mp).contiguous().to(DEV) if ln else None, out=out)
    torch.cuda.synchronize()
    r = _lib.routes(reset=True)
    got = out.double().cpu()
    err = (got - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"gated M={M} mp={mp} K={K} ln={ln} window={window}: max err/bound {worst:.3f}, max err {err.max().item():.3e}, routes", {k: v for k, v in r.items() if v})
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (M, mp, K, ln, worst)
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[1:M + 1, col0:col0 + mp] = False
    assert torch.isnan(buf[mask]).all(), "the kernel wrote outside its window"
    assert r["splitk"] == 0, r                                  # gated problems are never split along K (try_split_k returns 0)
    return r


@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("M", [1, 127, 129, 257, 512])
def test_gated_gemm_256_route_and_m_edges(M, ln):
    r = run_gated(M, 128, 128, ln=ln, seed=M)
    assert r["gemm_256"] == 1 and r["gemm_128"] == 0 and r["gemm_tail"] == 0, r


@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("M,mp", [(1, 64), (127, 64), (129, 192), (257, 64)])
def test_gated_gemm_128_route_and_m_edges(M, mp, ln):
    """N = 2 mp is not a multiple of 256: the 128 x 128 kernel alone (192: its last column tile is half empty)."""
    r = run_gated(M, mp, 64, ln=ln, seed=M + mp)
    assert r["gemm_128"] == 1 and r["gemm_256"] == 0, r


def head_tail_rows(edge):
    cus = _lib.load().visrep_device_cu_count()
    return cus // 32 * 256 + edge                              # mp = 4096: 32 column tiles; one full round + 32 tiles (<= CUs / 4) of remainder


@pytest.mark.parametrize("ln", [False, True])
def test_gated_gemm_head_plus_tail_at_full_width(ln):
    """mp = 4096 (giant's hidden width): one full round of 256 x 256 tiles, the remaining 129 rows on the 128 x 128 kernel, whose C
    pointer must advance by m1 * ldc with ldc = mp (not N)."""
    r = run_gated(head_tail_rows(129), 4096, 128, ln=ln, seed=11)
    assert r["gemm_256"] == 1 and r["gemm_tail"] == 1 and r["gemm_128"] == 1, r


def test_gated_gemm_is_not_split_along_k():
    """K = 1024 and two tiles: any other epilogue would take the split-K pair here (scratch is registered); the gated one must not."""
    engine.ensure_scratch(torch.device(DEV))
    a = bf(torch.randn(128, 1024)).to(DEV)
    w = bf(torch.randn(256, 1024) * 0.05).to(DEV)
    _lib.routes(reset=True)
    engine.gemm(a, w)
    torch.cuda.synchronize()
    assert _lib.routes(reset=True)["splitk"] == 1              # the shape is split-K territory
    r = run_gated(128, 128, 1024, ln=True, seed=5)
    assert r["splitk"] == 0 and r["gemm_256"] + r["gemm_128"] == 1, r


def test_gated_gemm_v2_kernel_and_the_k_rule():
    """The 256 x 256 v2 kernel (64-byte LDS rows) is the fallback of the default for K % 64 != 0 - which the dispatcher refuses for every
    epilogue (K % 64 == 0 is its own rule, the 128 x 128 tail needs it), so the gated instantiation of v2 is reached through the variant knob."""
    lib = _lib.load()
    old = lib.visrep_set_gemm_variant(2)
    try:
        for M, ln in ((257, False), (512, True)):
            r = run_gated(M, 128, 192, ln=ln, seed=21)
            assert r["gemm_256"] == 1, r
        r = run_gated(head_tail_rows(1), 4096, 64, ln=True, seed=22)
        assert r["gemm_256"] == 1 and r["gemm_tail"] == 1, r
    finally:
        lib.visrep_set_gemm_variant(old)
    a = torch.zeros(64, 96, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(256, 96, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="multiples of 64"):
        engine.gemm_gated(a, w)


@pytest.mark.parametrize("window", [(128 + 64, 8), (128 + 64, 4), (128 + 68, 36)])
def test_gated_gemm_windowed_output(window):
    """ldc > mp, NaN around the window: 16-byte aligned (wide stores), 8-byte aligned only, and an ldc that is not a multiple of 8."""
    for M in (129, 300):
        run_gated(M, 128, 64, ln=True, seed=31, window=window)
    run_gated(130, 64, 64, ln=False, seed=32, window=(64 + 16, 12))


@pytest.mark.parametrize("reserved", [0, 64, 128])
def test_gated_head_plus_tail_at_other_cu_counts(reserved):
    lib = _lib.load()
    old = lib.visrep_set_reserved_cus(reserved)
    try:
        r = run_gated(head_tail_rows(77), 4096, 64, ln=True, seed=41)
        assert r["gemm_256"] == 1 and r["gemm_tail"] == 1, (reserved, r)
    finally:
        lib.visrep_set_reserved_cus(old)


def test_unfused_pair_matches_its_definition():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(300, 2 * 344, generator=g)
    want = torch.nn.functional.silu(x[:, :344].double()) * x[:, 344:].double()
    assert rel(engine.swiglu(x.to(DEV)), want) < 1e-6
    xb = bf(torch.randn(300, 2 * 384, generator=g))
    wb = torch.nn.functional.silu(xb[:, :384].double()) * xb[:, 384:].double()
    got = engine.swiglu(xb.to(DEV)).double().cpu()
    assert ((got - wb).abs() <= (2.0 ** -8 + 2.0 ** -20) * wb.abs() + 1e-30).all()


@pytest.mark.parametrize("which", [1, 2, 3, 4])
def test_refusals_on_the_device(which):
    lib = _lib.load()
    _lib.routes(reset=True)
    assert lib.visrep_debug_gated_refusal(which) == -1 and "gated" in _lib.last_error()
    assert sum(_lib.routes(reset=True).values()) == 0
    a = torch.zeros(64, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="gated"):           # the row-mapped entry point hands the combination to the dispatcher
        engine.gemm_rows(a, 4, 8, 0, 16, torch.zeros(256, 64, dtype=torch.bfloat16, device=DEV), epilogue=_lib.EPI_GATED)


# ------------------------------------------------------------------------------------------------ composed forward
def bf16_rule(got, spec, w, px, n):
    want = SC.swiglu_hidden_states(spec, w, px.float(), n_layers=n)[n]
    e_ref = rel(SC.swiglu_hidden_states(spec, w, px.float(), n_layers=n, dtype=torch.bfloat16)[n], want)
    e_hip = rel(got, want)
    print(f"{spec.name} layers {n}: e_hip {e_hip:.3e} e_ref {e_ref:.3e}")
    assert e_hip < max(1.5 * e_ref, 2e-2), (e_hip, e_ref)


@pytest.mark.parametrize("fuse_ln", [True, False])
@pytest.mark.parametrize("fuse_gate", [True, False])
def test_tiny_swiglu_tower_bf16(fuse_gate, fuse_ln):
    spec = SC.swiglu_tiny_spec()
    w = VW.synthetic_weights(spec, seed=5)
    px = bf(torch.randn(3, 3, 42, 42, generator=torch.Generator().manual_seed(2)))
    eng = engine.VitEngine(spec, w, DEV, fuse_ln=fuse_ln, fuse_gate=fuse_gate)
    assert eng.mlp_pad == 384 and eng.fuse_gate == fuse_gate
    bf16_rule(eng.forward(px.to(DEV), n_layers=3), spec, w, px, 3)
    assert _lib.load().visrep_set_fuse_gate(1) == 1            # the engine restores the per-thread knob


def test_fuse_gate_env_knob(monkeypatch):
    spec = SC.swiglu_tiny_spec()
    w = VW.synthetic_weights(spec, seed=5, n_layers=1)
    monkeypatch.setenv("VISREP_FUSE_GATE", "0")
    assert engine.VitEngine(spec, w, DEV).fuse_gate is False
    monkeypatch.delenv("VISREP_FUSE_GATE")
    assert engine.VitEngine(spec, w, DEV).fuse_gate is True


def test_tiny_swiglu_tower_fp32_and_host():
    """fp32 engines at the level tests/test_gpu_f32.py holds its towers to (5e-6 against float64 per hidden state); native route on the tiny
    spec, split route on a spec whose shapes allow it (d, mlp % 256, heads of 64)."""
    spec = SC.swiglu_tiny_spec()
    w = VW.synthetic_weights(spec, seed=6)
    px = torch.randn(2, 3, 42, 42, generator=torch.Generator().manual_seed(3))
    hs = SC.swiglu_hidden_states(spec, w, px)
    native = engine.VitEngineF32(spec, w, DEV)
    assert native.gemm == "native"
    for n in (1, 3):
        assert rel(native.forward(px.to(DEV), n_layers=n), hs[n]) < 5e-6, n
    assert rel(engine.VitEngineCPU(spec, w).forward(px, n_layers=3), hs[3]) < 1e-5
    s2 = SC.swiglu_tiny_spec(d=256, heads=4, mlp=512, layers=2)
    w2 = VW.synthetic_weights(s2, seed=7)
    hs2 = SC.swiglu_hidden_states(s2, w2, px)
    split = engine.VitEngineF32(s2, w2, DEV, gemm="split")
    assert split.gemm == "split"
    assert rel(split.forward(px.to(DEV), n_layers=2), hs2[2]) < 5e-6
    assert rel(engine.VitEngineF32(s2, w2, DEV, gemm="native").forward(px.to(DEV), n_layers=2), hs2[2]) < 5e-6


@pytest.mark.parametrize("hostile", [None, "all"])
def test_giant_at_full_width(hostile):
    """SPECS['facebook/dinov2-giant'] at 224 px: d 1536, 24 heads, hidden 4096 (fc1 [8192, 1536]), fast synthetic weights, 3 of the 40
    layers and 2 images (the float64 restatement on the host sets the cost; depth is reduced, never width).  hostile = 'all': outlier
    channels, a near-constant token, spread LayerScale, sharp heads (vit_weights.hostile_weights).
    Routes at these 514 rows: every layer's gated fc1 (N = 8192: 3 x 32 tiles) on the 256 x 256 kernel - a gated problem is never split
    along K - while Q|K|V, out-proj and fc2 (K >= 1024, few tiles) take the split-K pair, as for any tower at two images."""
    spec = VW.SPECS[GIANT]
    w = fast_weights(spec, 9, 3, hostile)
    px = bf(torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(4)))
    eng = engine.VitEngine(spec, w, DEV)
    assert (eng.head_pad, eng.mlp_pad, eng.fuse_gate, eng.fuse_ln) == (64, 4096, True, True)
    _lib.routes(reset=True)
    got = eng.forward(px.to(DEV), n_layers=3)
    torch.cuda.synchronize()
    r = _lib.routes(reset=True)
    print("giant routes", {k: v for k, v in r.items() if v})
    assert r["gemm_256"] >= 3 and r["gemm_256"] + r["gemm_128"] + r["splitk"] >= 3 * 4, r
    bf16_rule(got, spec, w, px, 3)


# ------------------------------------------------------------------------------------------------ plug-in path
def write_dinov2_swiglu_checkpoint(path, spec, w):
    """A transformers-layout checkpoint directory (config.json + model.safetensors) of a Dinov2Model with use_swiglu_ffn, from packed weights."""
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({"model_type": "dinov2", "hidden_size": spec.d, "num_attention_heads": spec.heads, "mlp_ratio": 4, "use_swiglu_ffn": True,
                   "image_size": spec.image_size, "patch_size": spec.patch, "num_hidden_layers": spec.layers, "hidden_act": "gelu",
                   "layer_norm_eps": spec.eps, "num_channels": 3}, f)
    d = spec.d
    sd = {"embeddings.patch_embeddings.projection.weight": w["patch_w"].view(d, 3, spec.patch, spec.patch),
          "embeddings.patch_embeddings.projection.bias": w["patch_b"], "embeddings.cls_token": w["cls"].view(1, 1, d),
          "embeddings.position_embeddings": w["pos"].view(1, -1, d)}
    for i, L in enumerate(w["layers"]):
        pre = f"encoder.layer.{i}."
        for j, c in enumerate(("query", "key", "value")):
            sd[pre + f"attention.attention.{c}.weight"], sd[pre + f"attention.attention.{c}.bias"] = L["wqkv"][j * d:(j + 1) * d], L["bqkv"][j * d:(j + 1) * d]
        for hf, (wk, bk) in {"attention.output.dense": ("wo", "bo"), "norm1": ("ln1_g", "ln1_b"), "norm2": ("ln2_g", "ln2_b"),
                             "mlp.weights_in": ("w1", "b1"), "mlp.weights_out": ("w2", "b2")}.items():
            sd[pre + hf + ".weight"], sd[pre + hf + ".bias"] = L[wk], L[bk]
        sd[pre + "layer_scale1.lambda1"], sd[pre + "layer_scale2.lambda1"] = L["ls1"], L["ls2"]
    save_file({k: v.contiguous().clone() for k, v in sd.items()}, os.path.join(path, "model.safetensors"))


def test_plugin_tower_from_a_checkpoint_directory(tmp_path):
    from law_of_vision_representation_in_mllms_amd.llava.model.multimodal_encoder.dinov2_encoder import DinoV2VisionTower
    spec = replace(VW.SPECS[GIANT], layers=2, pos_grid=16)
    w = fast_weights(spec, 8, 2)
    path = str(tmp_path / "dinov2-giant-tiny-depth")
    write_dinov2_swiglu_checkpoint(path, spec, w)
    px = bf(torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(3)))
    direct = engine.VitEngine(spec, w, DEV).forward(px.to(DEV), n_layers=1)
    for dev, prec in ((DEV, "bf16"), (DEV, "fp32"), ("cpu", "fp32")):
        args = SimpleNamespace(mm_vision_select_layer=-2, mm_vision_select_feature="patch", device=dev, tower_precision=prec)
        tower = DinoV2VisionTower(path, args, delay_load=False)
        assert tower.hidden_size == 1536 and tower.spec.act == "swiglu" and tower.spec.mlp == 4096
        feats = tower(px if prec == "bf16" else px.float())
        assert feats.shape == (2, 256, 1536)
        if prec == "bf16":
            assert torch.equal(feats, direct[:, 1:])
        else:
            assert rel(feats, direct[:, 1:]) < 2e-2
