"""DINOv2 with registers without a GPU: the packed tower on the host twin against transformers' own Dinov2WithRegistersModel, plain DINOv2
untouched bit for bit, spec arithmetic, and the prefix attention scheme's rounding model under the existing derived bound
(tests/_register_cases.py; the kernel itself is tests/test_gpu_registers.py)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _attention_cases as AC  # noqa: E402
import _register_cases as RC  # noqa: E402

from law_of_vision_representation_in_mllms_amd import engine  # noqa: E402
from law_of_vision_representation_in_mllms_amd import vit_weights as VW  # noqa: E402
from law_of_vision_representation_in_mllms_amd.llava.model.multimodal_encoder.dinov2_encoder import DinoV2VisionTower  # noqa: E402


def host_tower(path, feature):
    args = SimpleNamespace(mm_vision_select_layer=-2, mm_vision_select_feature=feature, device="cpu", tower_precision="fp32")
    return DinoV2VisionTower(path, args, delay_load=False)


# ------------------------------------------------------------------------------------------------ 1. tower against transformers
@pytest.mark.parametrize("swiglu", [False, True], ids=["gelu", "swiglu"])
def test_tower_equals_transformers(tmp_path, swiglu):
    """State-dict names, the antialiased resize (native grid 5 -> 8 and 5 -> 4), register insertion order, no position term on registers."""
    pytest.importorskip("transformers")
    model = RC.hf_register_model(swiglu=swiglu, seed=3 + swiglu)
    for crop in ((112, 56) if not swiglu else (112,)):
        path = str(tmp_path / f"reg-{crop}")
        RC.save_checkpoint(model, path, crop)
        px = torch.randn(2, 3, crop, crop, generator=torch.Generator().manual_seed(crop))
        want = RC.hf_hidden(model, px)
        grid = crop // 14
        assert want.shape == (2, 1 + 4 + grid * grid, 128)
        for feature in ("patch", "cls_patch"):
            tower = host_tower(path, feature)
            assert tower.spec.registers == 4 and tower.spec.tokens == 5 + grid * grid and tower.num_patches == grid * grid
            assert tower.spec.act == ("swiglu" if swiglu else "gelu")
            got = tower(px)
            ref = RC.select(want, 4, feature)
            assert got.shape == ref.shape == (2, grid * grid + (feature == "cls_patch"), 128)
            e = RC.rel(got, ref)
            print(f"registers crop {crop} {feature} swiglu {swiglu}: rel-L2 {e:.2e}")
            assert e < 1e-5, (crop, feature, e)
        # the restatement the GPU tests use as their oracle is pinned here too
        hs = RC.hidden_states(tower.spec, VW.pack_hf_state_dict(model.state_dict(), tower.spec), px)
        assert RC.rel(hs[-2], want) < 1e-5


def test_packed_register_layout(tmp_path):
    pytest.importorskip("transformers")
    model = RC.hf_register_model(seed=9)
    cfg = model.config
    spec = VW.spec_from_hf_config(cfg, "reg", crop_size=112)
    assert (spec.family, spec.registers, spec.pos_grid, spec.image_size, spec.prefix, spec.tokens) == ("dinov2", 4, 5, 112, 5, 69)
    sd = {"dinov2_with_registers." + k: v for k, v in model.state_dict().items()}     # an AutoModel-prefixed checkpoint packs alike
    w = VW.pack_hf_state_dict(sd, spec)
    w0 = VW.pack_hf_state_dict(model.state_dict(), spec)
    assert all(torch.equal(a, b) for a, b in zip(VW.flatten(w).values(), VW.flatten(w0).values()))
    assert w["reg"].shape == (4, 128) and torch.equal(w["reg"], model.embeddings.register_tokens.detach().reshape(4, 128))
    assert w["pos"].shape == (69, 128) and not w["pos"][1:5].any() and w["pos_native"].shape == (26, 128)
    pn = w["pos_native"]
    aa = torch.nn.functional.interpolate(pn[1:].reshape(1, 5, 5, 128).permute(0, 3, 1, 2), size=(8, 8), mode="bicubic", align_corners=False,
                                         antialias=True).permute(0, 2, 3, 1).reshape(64, 128)
    assert torch.equal(w["pos"][5:], aa) and torch.equal(w["pos"][0], pn[0])
    # a change of resolution resizes once, from the native grid
    s12, w12 = VW.weights_at_resolution(spec, w, 168)
    a12 = torch.nn.functional.interpolate(pn[1:].reshape(1, 5, 5, 128).permute(0, 3, 1, 2), size=(12, 12), mode="bicubic", align_corners=False,
                                          antialias=True).permute(0, 2, 3, 1).reshape(144, 128)
    assert s12.tokens == 149 and torch.equal(w12["pos"][5:], a12) and not w12["pos"][1:5].any() and torch.equal(w12["pos_native"], pn)
    t = VW.prefix_table(spec, w)
    assert t.shape == (5, 128) and torch.equal(t[0], w["cls"]) and torch.equal(t[1:], w["reg"])


# ------------------------------------------------------------------------------------------------ 2. plain DINOv2 untouched
def _old_interpolate_pos(pos, has_cls, grid):
    """The resize as it was before registers existed: plain bicubic, no antialias."""
    cls = pos[:1] if has_cls else pos[:0]
    patch = pos[1:] if has_cls else pos
    n = int(round(patch.shape[0] ** 0.5))
    if n == grid:
        return pos
    d = pos.shape[-1]
    pp = patch.reshape(1, n, n, d).permute(0, 3, 1, 2).float()
    pp = torch.nn.functional.interpolate(pp, size=(grid, grid), mode="bicubic", align_corners=False)
    return torch.cat([cls, pp.permute(0, 2, 3, 1).reshape(grid * grid, d)], dim=0)


def _old_synthetic(spec, seed, n_layers):
    """synthetic_weights as it was: the same draws in the same order from RandomState(seed)."""
    rs = np.random.RandomState(seed)
    d, m, p = spec.d, spec.mlp, spec.patch
    m1 = 2 * m if spec.act == "swiglu" else m
    rn = lambda *shape, std=0.02, mean=0.0: torch.from_numpy((rs.standard_normal(shape) * std + mean).astype(np.float32))
    tokens = (spec.image_size // spec.patch) ** 2 + (1 if spec.has_cls else 0)
    w = {"patch_w": rn(d, 3 * p * p), "patch_b": rn(d) if spec.patch_bias else None, "cls": rn(d) if spec.has_cls else None, "pos": rn(tokens, d),
         "pre_ln_g": rn(d, std=0.1, mean=1.0) if spec.pre_ln else None, "pre_ln_b": rn(d) if spec.pre_ln else None}
    layers = []
    for _ in range(n_layers):
        layers.append({"ln1_g": rn(d, std=0.1, mean=1.0), "ln1_b": rn(d), "wqkv": rn(3 * d, d), "bqkv": rn(3 * d), "wo": rn(d, d), "bo": rn(d),
                       "ls1": rn(d, std=0.02, mean=0.1) if spec.layerscale else None, "ln2_g": rn(d, std=0.1, mean=1.0), "ln2_b": rn(d),
                       "w1": rn(m1, d), "b1": rn(m1), "w2": rn(d, m), "b2": rn(d), "ls2": rn(d, std=0.02, mean=0.1) if spec.layerscale else None})
    w["layers"] = layers
    return w


PLAIN = [n for n, s in VW.SPECS.items() if s.registers == 0]


@pytest.mark.parametrize("name", PLAIN)
def test_synthetic_stream_of_existing_specs_is_unchanged(name, monkeypatch):
    monkeypatch.delenv("VISREP_FAST_SYNTHETIC", raising=False)
    spec = VW.SPECS[name]
    assert spec.prefix == int(spec.has_cls) and spec.tokens == spec.grid ** 2 + int(spec.has_cls)
    got, want = VW.flatten(VW.synthetic_weights(spec, seed=3, n_layers=1)), VW.flatten(_old_synthetic(spec, 3, 1))
    assert list(got) == list(want) and "reg" not in got
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_plain_dinov2_checkpoint_packs_as_before():
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(5)
    cfg = transformers.Dinov2Config(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, mlp_ratio=4, patch_size=14, image_size=70)
    model = transformers.Dinov2Model(cfg).eval()
    with torch.no_grad():
        model.embeddings.position_embeddings.normal_()
    spec = VW.spec_from_hf_config(cfg, "plain", crop_size=112)
    assert spec.registers == 0 and spec.tokens == 65
    w = VW.pack_hf_state_dict(model.state_dict(), spec)
    native = model.embeddings.position_embeddings.detach().reshape(-1, 128)
    want = _old_interpolate_pos(native, True, 8)
    assert "reg" not in w and torch.equal(w["pos"], want) and torch.equal(w["pos_native"], native)
    # antialiasing only changes a DOWNsampling resize: there the two differ, and plain DINOv2 keeps the non-antialiased one
    assert not torch.equal(VW.interpolate_pos(native, True, 3, antialias=True), _old_interpolate_pos(native, True, 3))
    assert torch.equal(VW.weights_at_resolution(spec, w, 42)[1]["pos"], _old_interpolate_pos(native, True, 3))
    assert VW.prefix_table(spec, w) is w["cls"]


# ------------------------------------------------------------------------------------------------ 3. registry and spec arithmetic
def test_spec_arithmetic_and_registry():
    big, giant = VW.SPECS["facebook/dinov2-with-registers-large"], VW.SPECS["facebook/dinov2-with-registers-giant"]
    from dataclasses import replace
    assert replace(big, name="", registers=0) == replace(VW.SPECS["facebook/dinov2-large"], name="")
    assert replace(giant, name="", registers=0) == replace(VW.SPECS["facebook/dinov2-giant"], name="")
    for s in (big, giant):
        assert (s.registers, s.prefix, s.num_patches, s.tokens) == (4, 5, 256, 261)
        assert s.at_resolution(336).tokens == 581
    t = RC.register_tiny_spec()
    assert (t.d, t.heads, t.layers, t.grid, t.prefix, t.tokens) == (128, 2, 3, 8, 5, 69) and t.at_resolution(56).tokens == 21
    assert VW.tiny_spec("dinov2").registers == 0
    with pytest.raises(ValueError, match="CLS"):
        VW.tiny_spec("siglip", registers=2)
    with pytest.raises(ValueError, match="unsupported"):
        VW.spec_from_hf_config(SimpleNamespace(model_type="dinov2_with_something_else"))
    w = VW.synthetic_weights(t, seed=2, n_layers=1)
    assert w["reg"].shape == (4, 128) and w["pos"].shape == (69, 128) and not w["pos"][1:5].any() and w["pos"][5:].any()
    hw = VW.hostile_weights(t, seed=2, n_layers=1, profile="all")
    assert hw["hostile"]["const_token"] == 7 + 5                 # a patch row, not a register


def test_engines_name_the_right_row_count():
    t = RC.register_tiny_spec()
    w = VW.synthetic_weights(t, seed=2, n_layers=1)
    w["pos"] = w["pos"][:65]                                     # the table of the same tower without registers
    with pytest.raises(ValueError, match="65 rows, spec wants 69"):
        engine.VitEngineCPU(t, w)
    import inspect
    for cls in (engine.VitEngine, engine.VitEngineF32, engine.VitEngineCPU):        # the GPU engines need a device: same check, same words
        assert "rows, spec wants {spec.tokens}" in inspect.getsource(cls.__init__)


def test_host_twin_runs_a_synthetic_register_tower():
    for act in ("gelu", "swiglu"):
        for size in (112, 56):
            t = RC.register_tiny_spec(act, size)
            w = VW.hostile_weights(t, seed=4, profile="all")
            px = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(1))
            hs = RC.hidden_states(t, w, px)
            assert RC.rel(engine.VitEngineCPU(t, w).forward(px, n_layers=3), hs[3]) < 1e-5


# ------------------------------------------------------------------------------------------------ 4. the bound covers the prefix scheme
@pytest.mark.parametrize("pc", RC.KERNEL_CASES, ids=[c.id for c in RC.KERNEL_CASES])
def test_rounding_model_is_inside_the_bound(pc):
    inp = RC.make_inputs(pc)
    O, A, L = RC.oracle(inp, pc)
    r = AC.ratio(RC.rounding_model(inp, pc), O, A, L)
    print(f"[prefix-model] {pc.id}: ratio {r:.3f} (L = {L:.1f})")
    assert r <= 1.0, (pc.id, r)
    f = RC.figures(inp, pc)
    if pc.kind == "sink":
        assert (f["pre_max"][:, None] - f["tile_max"] > 39.0).all()
    elif pc.kind == "stair":
        steps = np.diff(np.concatenate([f["pre_max"][:, None], f["tile_max"]], 1), axis=1)
        assert (np.abs(steps - pc.param[0]) < 0.25).all()
    elif pc.kind == "apart" and pc.NP > 1:
        gaps = np.diff(np.sort(f["pre"], axis=1), axis=1)
        assert (gaps > 190.0).all()
        with np.errstate(under="ignore"):
            p = np.exp2((f["pre"] - f["pre_max"][:, None]).astype(np.float32)).astype(np.float32)
        assert ((p == 0).sum(1) == pc.NP - 1).all()             # all but one prefix weight underflow to exactly 0
