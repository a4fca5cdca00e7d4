"""ConvNeXt towers, host side: spec reader, packer (both key layouts), host twins of the two new kernels against float64, refusals and the
tower protocol.  No GPU needed."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _convnext_cases as CC
from law_of_vision_representation_in_mllms_amd import _lib, convnext_weights as CW, engine
from law_of_vision_representation_in_mllms_amd.llava.model.multimodal_encoder import builder
from law_of_vision_representation_in_mllms_amd.llava.model.multimodal_encoder.convnext_encoder import ConvNextVisionTower


# ------------------------------------------------------------------------------------------------ 1. spec reader and packer
def hf_model(spec, seed=0):
    """A random-init transformers.ConvNextModel with non-trivial LayerScale, norm weights and biases."""
    import transformers
    torch.manual_seed(seed)
    model = transformers.ConvNextModel(CW.hf_config(spec)).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "layer_scale" in n or ("layernorm" in n and n.endswith("weight")):
                p.copy_((torch.rand(p.shape, generator=g) + 0.5) * torch.where(torch.rand(p.shape, generator=g) < 0.25, -1.0, 1.0))
            elif n.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            elif "dwconv.weight" in n:
                p.copy_(torch.randn(p.shape, generator=g) / 7)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * p[0].numel() ** -0.5)
    return model


@pytest.mark.parametrize("image,batch", [(64, 2), (96, 3)])
def test_packer_round_trip_against_transformers(image, batch):
    spec0 = CW.tiny_spec(image, **CC.TINY)
    model = hf_model(spec0)
    spec = CW.spec_from_hf_config(model.config, "tiny")
    assert (spec.depths, spec.hidden_sizes, spec.image_size, spec.eps, spec.layerscale) == ((1, 1, 2, 1), (64, 128, 192, 256), image, 1e-6, True)
    w = CW.pack_hf_state_dict(model.state_dict(), spec)
    px = CC.pixels(batch, image, 3)
    want = CC.hf_hidden_states(model, px)
    got = CW.torch_forward(spec, w, px)
    assert [tuple(t.shape) for t in got] == [(batch, spec.grid(k) ** 2, spec.width(k)) for k in range(5)]
    for k in range(5):
        assert CC.rel(got[k], want[k]) < 1e-5, k
    # ... and the inverse the GPU tests build their oracle with
    back = CW.to_hf_state_dict(spec, w)
    sd = model.state_dict()
    assert set(back) == {k for k in sd if not k.startswith("layernorm.")} and all(torch.equal(back[k], sd[k]) for k in back)


def test_timm_layout_packs_to_the_same_tensors():
    spec = CW.tiny_spec(64, **CC.TINY)
    model = hf_model(spec, seed=2)
    a = CW.pack_hf_state_dict(model.state_dict(), spec)
    b = CW.pack_hf_state_dict(CC.timm_state_dict(model.state_dict()), spec)
    c = CW.pack_hf_state_dict({"convnext." + k: v for k, v in model.state_dict().items()}, spec)
    for other in (b, c):
        for k in ("stem_w", "stem_b", "stem_ln_g", "stem_ln_b"):
            assert torch.equal(a[k], other[k]), k
        for sa, sb in zip(a["stages"], other["stages"]):
            for k in ("ds_ln_g", "ds_ln_b", "ds_w", "ds_b"):
                assert (sa[k] is None and sb[k] is None) or torch.equal(sa[k], sb[k]), k
            assert len(sa["blocks"]) == len(sb["blocks"])
            for La, Lb in zip(sa["blocks"], sb["blocks"]):
                assert set(La) == set(Lb) and all(torch.equal(La[k], Lb[k]) for k in La)


def test_specs_and_config_reader():
    assert CW.SPECS["facebook/convnext-base-224"].hidden_sizes == (128, 256, 512, 1024)
    s = CW.SPECS["laion/CLIP-convnext_large_d_320.laion2B-s29B-b131K-ft-soup"]
    assert (s.hidden_sizes, s.image_size, s.grid(3), s.grid(4), s.width(4)) == ((192, 384, 768, 1536), 320, 20, 10, 1536)
    x = CW.SPECS["laion/CLIP-convnext_xxlarge-laion2B-s34B-b82K-augreg-soup"]
    assert (x.hidden_sizes, x.image_size, x.depths) == ((384, 768, 1536, 3072), 256, (3, 4, 30, 3))
    import transformers
    cfg = transformers.ConvNextConfig(hidden_sizes=[128, 256, 512, 1024], depths=[3, 3, 27, 3], layer_scale_init_value=0.0)
    got = CW.spec_from_hf_config(cfg, "b", crop_size=256)
    assert (got.image_size, got.layerscale, got.depths) == (256, False, (3, 3, 27, 3))
    with pytest.raises(ValueError, match="model_type"):
        CW.spec_from_hf_config(transformers.CLIPVisionConfig())


def test_device_layout_folds_the_norm_and_pads_to_128():
    spec = CW.tiny_spec(64, **CC.TINY)
    w = CW.synthetic_weights(spec, seed=3)
    D = CW.device_layout(spec, w)
    assert D["stem_w"].shape == (128, 64) and D["stem_w"].dtype == torch.bfloat16 and not D["stem_w"][64:].any() and not D["stem_w"][:, 48:].any()
    st = D["stages"][2]
    assert st["ds_w"].shape == (256, 4 * 128) and not st["ds_w"][192:].any() and not st["ds_b"][192:].any()
    L, L0 = st["blocks"][1], w["stages"][2]["blocks"][1]
    assert L["w1"].shape == (768, 192) and L["w2"].shape == (256, 768) and L["ls"].shape == (256,) and not L["w2"][192:].any() and not L["ls"][192:].any()
    assert torch.equal(L["s1"], L["w1"].float().sum(1))
    # Linear(LayerNorm(y)) restated from the folded arrays: rstd (y Wf^T - mean s) + b'
    y = torch.randn(5, 192, generator=torch.Generator().manual_seed(0)) * 3 + 1
    mean, rstd = y.mean(1, keepdim=True), (y.var(1, unbiased=False, keepdim=True) + spec.eps).rsqrt()
    got = rstd * (y @ L["w1"].float().t() - mean * L["s1"]) + L["b1"]
    want = torch.nn.functional.layer_norm(y, (192,), L0["ln_g"], L0["ln_b"], spec.eps) @ L0["w1"].t() + L0["b1"]
    assert CC.rel(got, want) < 1e-2                                   # bf16 weights: 2^-9 per entry


def test_hostile_weights_plant_what_they_say():
    spec = CW.tiny_spec(64, depths=(2, 1, 2, 1), hidden_sizes=(64, 128, 192, 256))
    base = CW.synthetic_weights(spec, seed=4)
    w = CW.hostile_weights(spec, seed=4, profile="all")
    ch = w["hostile"]["channels"][0]
    assert len(ch) == 4 and sorted(w["hostile"]["channels"]) == [0, 2]
    r = (w["stages"][0]["blocks"][0]["w2"][ch].norm(dim=1) / base["stages"][0]["blocks"][0]["w2"][ch].norm(dim=1))
    assert (r >= 49.9).all() and (r <= 200.1).all()
    assert sorted(w["stages"][0]["blocks"][1]["ln_g"][ch].tolist()) == pytest.approx([0.02, 0.02, 3.0, 3.0])
    ls = torch.cat([L["ls"].abs() for st in w["stages"] for L in st["blocks"]])
    assert ls.min() >= 1e-5 * 0.999 and ls.max() <= 1.0 and (ls < 1e-3).any() and (ls > 0.3).any()
    assert torch.allclose(w["stages"][1]["blocks"][0]["dw_b"], base["stages"][1]["blocks"][0]["dw_b"] + 25.0)
    with pytest.raises(ValueError, match="profile"):
        CW.hostile_weights(spec, profile="nope")


# ------------------------------------------------------------------------------------------------ 2. host twins against float64
HOST_DW_CASES = tuple(c for c in CC.DW_CASES if c[3] <= 192)             # the 3072-channel map is the GPU test's; the twin has no width-dependent path


@pytest.mark.parametrize("case", HOST_DW_CASES, ids=str)
def test_dwconv_twin_against_float64(case):
    x, wt, bias = CC.dw_input(case)
    y, rt = engine.dwconv7x7_stats_cpu(x, wt, bias)
    frac = CC.dw_check_output(y, case)
    worst = CC.dw_check_rt(rt, y, case)
    print(f"[convnext] twin {case}: {frac:.2e} of the outputs on a rounding boundary, rt at {worst:.3f} of its bound")


def test_dwconv_twin_statistics_come_from_the_rounded_outputs():
    x, wt, bias = CC.rounded_stats_input()
    y, rt = engine.dwconv7x7_stats_cpu(x, wt, bias)
    CC.rounded_stats_check(y, rt)


def test_dwconv_twin_orientation_and_padding_columns():
    """Cross-correlation: an impulse at (cy, cx) with a distinct weight per tap puts tap (ky, kx) at output (cy - ky + 3, cx - kx + 3)."""
    C_, H, W = 64, 9, 11
    x = torch.zeros(1, H, W, C_ + 8, dtype=torch.bfloat16)
    x[0, 4, 5, :C_] = 1.0
    x[..., C_:] = float("nan")                                       # ldx padding columns are never read
    wt = (torch.arange(49, dtype=torch.float32)[:, None] + 1).repeat(1, C_) * (1 + torch.arange(C_) % 2)
    y, rt = engine.dwconv7x7_stats_cpu(x, wt, torch.zeros(C_), C=C_)
    assert torch.isfinite(y.float()).all() and torch.isfinite(rt).all()
    for ky in range(7):
        for kx in range(7):
            assert torch.equal(y[0, 4 - ky + 3, 5 - kx + 3].float(), wt[ky * 7 + kx]), (ky, kx)
    assert y[0, 0, 0].abs().sum() == 0


@pytest.mark.parametrize("case", CC.S2D_CASES, ids=str)
def test_space_to_depth_twin_against_float64(case):
    x, g, b = CC.s2d_input(case)
    out = engine.ln_space_to_depth2_cpu(x, g, b)
    assert out.shape == (case[0] * case[1] * case[2] // 4, 4 * case[3])
    CC.s2d_check(out, x, g, b)


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals():
    with pytest.raises(ValueError, match="convnext-tiny"):
        CW.ConvNextSpec("t", 224, (3, 3, 9, 3), (96, 192, 384, 768))
    with pytest.raises(ValueError, match="multiple of 32"):
        CW.tiny_spec(72)
    with pytest.raises(ValueError, match="multiple of 32"):
        CW.SPECS["facebook/convnext-base-224"].at_resolution(230)
    spec = CW.tiny_spec(64)
    w = CW.synthetic_weights(spec)
    with pytest.raises(ValueError, match="bf16 only"):
        engine.make_convnext_engine(spec, w, None, "fp32")
    with pytest.raises(ValueError, match="no host engine"):
        engine.make_convnext_engine(spec, w, "cpu")
    lib = _lib.load()
    buf = (C.c_char * 65536)()
    p = C.addressof(buf) // 16 * 16 + 16
    q = p + 32768
    _lib.routes(reset=True)
    # odd H at a downsample, odd W, narrow ldo, aliasing
    for args, msg in (((p, 64, p, p, q, 256, 1, 3, 4, 64), "even"), ((p, 64, p, p, q, 256, 1, 4, 5, 64), "even"), ((p, 64, p, p, q, 128, 1, 4, 4, 64), "4 C"),
                      ((p, 64, p, p, p, 256, 1, 4, 4, 64), "alias"), ((p, 64, p, p, q, 256, 1, 4, 4, 60), "multiple of 8")):
        assert lib.visrep_ln_space_to_depth2(*args, 1e-6, None) < 0 and msg in _lib.last_error(), (args, _lib.last_error())
        assert lib.visrep_ln_space_to_depth2_cpu(*args, 1e-6, 1) < 0 and msg in _lib.last_error(), (args, _lib.last_error())
    for args, rc, msg in (((p, 96, p, p, q, 96, q, q, 1, 4, 4, 96), -2, "multiple of 64"), ((p, 64, p, p, q, 64, q, q, 1, 0, 4, 64), -2, "H >= 1"),
                          ((p, 56, p, p, q, 64, q, q, 1, 4, 4, 64), -2, ">= C"), ((p, 64, p, p, p, 64, q, q, 1, 4, 4, 64), -1, "alias"),
                          ((p + 8, 64, p, p, q, 64, q, q, 1, 4, 4, 64), -1, "aligned"), ((None, 64, p, p, q, 64, q, q, 1, 4, 4, 64), -1, "null")):
        assert lib.visrep_dwconv7x7_stats(*args, 1e-6, None) == rc and msg in _lib.last_error(), (args, _lib.last_error())
    assert lib.visrep_dwconv7x7_stats_cpu(p, 96, p, p, q, 96, q, 1, 4, 4, 96, 1e-6, 1) == -2 and "multiple of 64" in _lib.last_error()
    cfg = _lib.ConvNextConfig(72, 64, (C.c_int * 4)(1, 1, 1, 1), (C.c_int * 4)(64, 128, 192, 256), 1e-6)
    assert lib.visrep_convnext_workspace_bytes(C.byref(cfg), 1) == 0 and "multiple of 32" in _lib.last_error()
    cfg = _lib.ConvNextConfig(64, 64, (C.c_int * 4)(1, 1, 1, 1), (C.c_int * 4)(96, 192, 384, 768), 1e-6)
    assert lib.visrep_convnext_workspace_bytes(C.byref(cfg), 1) == 0 and "multiple of 64" in _lib.last_error()
    assert not any(_lib.routes(reset=True).values())                 # refused before any launch


def test_abi_covers_the_new_exports():
    for name in ("visrep_dwconv7x7_stats", "visrep_ln_space_to_depth2", "visrep_dwconv7x7_stats_cpu", "visrep_ln_space_to_depth2_cpu",
                 "visrep_convnext_workspace_bytes", "visrep_convnext_forward"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name), name
    assert _lib.CONVNEXT_ROUTES == ("dwconv_16", "dwconv_8", "dwconv_finalize", "ln_s2d")
    assert list(_lib.routes())[19:] == list(_lib.CONVNEXT_ROUTES)
    cfg = _lib.ConvNextConfig(64, 64, (C.c_int * 4)(1, 1, 2, 1), (C.c_int * 4)(64, 128, 192, 256), 1e-6)
    assert _lib.load().visrep_convnext_workspace_bytes(C.byref(cfg), 3) > 3 * 256 * 256 * 2


# ------------------------------------------------------------------------------------------------ 4. tower protocol
def tower_args(**kw):
    return SimpleNamespace(**{"mm_vision_select_layer": -2, "mm_vision_select_feature": "patch", "synthetic_weights": True, **kw})


def test_tower_protocol_properties():
    name = "laion/CLIP-convnext_large_d_320.laion2B-s29B-b131K-ft-soup"
    for layer, size, grid in ((-1, 1536, 10), (-2, 768, 20), (0, 192, 80), (1, 192, 80), (4, 1536, 10)):
        t = ConvNextVisionTower(name, tower_args(mm_vision_select_layer=layer), delay_load=True)
        assert not t.is_loaded and t.vision_tower_name == name and t.select_feature == "patch"
        assert (t.hidden_size, t.num_patches) == (size, grid * grid), layer
    t = builder.build_convnext_vision_tower(SimpleNamespace(mm_vision_tower=name, **vars(tower_args(vit_img_size=256))), delay_load=True)
    assert isinstance(t, ConvNextVisionTower) and (t.hidden_size, t.num_patches, t.config.image_size) == (768, 16 * 16, 256)
    with pytest.raises(ValueError, match="Unexpected select feature: cls_patch"):
        ConvNextVisionTower(name, tower_args(mm_vision_select_feature="cls_patch"), delay_load=True)
    with pytest.raises(ValueError, match="multiple of 32"):
        ConvNextVisionTower(name, tower_args(vit_img_size=250), delay_load=True)
    with pytest.raises(ValueError, match="five hidden states"):
        ConvNextVisionTower(name, tower_args(mm_vision_select_layer=5), delay_load=True)
    with pytest.raises(OSError, match="no built-in architecture"):
        ConvNextVisionTower("facebook/convnext-tiny-224", tower_args(), delay_load=True)


def test_checkpoint_directory_is_read(tmp_path):
    """A local HF ConvNeXt directory: config.json + safetensors + preprocessor_config.json drive spec, weights and the image processor."""
    import json
    from safetensors.torch import save_file
    spec = CW.tiny_spec(64, **CC.TINY)
    model = hf_model(spec, seed=5)
    model.config.save_pretrained(tmp_path)
    save_file({k: v.contiguous() for k, v in model.state_dict().items()}, str(tmp_path / "model.safetensors"))
    (tmp_path / "preprocessor_config.json").write_text(json.dumps({"crop_size": 96, "image_mean": [0.5, 0.5, 0.5], "image_std": [0.25, 0.25, 0.25]}))
    t = ConvNextVisionTower(str(tmp_path), tower_args(mm_vision_select_layer=-1), delay_load=True)
    assert (t.hidden_size, t.num_patches, t.config.image_size) == (256, 9, 96)
    proc = t._make_image_processor(t._retarget(t._spec(str(tmp_path))), str(tmp_path))
    assert proc.image_mean == [0.5, 0.5, 0.5] and proc.crop_size == {"height": 96, "width": 96}
    from PIL import Image
    assert proc.preprocess(Image.new("RGB", (120, 100)))["pixel_values"].shape == (1, 3, 96, 96)
    default = t._make_image_processor(spec, None)
    assert default.image_mean == pytest.approx([0.48145466, 0.4578275, 0.40821073])
