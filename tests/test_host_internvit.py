"""InternViT without a GPU: spec and packer against the real transformers.InternVLVisionModel, the host twin against its hidden states over
the matrix norm_type x use_qk_norm x attention_bias x head geometry, exactness of the bf16 packer's per-head padding of the QK-norm weights,
the softmax-constant fold into qn_g, the checkpoint-directory round trip through the plug-in tower, and the unchanged specs / synthetic
streams / packed dicts of every tower family from before.  Cases and oracles are in tests/_internvit_cases.py."""
import ctypes as C
import hashlib
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

transformers = pytest.importorskip("transformers")


# ------------------------------------------------------------------------------------------------ 1. spec and packer
def test_spec_and_packing_of_a_real_internvl_vision_model():
    model = IC.hf_model(seed=1, norm_type="rms_norm", qk=True, bias=False, heads=(2, 72))
    spec = VW.spec_from_hf_config(model.config, "tiny-internvit")
    assert (spec.family, spec.norm, spec.qk_norm, spec.d, spec.heads, spec.image_size, spec.patch, spec.tokens) == ("internvl", "rmsnorm", True, 144, 2, 28, 7, 17)
    assert spec.has_cls and spec.patch_bias and spec.layerscale and not spec.pre_ln and spec.act == "gelu" and spec.eps == pytest.approx(1e-6)
    w = VW.pack_hf_state_dict(model.state_dict(), spec)
    sd = model.state_dict()
    L = w["layers"][1]
    assert L["qn_g"].shape == L["kn_g"].shape == (144,)
    assert torch.equal(L["qn_g"], sd["encoder.layer.1.attention.q_norm.weight"]) and torch.equal(L["kn_g"], sd["encoder.layer.1.attention.k_norm.weight"])
    assert torch.equal(L["ls1"], sd["encoder.layer.1.lambda_1"]) and torch.equal(L["ls2"], sd["encoder.layer.1.lambda_2"])
    assert L["bqkv"].shape == (432,) and not L["bqkv"].any()                       # attention_bias = False packs zeros
    assert not L["ln1_b"].any() and not L["ln2_b"].any()                           # RMSNorm has no bias
    assert torch.equal(L["wqkv"][144:288], sd["encoder.layer.1.attention.k_proj.weight"])
    # the InternVL wrapper config resolves to its vision_config; use_mask_token only adds a parameter
    assert VW.spec_from_hf_config(transformers.InternVLConfig(vision_config=model.config.to_dict()), "tiny-internvit") == spec
    masked = IC.hf_model(seed=1, norm_type="rms_norm", qk=True, bias=False, heads=(2, 72), use_mask_token=True)
    assert VW.spec_from_hf_config(masked.config, "tiny-internvit") == spec
    assert sorted(VW.flatten(VW.pack_hf_state_dict(masked.state_dict(), spec))) == sorted(VW.flatten(w))
    ln = IC.hf_model(seed=2, norm_type="layer_norm", qk=False, bias=True, heads=(2, 64))
    s2 = VW.spec_from_hf_config(ln.config, "x")
    w2 = VW.pack_hf_state_dict(ln.state_dict(), s2)
    assert (s2.norm, s2.qk_norm) == ("layernorm", False) and "qn_g" not in w2["layers"][0]
    assert w2["layers"][0]["ln1_b"].any() and w2["layers"][0]["bqkv"].any()


def test_refused_configs():
    with pytest.raises(ValueError, match="non-square"):
        VW.spec_from_hf_config(transformers.InternVLVisionConfig(image_size=[28, 42], patch_size=[7, 7]))
    with pytest.raises(ValueError, match="non-square"):
        VW.spec_from_hf_config(transformers.InternVLVisionConfig(image_size=[28, 28], patch_size=[7, 14]))
    with pytest.raises(ValueError, match="use_absolute_position_embeddings"):
        VW.spec_from_hf_config(transformers.InternVLVisionConfig(use_absolute_position_embeddings=False))
    with pytest.raises(ValueError, match="pre-LayerNorm"):
        replace(VW.tiny_spec("clip"), norm="rmsnorm")
    with pytest.raises(ValueError, match="norm must be"):
        replace(VW.tiny_spec("clip"), norm="t5")


def test_registry_specs():
    a, b = VW.SPECS["OpenGVLab/InternViT-300M-448px-V2_5"], VW.SPECS["OpenGVLab/InternViT-6B-448px-V2_5"]
    assert (a.d, a.layers, a.heads, a.mlp, a.norm, a.qk_norm, a.tokens, a.layerscale) == (1024, 24, 16, 4096, "layernorm", False, 1025, True)
    assert (b.d, b.layers, b.heads, b.mlp, b.norm, b.qk_norm, b.tokens, b.d // b.heads) == (3200, 45, 25, 12800, "rmsnorm", True, 1025, 128)
    assert engine.mhsa_cls_supported(a.tokens) and engine.head_pad_for(128) == 128


# ------------------------------------------------------------------------------------------------ 2. host twin against transformers
@pytest.mark.parametrize("cell", IC.HOST_MATRIX, ids=[IC.matrix_id(c) for c in IC.HOST_MATRIX])
def test_host_twin_against_transformers(cell):
    norm, qk, bias, heads = cell
    model = IC.hf_model(seed=3 + IC.HOST_MATRIX.index(cell), norm_type=norm, qk=qk, bias=bias, heads=heads)
    spec = VW.spec_from_hf_config(model.config, "x")
    w = VW.pack_hf_state_dict(model.state_dict(), spec)
    px = torch.randn(2, 3, 28, 28, generator=torch.Generator().manual_seed(5))
    eng = engine.VitEngineCPU(spec, w)
    for k in range(4):
        e = IC.rel(eng.forward(px, n_layers=k), IC.hf_hidden(model, px, k))
        print(f"[internvit] host twin {IC.matrix_id(cell)} hidden_states[{k}]: {e:.3e}")
        assert e < 1e-5, (cell, k, e)


def test_block_norm_eps_is_not_the_qk_norm_eps():
    """q_norm / k_norm keep the RMSNorm class default 1e-6 whatever layer_norm_eps says."""
    model = IC.hf_model(seed=9, norm_type="rms_norm", qk=True, bias=True, heads=(2, 64), eps=1e-2)
    spec = VW.spec_from_hf_config(model.config, "x")
    px = torch.randn(2, 3, 28, 28, generator=torch.Generator().manual_seed(6)) * 0.05       # small activations: eps matters
    got = engine.VitEngineCPU(spec, VW.pack_hf_state_dict(model.state_dict(), spec)).forward(px, n_layers=3)
    assert IC.rel(got, IC.hf_hidden(model, px, 3)) < 1e-5


def test_resolution_change_matches_transformers_interpolation():
    model = IC.hf_model(seed=4, norm_type="rms_norm", qk=True, bias=False, heads=(2, 64))
    spec = VW.spec_from_hf_config(model.config, "x")
    s2, w2 = VW.weights_at_resolution(spec, VW.pack_hf_state_dict(model.state_dict(), spec), 42)
    want = model.embeddings.interpolate_pos_encoding(torch.zeros(1, 37, 128), 42, 42)[0]
    assert s2.tokens == 37 and float((w2["pos"] - want.detach()).abs().max()) <= 1e-5
    px = torch.randn(1, 3, 42, 42, generator=torch.Generator().manual_seed(7))
    assert IC.rel(engine.VitEngineCPU(s2, w2).forward(px, n_layers=3), IC.hf_hidden(model, px, 3)) < 1e-5


# ------------------------------------------------------------------------------------------------ 3. the bf16 packer's padding and scale fold
def host_qk_norm(qk, width, d_true, qg, kg):
    lib = _lib.load()
    buf = qk.clone().float().contiguous()
    qg, kg = qg.float().contiguous(), kg.float().contiguous()
    rc = lib.visrep_qk_rmsnorm_cpu(_lib.ptr(buf), buf.shape[1], width, d_true, _lib.ptr(qg), _lib.ptr(kg), buf.shape[0], _lib.QK_NORM_EPS, 1)
    assert rc == 0, _lib.last_error()
    return buf


@pytest.mark.parametrize("heads,hd,hp", [(2, 72, 96), (3, 80, 96), (2, 100, 128)])
def test_padded_qk_gains_with_the_true_divisor_are_exact(heads, hd, hp):
    spec = IC.internvit_tiny_spec(heads=(heads, hd))
    g = torch.Generator().manual_seed(hd)
    d = heads * hd
    qk = torch.randn(9, 2 * d, generator=g)
    qg, kg = torch.randn(d, generator=g), torch.randn(d, generator=g)
    plain = host_qk_norm(qk, d, d, qg, kg).reshape(9, 2, heads, hd)
    padded_in = torch.zeros(9, 2, heads, hp)
    padded_in[..., :hd] = qk.reshape(9, 2, heads, hd)
    pq, pk = engine.pad_qk_gain(spec, qg, hp), engine.pad_qk_gain(spec, kg, hp)
    assert pq.shape == (heads * hp,) and not pq.reshape(heads, hp)[:, hd:].any()
    padded = host_qk_norm(padded_in.reshape(9, -1), heads * hp, d, pq, pk).reshape(9, 2, heads, hp)
    assert torch.equal(padded[..., :hd], plain)                                       # bit for bit
    assert not padded[..., hd:].any()
    wrong = host_qk_norm(padded_in.reshape(9, -1), heads * hp, heads * hp, pq, pk).reshape(9, 2, heads, hp)
    assert not torch.equal(wrong[..., :hd], plain)                                    # the padded width as divisor is a different tower


def test_softmax_constant_in_qn_g_equals_scaling_q_after_the_norm():
    g = torch.Generator().manual_seed(3)
    d, c = 128, 64 ** -0.5 * 1.4426950408889634
    qk = torch.randn(11, 2 * d, generator=g)
    qg, kg = torch.randn(d, generator=g), torch.randn(d, generator=g)
    after = host_qk_norm(qk, d, d, qg, kg)
    after[:, :d] *= c
    folded = host_qk_norm(qk, d, d, qg * c, kg)
    assert torch.equal(folded[:, d:], after[:, d:])
    # (x rstd) is common; after = fl(fl(. g) c), folded = fl(. fl(g c)): two roundings of relative size u = 2^-24 on each side, 4 u apart at most
    assert float(((folded - after).abs() / after.abs().clamp_min(1e-30)).max()) <= 4 * 2.0 ** -24 * 1.01
    before = host_qk_norm(torch.cat([qk[:, :d] * c, qk[:, d:]], 1), d, d, qg, kg)        # the constant in the projection: the norm undoes it
    assert IC.rel(before[:, :d] * c, after[:, :d]) < 1e-4 and IC.rel(before[:, :d], after[:, :d]) > 0.5


def test_host_rmsnorm_twins_against_float64():
    lib = _lib.load()
    x, g = IC.rms_rows_input(5, 3200, seed=1)
    rstd, y = IC.rms_oracle(x, g)
    xt, gt = torch.from_numpy(x).float().contiguous(), torch.from_numpy(g)
    out, rt = torch.empty_like(xt), torch.empty(5, 2)
    assert lib.visrep_rmsnorm_cpu(_lib.ptr(xt), 3200, _lib.ptr(gt), _lib.ptr(out), 3200, 5, 3200, IC.EPS, 1) == 0
    assert lib.visrep_rmsnorm_stats_cpu(_lib.ptr(xt), 3200, _lib.ptr(rt), 5, 3200, IC.EPS, 1) == 0
    assert np.abs(out.double().numpy() - y).max() <= 4 * 2.0 ** -24 * np.abs(y).max()
    assert np.allclose(rt[:, 0].double().numpy(), rstd, rtol=2 * 2.0 ** -24, atol=0) and not rt[:, 1].any()
    assert rt[4, 0].item() == pytest.approx(1e3, rel=1e-6) and not out[4].any()       # the all-zero row: rstd = eps^-0.5, finite output


# ------------------------------------------------------------------------------------------------ 4. checkpoint directory -> tower
@pytest.mark.parametrize("wrap", [False, True], ids=["bare", "internvl"])
def test_checkpoint_directory_round_trip(tmp_path, wrap):
    from law_of_vision_representation_in_mllms_amd.llava.model.multimodal_encoder.builder import build_internvit_vision_tower
    model = IC.hf_model(seed=11, norm_type="rms_norm", qk=True, bias=False, heads=(2, 64))
    path = str(tmp_path / "internvit")
    IC.save_checkpoint(model, path, wrap=wrap)
    px = torch.randn(2, 3, 28, 28, generator=torch.Generator().manual_seed(8))
    for feature, rows in (("patch", 16), ("cls_patch", 17)):
        cfg = SimpleNamespace(mm_vision_tower=path, vision_tower=path, mm_vision_select_layer=-2, mm_vision_select_feature=feature, device="cpu",
                              tower_precision="fp32")
        tower = build_internvit_vision_tower(cfg)
        assert tower.spec.family == "internvl" and tower.spec.qk_norm and tower.num_patches == 16 and tower.hidden_size == 128
        got = tower(px)
        want = IC.hf_hidden(model, px, -2)
        assert got.shape == (2, rows, 128)
        assert IC.rel(got, want if feature == "cls_patch" else want[:, 1:]) < 1e-5


@pytest.mark.parametrize("prefix", ["model.", ""], ids=["model.vision_tower", "vision_tower"])
def test_internvl_checkpoint_language_model_is_never_packed(tmp_path, prefix, monkeypatch):
    """Both key layouts of an InternVL checkpoint: only the tower's tensors reach the packer (a bf16 language model is not cast to fp32 on the
    way), and a delay-loaded tower reports the vision_config's sizes as integers."""
    from law_of_vision_representation_in_mllms_amd.llava.model.multimodal_encoder.builder import build_internvit_vision_tower
    model = IC.hf_model(seed=12, norm_type="rms_norm", qk=True, bias=False, heads=(2, 64))
    path = str(tmp_path / "internvl")
    extra = {prefix + "language_model.layers.0.w": torch.zeros(4, 4, dtype=torch.bfloat16), prefix + "multi_modal_projector.linear_1.weight": torch.zeros(4, 4),
             "lm_head.weight": torch.zeros(4, 4, dtype=torch.bfloat16)}
    IC.save_checkpoint(model, path, wrap=True, prefix=prefix, extra=extra)
    seen = {}
    real = VW.pack_hf_state_dict
    monkeypatch.setattr(VW, "pack_hf_state_dict", lambda sd, spec: seen.update(keys=sorted(sd)) or real(sd, spec))
    cfg = SimpleNamespace(mm_vision_tower=path, vision_tower=path, mm_vision_select_layer=-2, mm_vision_select_feature="patch", device="cpu", tower_precision="fp32")
    tower = build_internvit_vision_tower(cfg)
    assert seen["keys"] and all(k.startswith(prefix + "vision_tower.") for k in seen["keys"]), seen["keys"][:3]
    px = torch.randn(2, 3, 28, 28, generator=torch.Generator().manual_seed(8))
    assert IC.rel(tower(px), IC.hf_hidden(model, px, -2)[:, 1:]) < 1e-5
    lazy = build_internvit_vision_tower(cfg, delay_load=True)
    assert not lazy.is_loaded and (lazy.hidden_size, lazy.num_patches, lazy.config.image_size, lazy.config.patch_size) == (128, 16, 28, 7)


# ------------------------------------------------------------------------------------------------ 5. old behaviour restated
def digest(w):
    h = hashlib.sha256()
    for k, v in sorted(VW.flatten(w).items()):
        h.update(k.encode() + v.detach().float().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


OLD_SPECS = {
    "openai/clip-vit-large-patch14-336": (336, 14, 1024, 24, 16, 4096, "quick_gelu", 1e-5, True, True, False, False, "clip", 0, 0),
    "google/siglip-so400m-patch14-384": (384, 14, 1152, 27, 16, 4304, "gelu_tanh", 1e-6, False, False, True, False, "siglip", 0, 0),
    "facebook/dinov2-giant": (224, 14, 1536, 40, 24, 4096, "swiglu", 1e-6, True, False, True, True, "dinov2", 37, 0),
    "facebook/dinov2-with-registers-large": (224, 14, 1024, 24, 16, 4096, "gelu", 1e-6, True, False, True, True, "dinov2", 37, 4),
}
# sha256 prefixes of the flattened dicts, recorded on the parent commit
OLD_STREAMS = {("clip", 0, "synthetic"): "462205424071577a", ("siglip", 0, "synthetic"): "7fad3fde44991058", ("dinov2", 0, "synthetic"): "09c574ca231e253f",
               ("dinov2", 4, "synthetic"): "71f64c6ced2687e8", ("clip", 0, "hostile"): "7e4f7ad35a865f31", ("dinov2", 4, "hostile"): "b35b0ed90d6c7718"}


def test_old_specs_are_unchanged():
    for name, t in OLD_SPECS.items():
        s = VW.SPECS[name]
        assert (s.image_size, s.patch, s.d, s.layers, s.heads, s.mlp, s.act, s.eps, s.has_cls, s.pre_ln, s.patch_bias, s.layerscale, s.family,
                s.pos_grid, s.registers) == t, name
        assert (s.norm, s.qk_norm) == ("layernorm", False)
    assert len(VW.SPECS) == 12


@pytest.mark.parametrize("key", sorted(OLD_STREAMS), ids=[f"{f}-r{r}-{k}" for f, r, k in sorted(OLD_STREAMS)])
def test_old_synthetic_streams_are_unchanged(key):
    family, reg, kind = key
    spec = VW.tiny_spec(family, registers=reg)
    w = VW.synthetic_weights(spec, seed=3) if kind == "synthetic" else VW.hostile_weights(spec, seed=3, profile="all")
    w.pop("hostile", None)
    assert all("qn_g" not in L and "kn_g" not in L for L in w["layers"])
    assert digest(w) == OLD_STREAMS[key], (key, digest(w))


def test_qk_norm_spec_keeps_the_old_stream_unless_gains_are_asked_for():
    spec = IC.internvit_tiny_spec("rmsnorm", True)
    plain, base = VW.synthetic_weights(spec, seed=3), VW.synthetic_weights(replace(spec, norm="layernorm", qk_norm=False), seed=3)
    assert digest(plain) == digest(base) and "qn_g" not in plain["layers"][0]
    gains = VW.synthetic_weights(spec, seed=3, qk_gains=True)
    assert all(L["qn_g"].shape == (128,) and L["kn_g"].shape == (128,) for L in gains["layers"])
    for L in gains["layers"]:
        L.pop("qn_g"), L.pop("kn_g")
    assert digest(gains) == digest(plain)                                           # drawn after everything else
    h = VW.hostile_weights(spec, seed=3, profile="all")
    for L in h["layers"]:
        for k in ("qn_g", "kn_g"):
            a = L[k].abs()
            assert 0.02 <= float(a.min()) and float(a.max()) <= 3.0 and 0.2 < float((L[k] < 0).float().mean()) < 0.8
    px = torch.randn(2, 3, 28, 28, generator=torch.Generator().manual_seed(1))      # absent gains = ones, on the engine and in the oracle
    assert IC.rel(engine.VitEngineCPU(spec, plain).forward(px, n_layers=3), IC.hf_hidden(IC.hf_from_packed(spec, plain), px, 3)) < 1e-5
    assert IC.rel(engine.VitEngineCPU(spec, h).forward(px, n_layers=3), IC.hf_hidden(IC.hf_from_packed(spec, h), px, 3)) < 1e-5


def test_old_packed_dicts_are_unchanged():
    """CLIP, SigLIP, DINOv2 and register towers from transformers modules: the keys of before, no QK-norm entries, the same tensors."""
    from transformers import CLIPVisionConfig, CLIPVisionModel, Dinov2WithRegistersConfig, Dinov2WithRegistersModel, SiglipVisionConfig, SiglipVisionModel
    torch.manual_seed(0)
    cases = [(CLIPVisionModel(CLIPVisionConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, image_size=28, patch_size=7)), None),
             (SiglipVisionModel(SiglipVisionConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, image_size=28, patch_size=7)), None),
             (Dinov2WithRegistersModel(Dinov2WithRegistersConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=2, image_size=28, patch_size=7,
                                                                 num_register_tokens=2)), 28)]
    keys = {"b1", "b2", "bo", "bqkv", "ln1_b", "ln1_g", "ln2_b", "ln2_g", "ls1", "ls2", "w1", "w2", "wo", "wqkv"}
    for model, crop in cases:
        spec = VW.spec_from_hf_config(model.config, "x", crop_size=crop)
        assert (spec.norm, spec.qk_norm) == ("layernorm", False)
        w = VW.pack_hf_state_dict(model.state_dict(), spec)
        assert set(w["layers"][0]) == keys and set(w) - {"reg"} == {"patch_w", "patch_b", "cls", "pos", "pos_native", "pre_ln_g", "pre_ln_b", "layers"}
        sd = {k.split(".", 1)[-1] if k.startswith(("vision_model.", "dinov2_with_registers.")) else k: v for k, v in model.state_dict().items()}
        q = [k for k in sd if k.endswith(("layers.1.self_attn.q_proj.weight", "layer.1.attention.attention.query.weight"))][0]
        assert torch.equal(w["layers"][1]["wqkv"][:64], sd[q])


# ------------------------------------------------------------------------------------------------ 6. ABI
def test_abi_covers_the_new_exports():
    for name in ("visrep_rmsnorm", "visrep_rmsnorm_stats", "visrep_qk_rmsnorm", "visrep_rmsnorm_f32", "visrep_qk_rmsnorm_f32", "visrep_rmsnorm_cpu",
                 "visrep_rmsnorm_stats_cpu", "visrep_qk_rmsnorm_cpu", "visrep_gemm_bf16_resid_rms_stats"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name), name
    assert [n for n, _ in _lib.VitConfig._fields_][-2:] == ["norm", "qk_norm"] and [n for n, _ in _lib.VitLayer._fields_][-2:] == ["qn_g", "kn_g"]
    assert _lib.ROUTES[14:] == ("stats_epilogue", "stats_reduce", "stats_rows", "rms", "qk_norm") and _lib.ABI_VERSION == 650
    assert C.sizeof(_lib.VitConfig) == 18 * 4 and C.sizeof(_lib.VitLayer) == 18 * C.sizeof(C.c_void_p)


def test_row_entry_points_refuse_before_any_launch():
    lib = _lib.load()
    buf = (C.c_char * 4096)()
    p = C.addressof(buf) // 16 * 16 + 16
    _lib.routes(reset=True)
    for args, msg in (((None, 64, p, p, 64, 1, 64), "null"), ((p, 64, p, p + 8, 64, 1, 64), "16-byte"), ((p, 64, p, p, 64, 1, 60), "d % 8"),
                      ((p, 4104, p, p, 4104, 1, 4104), "d <= 4096"), ((p, 68, p, p, 64, 1, 64), "% 8"), ((p, 56, p, p, 64, 1, 64), ">= d")):
        assert lib.visrep_rmsnorm(*args, 1e-6, None) < 0 and msg in _lib.last_error(), (args, _lib.last_error())
    for args, msg in (((p, 64, None, 1, 64), "null"), ((p + 8, 64, p, 1, 64), "aligned"), ((p, 64, p + 4, 1, 64), "aligned"), ((p, 64, p, 1, 4104), "d <= 4096")):
        assert lib.visrep_rmsnorm_stats(*args, 1e-6, None) < 0 and msg in _lib.last_error(), (args, _lib.last_error())
    for name, over, rc, msg in IC.QK_REFUSALS:
        assert lib.visrep_qk_rmsnorm(*IC.qk_refusal_args(over, p), None) == rc and msg in _lib.last_error(), (name, _lib.last_error())
    assert not any(_lib.routes(reset=True).values())
