"""SwiGLU-FFN towers (HF Dinov2SwiGLUFFN, facebook/dinov2-giant) on the host: spec and packing from a checkpoint directory, the padding and
the 16-row interleave of the gated GEMM, the host twin against a float64 restatement, the dispatcher's refusals (no device needed: they
happen before any launch) and the random streams of every other activation, which must not have moved."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _swiglu_cases as SC  # noqa: E402

from law_of_vision_representation_in_mllms_amd import _lib, engine  # noqa: E402
from law_of_vision_representation_in_mllms_amd import vit_weights as VW  # noqa: E402


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_checkpoint_directory_with_swiglu_ffn_runs_on_the_host_twin(tmp_path):
    """A tiny transformers Dinov2Model(use_swiglu_ffn=True) (d 128, 2 heads, mlp_ratio 4 -> hidden width 344: neither a multiple of 16 nor
    of 128) saved to a directory, loaded through DinoV2VisionTower on device "cpu" and compared with HF's own hidden_states[-2][:, 1:].
    fp32 against fp32: relative L2 below 1e-5, the bar tests/test_host_cpu_twins.py holds the host tower to against the reference towers.
    Before this feature the spec came out as act='gelu', mlp=512 and packing died with KeyError 'encoder.layer.0.mlp.fc1.weight'."""
    transformers = pytest.importorskip("transformers")
    from law_of_vision_representation_in_mllms_amd.llava.model.multimodal_encoder.dinov2_encoder import DinoV2VisionTower
    torch.manual_seed(5)
    cfg = transformers.Dinov2Config(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, mlp_ratio=4, image_size=70, patch_size=14,
                                    use_swiglu_ffn=True)
    model = transformers.Dinov2Model(cfg).eval()
    with torch.no_grad():                                        # LayerScale away from its constant init, biases away from zero
        for n, prm in model.named_parameters():
            if "lambda1" in n or n.endswith(".bias"):
                prm.copy_(torch.randn_like(prm) * 0.3)
    path = str(tmp_path / "dinov2-swiglu")
    model.save_pretrained(path, safe_serialization=True)
    import json
    with open(os.path.join(path, "preprocessor_config.json"), "w") as fh:
        json.dump({"crop_size": {"height": 42, "width": 42}, "do_center_crop": True, "image_mean": [0.5, 0.5, 0.5], "image_std": [0.5, 0.5, 0.5]}, fh)
    tower = DinoV2VisionTower(path, SimpleNamespace(mm_vision_select_layer=-2, mm_vision_select_feature="patch", device="cpu"), delay_load=True)
    spec, w = tower._spec_and_weights()
    assert spec.act == "swiglu" and spec.mlp == 344 == VW.swiglu_hidden(128, 4) and spec.fc1_rows == 688
    assert w["layers"][0]["w1"].shape == (688, 128) and w["layers"][0]["b1"].shape == (688,) and w["layers"][0]["w2"].shape == (128, 344)
    assert torch.equal(w["layers"][1]["w1"], model.state_dict()["encoder.layer.1.mlp.weights_in.weight"])
    tower.load_model()
    assert tower.hidden_size == 128
    px = torch.randn(2, 3, 42, 42, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        want = model(px, output_hidden_states=True).hidden_states[-2][:, 1:]
    got = tower(px)
    assert got.shape == want.shape
    e = rel(got, want)
    print("host twin vs HF Dinov2SwiGLUFFN tower: rel L2", e)
    assert e < 1e-5
    # and the restatement the GPU tests lean on is HF's arithmetic
    assert rel(SC.swiglu_hidden_states(spec, w, px, n_layers=2)[2][:, 1:], want) < 1e-5


def test_registry_entry_and_hidden_width():
    g = VW.SPECS["facebook/dinov2-giant"]
    assert (g.image_size, g.patch, g.d, g.layers, g.heads, g.mlp, g.act, g.eps, g.layerscale, g.pos_grid, g.family) == \
        (224, 14, 1536, 40, 24, 4096, "swiglu", 1e-6, True, 37, "dinov2")
    assert VW.swiglu_hidden(1536, 4) == 4096 and g.fc1_rows == 8192 and g.d // g.heads == 64
    assert _lib.ACT["swiglu"] == 4 and _lib.EPI_GATED == 7


def test_interleave_is_a_permutation_the_gate_commutes_with():
    """silu(g) * u computed on HF chunk order, and on the interleaved columns with the kernel's pairing (32 t + r, 32 t + 16 + r) -> 16 t + r:
    bitwise the same fp32 values; the inverse permutation restores the input exactly."""
    g = torch.Generator().manual_seed(1)
    for mp in (128, 384, 4096):
        idx = engine.swiglu_interleave_index(mp)
        assert sorted(idx.tolist()) == list(range(2 * mp))
        x = torch.randn(5, 2 * mp, generator=g)
        xi = x[:, idx]
        back = torch.empty_like(x)
        back[:, idx] = xi
        assert torch.equal(back, x)
        s = torch.nn.functional.silu(x)                          # one evaluation per element (libm's vector and scalar paths may differ in the last bit)
        want = s[:, :mp] * x[:, mp:]
        sb, xb = s[:, idx].reshape(5, mp // 16, 2, 16), xi.reshape(5, mp // 16, 2, 16)
        got = (sb[:, :, 0] * xb[:, :, 1]).reshape(5, mp)          # the kernel's pairing: block 2 t holds gates, block 2 t + 1 their values
        assert torch.equal(got, want)
        t = torch.arange(2 * mp)[idx]                           # GEMM row 32 t + r = gate of unit 16 t + r; 32 t + 16 + r = its value row
        assert t[32 * 3 + 5] == 16 * 3 + 5 and t[32 * 3 + 16 + 5] == mp + 16 * 3 + 5
    with pytest.raises(ValueError):
        engine.swiglu_interleave_index(344)


def test_padding_pads_each_half_with_exact_zeros():
    spec = SC.swiglu_tiny_spec()
    w = VW.synthetic_weights(spec, seed=2, n_layers=1)
    L = engine.pad_tower_weights(spec, w["layers"][0], 64, 384)
    assert L["w1"].shape == (768, 128) and L["b1"].shape == (768,) and L["w2"].shape == (128, 384)
    for half in (0, 1):
        assert torch.equal(L["w1"][half * 384: half * 384 + 344], w["layers"][0]["w1"][half * 344: (half + 1) * 344])
        assert torch.equal(L["b1"][half * 384: half * 384 + 344], w["layers"][0]["b1"][half * 344: (half + 1) * 344])
        assert L["w1"][half * 384 + 344: (half + 1) * 384].abs().max() == 0 and L["b1"][half * 384 + 344: (half + 1) * 384].abs().max() == 0
    assert torch.equal(L["w2"][:, :344], w["layers"][0]["w2"]) and L["w2"][:, 344:].abs().max() == 0
    # a non-gated spec pads exactly as before
    s2 = VW.tiny_spec("siglip", d=128, heads=2, mlp=200)
    L2 = engine.pad_tower_weights(s2, VW.synthetic_weights(s2, seed=2, n_layers=1)["layers"][0], 64, 256)
    assert L2["w1"].shape == (256, 128) and L2["w1"][200:].abs().max() == 0 and L2["b1"].shape == (256,)


# sha256 of the flattened synthetic_weights(spec, seed=1, n_layers=1) of the five reference-registry specs, computed on the parent commit
PARENT_DIGESTS = {
    "openai/clip-vit-large-patch14-336": "c93a667320ab2b754a82c722019f2819a262b326d30f540386f36f1e0658fb5d",
    "openai/clip-vit-large-patch14": "9aaa13150b29fd7b8a36c7ef170b3d571658de732a0ea39c2e52a503600a0ee6",
    "laion/CLIP-ViT-L-14-laion2B-s32B-b82K": "9aaa13150b29fd7b8a36c7ef170b3d571658de732a0ea39c2e52a503600a0ee6",
    "facebook/dinov2-large": "eeab3243a3e991aca652348558165a612d30b8627e033d1054f4eff59644b76b",
    "google/siglip-base-patch16-224": "3c5d8735f6f9989f8bf0d7f4cc83570e70764fd39823bb6e01e4cd4ca35b6aff",
}


@pytest.mark.parametrize("name", sorted(PARENT_DIGESTS))
def test_other_activations_keep_their_random_streams(name):
    assert SC.weights_digest(VW.synthetic_weights(VW.SPECS[name], seed=1, n_layers=1)) == PARENT_DIGESTS[name]


def test_swiglu_synthetic_and_hostile_weights_draw_the_doubled_fc1():
    spec = SC.swiglu_tiny_spec()
    for w in (VW.synthetic_weights(spec, seed=3, n_layers=2), VW.hostile_weights(spec, seed=3, n_layers=2, profile="all")):
        for L in w["layers"]:
            assert L["w1"].shape == (688, 128) and L["b1"].shape == (688,) and L["w2"].shape == (128, 344)


@pytest.mark.parametrize("hostile", [False, True])
def test_host_twin_matches_the_float64_restatement(hostile):
    spec = SC.swiglu_tiny_spec()
    w = VW.hostile_weights(spec, seed=4, profile="all") if hostile else VW.synthetic_weights(spec, seed=4)
    px = torch.randn(2, 3, 42, 42, generator=torch.Generator().manual_seed(7))
    eng = engine.make_engine(spec, w, device="cpu")
    assert isinstance(eng, engine.VitEngineCPU)
    for n in (1, 3):
        e = rel(eng.forward(px, n_layers=n), SC.swiglu_hidden_states(spec, w, px, n_layers=n)[n])
        print("host twin vs float64, layers", n, "hostile", hostile, ":", e)
        assert e < 1e-5


@pytest.mark.parametrize("which,text", [(1, "convolution"), (2, "row map"), (3, "row statistics"), (4, "GroupNorm")])
def test_dispatcher_refuses_the_gated_epilogue_in_combinations_it_does_not_serve(which, text):
    """conv / A row map / stat_rt / gn_partial together with EPI_GATED: an error code and a message, and no launch (the dispatcher's route
    counters do not move) - checked through visrep_debug_gated_refusal, which needs no device because nothing may be launched."""
    lib = _lib.load()
    _lib.routes(reset=True)
    rc = lib.visrep_debug_gated_refusal(which)
    assert rc == -1, (rc, _lib.last_error())
    assert "gated" in _lib.last_error() and text in _lib.last_error()
    assert sum(_lib.routes(reset=True).values()) == 0
    # shapes: mp must be a multiple of 64, C at least mp wide - refused before any device work as well
    assert lib.visrep_gemm_bf16_gated(8, 64, 8, 64, None, None, None, 8, 64, 16, 192, 64, None) == -2 and "gated" in _lib.last_error()
    assert lib.visrep_gemm_bf16_gated(8, 64, 8, 64, None, None, None, 8, 64, 16, 256, 64, None) == -2 and "ldc" in _lib.last_error()
    assert lib.visrep_gemm_bf16_gated(8, 64, 8, 64, None, 8, None, 8, 128, 16, 256, 64, None) == -1      # ln_rt without ln_s
