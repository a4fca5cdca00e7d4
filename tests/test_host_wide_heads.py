"""Towers whose heads are not 64 wide (SigLIP-so400m 16 x 72 / MLP 4304, ViT-H/14 16 x 80), host side: the bf16 engine's zero padding of
heads and MLP units (engine.pad_tower_weights) is exact, the packed layout agrees with the HF module at these shapes, and the host twin
takes them.  The GPU side is tests/test_gpu_wide_heads.py."""
import math
from dataclasses import replace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from law_of_vision_representation_in_mllms_amd import engine
from law_of_vision_representation_in_mllms_amd import vit_weights as VW
from oracle import vit as OV

SO400M = "google/siglip-so400m-patch14-384"
VITH = "laion/CLIP-ViT-H-14-laion2B-s32B-b79K"


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def small(name, side, layers=2):
    """The registry's shape at a small input (a few tokens) and depth."""
    return replace(VW.SPECS[name], image_size=side, layers=layers)


def test_registry_shapes():
    s, h = VW.SPECS[SO400M], VW.SPECS[VITH]
    assert (s.tokens, s.d // s.heads, s.mlp, s.has_cls, s.act, s.layers) == (729, 72, 4304, False, "gelu_tanh", 27)
    assert (h.tokens, h.d // h.heads, h.mlp, h.has_cls, h.pre_ln, h.act, h.layers) == (257, 80, 5120, True, True, "gelu", 32)
    assert [engine.head_pad_for(w) for w in (64, 65, 72, 80, 88, 96, 97, 128)] == [64, 96, 96, 96, 96, 96, 128, 128]
    for w in (32, 63, 129, 256):
        with pytest.raises(ValueError, match="head_dim"):
            engine.head_pad_for(w)


def padded_hidden_states(spec, w, px, dp, mp):
    """oracle/vit.py's forward with `heads x dp` semantics restated: the layers of `w` are PADDED (pad_tower_weights), the softmax scale is
    the TRUE width's.  Returns (hidden states, per-layer intermediates q, k, v, attention output, MLP hidden)."""
    d, H, p = spec.d, spec.heads, spec.patch
    da, scale = H * dp, 1.0 / math.sqrt(d // H)
    B = px.shape[0]
    t = F.conv2d(px, w["patch_w"].view(d, 3, p, p), w.get("patch_b"), stride=p).flatten(2).transpose(1, 2)
    if w.get("cls") is not None:
        t = torch.cat([w["cls"].view(1, 1, d).expand(B, 1, d), t], 1)
    t = t + w["pos"][None]
    if w.get("pre_ln_g") is not None:
        t = F.layer_norm(t, (d,), w["pre_ln_g"], w["pre_ln_b"], spec.eps)
    hs, inter = [t], []
    for L in w["layers"]:
        assert L["wqkv"].shape == (3 * da, d) and L["wo"].shape == (d, da) and L["w1"].shape == (mp, d) and L["w2"].shape == (d, mp)
        h = F.layer_norm(t, (d,), L["ln1_g"], L["ln1_b"], spec.eps)
        q, k, v = F.linear(h, L["wqkv"], L["bqkv"]).split(da, -1)
        T = q.shape[1]
        q, k, v = (x.view(B, T, H, dp).transpose(1, 2) for x in (q, k, v))
        a = torch.softmax(q @ k.transpose(-1, -2) * scale, -1)
        o = (a @ v).transpose(1, 2).reshape(B, T, da)
        t = t + F.linear(o, L["wo"], L["bo"])
        m = OV._act(F.linear(F.layer_norm(t, (d,), L["ln2_g"], L["ln2_b"], spec.eps), L["w1"], L["b1"]), spec.act)
        t = t + F.linear(m, L["w2"], L["b2"])
        hs.append(t)
        inter.append({"q": q, "k": k, "v": v, "o": o.view(B, T, H, dp), "m": m})
    return hs, inter


@pytest.mark.parametrize("name,dp", [(SO400M, 96), (SO400M, 128), (VITH, 96), (VITH, 128)])
def test_padding_is_exact(name, dp):
    """Zero rows / columns change nothing: the padded weight set under heads x dp semantics gives the unpadded oracle's hidden states to
    fp32 summation order, unpadding by slicing gives the original matrices back bit for bit, and the padded lanes of every intermediate
    (q, k, v, the attention output, the MLP's hidden units) are exactly 0."""
    spec = small(name, 42)                                                    # 3 x 3 patches
    w = VW.synthetic_weights(spec, seed=4)
    dh, H, m = spec.d // spec.heads, spec.heads, spec.mlp
    mp = (m + 127) // 128 * 128
    wp = dict(w)
    wp["layers"] = [engine.pad_tower_weights(spec, L, dp, mp) for L in w["layers"]]
    for L, P in zip(w["layers"], wp["layers"]):
        assert torch.equal(P["wqkv"].view(3, H, dp, spec.d)[:, :, :dh].reshape(3 * spec.d, spec.d), L["wqkv"])
        assert torch.equal(P["bqkv"].view(3, H, dp)[:, :, :dh].reshape(-1), L["bqkv"])
        assert torch.equal(P["wo"].view(spec.d, H, dp)[:, :, :dh].reshape(spec.d, spec.d), L["wo"])
        assert torch.equal(P["w1"][:m], L["w1"]) and torch.equal(P["b1"][:m], L["b1"]) and torch.equal(P["w2"][:, :m], L["w2"])
        assert not P["wqkv"].view(3, H, dp, spec.d)[:, :, dh:].any() and not P["wo"].view(spec.d, H, dp)[:, :, dh:].any()
        assert not P["w1"][m:].any() and not P["b1"][m:].any() and not P["w2"][:, m:].any()
    px = torch.from_numpy(np.random.RandomState(5).standard_normal((2, 3, 42, 42)).astype(np.float32))
    want = OV.vit_hidden_states(spec, w, px)
    got, inter = padded_hidden_states(spec, wp, px, dp, mp)
    for a, b in zip(got, want):
        assert rel(a, b) < 1e-6
    for it in inter:
        for n in ("q", "k", "v", "o"):
            assert not it[n][..., dh:].any(), n
        assert not it["m"][..., m:].any()


def test_unpadded_towers_pass_through():
    spec = VW.tiny_spec("clip", d=128, heads=2, mlp=256)
    L = VW.synthetic_weights(spec, seed=1)["layers"][0]
    P = engine.pad_tower_weights(spec, L, 64, 256)
    assert all(P[k] is L[k] for k in L)


def test_hf_siglip_so400m_shape_agrees_with_the_packed_layout():
    """spec_from_hf_config on the so400m vision config (2 layers) gives 729 tokens and 72-wide heads, and pack_hf_state_dict of a randomly
    initialised HF model of that config through oracle/vit.py reproduces the HF model's hidden_states[-2]."""
    tf = pytest.importorskip("transformers")
    cfg = tf.SiglipVisionConfig(hidden_size=1152, num_attention_heads=16, intermediate_size=4304, image_size=384, patch_size=14,
                                num_hidden_layers=2)
    spec = VW.spec_from_hf_config(cfg, SO400M)
    assert spec.tokens == 729 and spec.d // spec.heads == 72 and spec.mlp == 4304 and not spec.has_cls and spec.act == "gelu_tanh"
    assert replace(VW.SPECS[SO400M], layers=2) == spec                        # the built-in entry is what the public config says
    torch.manual_seed(0)
    model = tf.SiglipVisionModel(cfg).eval()
    px = torch.randn(1, 3, 384, 384)
    with torch.no_grad():
        want = model(pixel_values=px, output_hidden_states=True).hidden_states[-2]
    w = VW.pack_hf_state_dict(model.state_dict(), spec)
    got = OV.vit_hidden_states(spec, w, px)[-2]
    assert got.shape == want.shape == (1, 729, 1152)
    assert rel(got, want) < 1e-5


@pytest.mark.parametrize("name,side", [(SO400M, 56), (VITH, 56), (SO400M, 48)])
def test_cpu_twin_takes_the_wide_head_shapes(name, side):
    """visrep_vit_forward_cpu on the full-width, 2-layer, 4 x 4-patch towers against the fp32 oracle, at the bar of test_host_cpu_twins;
    side 48 = 3 x 3 patches of 14 with 6 trailing pixels dropped, as Conv2d does and as so400m's 384 / 14 = 27 needs."""
    spec = small(name, side)
    w = VW.synthetic_weights(spec, seed=6)
    px = torch.from_numpy(np.random.RandomState(7).standard_normal((2, 3, side, side)).astype(np.float32))
    eng = engine.make_engine(spec, w, device="cpu")
    assert isinstance(eng, engine.VitEngineCPU)
    for n in (1, 2):
        got, want = eng.forward(px, n_layers=n), OV.vit_hidden_states(spec, w, px)[n]
        assert got.shape == want.shape
        assert (got - want).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item()), (n, (got - want).abs().max().item())
