"""SAM ViT towers without a GPU: spec reader, packer round trips for both key layouts, refusals, the host twins of the relative-position
kernels against float64, the rounding model of the attention scheme inside the derived bound, the pad-row rule restated from the reference
module, and the oracle trap (a freshly constructed SamVisionModel has zero weights: planted weights must make the tables matter)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _attention_cases as AC  # noqa: E402
import _sam_cases as SC  # noqa: E402

from law_of_vision_representation_in_mllms_amd import _lib, engine, sam_weights as SW  # noqa: E402

TINY = SC.tiny_spec()


def test_specs_and_config_reader():
    from transformers import SamConfig, SamVisionConfig
    b, l = SW.SPECS["facebook/sam-vit-base"], SW.SPECS["facebook/sam-vit-large"]
    assert (b.d, b.layers, b.heads, b.mlp, b.global_attn_indexes) == (768, 12, 12, 3072, (2, 5, 8, 11))
    assert (l.d, l.layers, l.heads, l.mlp, l.global_attn_indexes) == (1024, 24, 16, 4096, (5, 11, 17, 23))
    for s in (b, l):
        assert (s.image_size, s.patch, s.window, s.out_channels, s.grid, s.n_states) == (1024, 16, 14, 256, 64, s.layers + 2)
    got = SW.spec_from_hf_config(SamVisionConfig(), "facebook/sam-vit-base")
    assert got == b
    assert SW.spec_from_hf_config(SamConfig(), "facebook/sam-vit-base") == b
    assert SW.spec_from_hf_config(SW.hf_config(TINY), TINY.name) == TINY


def test_refusals_name_the_cause():
    from transformers import SamVisionConfig
    with pytest.raises(ValueError, match="64 wide"):
        SW.spec_from_hf_config(SamVisionConfig(hidden_size=1280, num_attention_heads=16, num_hidden_layers=32, global_attn_indexes=[7, 15, 23, 31]))
    with pytest.raises(ValueError, match="use_rel_pos"):
        SW.spec_from_hf_config(SamVisionConfig(use_rel_pos=False))
    with pytest.raises(ValueError, match="use_abs_pos"):
        SW.spec_from_hf_config(SamVisionConfig(use_abs_pos=False))
    with pytest.raises(ValueError, match="vit_img_size"):
        SW.spec_from_hf_config(SamVisionConfig(), vit_img_size=512)
    with pytest.raises(ValueError, match="bf16 only"):
        engine.make_sam_engine(TINY, {}, None, "fp32")
    with pytest.raises(ValueError, match="no host engine"):
        engine.SamEngine(TINY, {}, "cpu")


@pytest.mark.parametrize("prefix", ["vision_encoder.", ""], ids=["model", "bare"])
def test_pack_round_trip(prefix):
    w = SW.synthetic_weights(TINY, seed=3)
    sd = SW.to_hf_state_dict(TINY, w, prefix=prefix)
    if prefix:
        sd["prompt_encoder.no_mask_embed.weight"] = torch.zeros(1, 4)       # a SamModel checkpoint carries more than the encoder
    back = SW.pack_hf_state_dict(sd, TINY)
    for k in w:
        if k != "layers":
            assert torch.equal(back[k], w[k]), k
    for a, b in zip(back["layers"], w["layers"]):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_to_hf_state_dict_loads_and_the_tables_matter():
    """The oracle trap: SamVisionConfig.initializer_range is 1e-10, so a fresh module is the identity in every block and its tables have no
    effect; with the packed weights loaded, zeroing rel_pos_* moves the output by far more than bf16 error (2^-8)."""
    from transformers import SamVisionModel
    spec = SC.tiny_spec(image_size=112)
    px = SC.pixels_for(spec, 1, seed=2)
    fresh = SC.hf_states(SamVisionModel(SW.hf_config(spec)).eval(), px)
    assert SC.rel_err(fresh[-2], fresh[0]) < 1e-6, "a freshly constructed module no longer has (near) zero weights: the trap is gone"
    w = SW.synthetic_weights(spec, seed=1)
    ref = SC.hf_states(SC.hf_from_packed(spec, w), px)
    assert len(ref) == spec.n_states and ref[-1].shape == (1, spec.grid ** 2, spec.out_channels) and ref[-2].shape == (1, spec.grid ** 2, spec.d)
    assert SC.rel_err(ref[1], ref[0]) > 0.05
    norel = SC.hf_states(SC.hf_from_packed(spec, SC.zero_rel(w)), px)
    e = [SC.rel_err(a, b) for a, b in zip(norel, ref)]
    print(f"[sam] zeroed rel_pos: relative change per state {['%.3f' % v for v in e]}")
    assert e[0] == 0.0 and min(e[1:]) > 10 * 2.0 ** -8


def test_hostile_weights_plant_what_they_claim():
    """A qkv bias of several units, massive-activation channels, and - measured on the oracle's own activations of one hostile layer - a
    position term that exceeds scale q.k in some head."""
    spec = SC.tiny_spec(image_size=112)
    hw = SW.hostile_weights(spec, seed=1)
    assert max(float(L["bqkv"].abs().max()) for L in hw["layers"]) >= 4.0 and hw["hostile"]["channels"]
    l = hw["hostile"]["rel_layers"][0]
    assert l not in spec.global_attn_indexes and spec.grid == spec.window           # one unpadded window: the map is the grid
    m = SC.hf_from_packed(spec, hw)
    px = SC.pixels_for(spec, 1, seed=2)
    with torch.no_grad():
        enc = m.vision_encoder
        x = enc.patch_embed(px) + enc.pos_embed
        for layer in enc.layers[:l]:
            x = layer(x)
            x = x[0] if isinstance(x, tuple) else x
        L, S, H, d = hw["layers"][l], spec.window, spec.heads, spec.d
        n = torch.nn.functional.layer_norm(x, (d,), L["ln1_g"], L["ln1_b"], spec.eps).reshape(-1, d)
        proj = n @ L["wqkv"].t() + L["bqkv"]
        q, k = (proj[:, i * d:(i + 1) * d].reshape(S * S, H, 64).permute(1, 0, 2) for i in range(2))
        idx = torch.arange(S)[:, None] - torch.arange(S)[None, :] + S - 1
        qg = q.reshape(H, S, S, 64)
        rel_h = torch.einsum("hywc,ykc->hywk", qg, L["rel_h"][idx]).reshape(H, S * S, S)
        rel_w = torch.einsum("hywc,wkc->hywk", qg, L["rel_w"][idx]).reshape(H, S * S, S)
        key = torch.arange(S * S)
        bias = rel_h[..., key // S] + rel_w[..., key % S]
        qk = 0.125 * q @ k.transpose(-1, -2)
    per_head = [(float(bias[h].abs().max()), float(qk[h].abs().max())) for h in range(H)]
    print(f"[sam] hostile layer {l}: (max |bias|, max |scale q.k|) per head {per_head}")
    assert any(b > s for b, s in per_head) and max(b for b, _ in per_head) > 10.0


def test_wrong_length_rel_pos_table_is_refused():
    spec = SC.tiny_spec(image_size=112)
    sd = SW.to_hf_state_dict(spec, SW.synthetic_weights(spec, seed=3))
    sd["vision_encoder.layers.0.attn.rel_pos_h"] = torch.zeros(2 * 7 - 1, 64)
    with pytest.raises(ValueError, match="another length"):
        SW.pack_hf_state_dict(sd, spec)


def test_pad_rows_are_the_raw_bias():
    """The rule the engine implements, restated from SamVisionLayer: the map is zero-padded AFTER layer_norm1 and BEFORE qkv, so a pad token's
    Q | K | V is the raw qkv bias, it is a key like any other, and window_unpartition drops the pad queries.  One layer, g = 20, window 14."""
    spec = SC.tiny_spec(layers=1, global_attn_indexes=())
    w = SW.synthetic_weights(spec, seed=5)
    layer = SC.hf_from_packed(spec, w).vision_encoder.layers[0]
    g, wd, d, H = spec.grid, spec.window, spec.d, spec.heads
    x = torch.from_numpy(np.random.RandomState(0).standard_normal((2, g, g, d)).astype(np.float32))
    with torch.no_grad():
        want = layer(x)
        want = want[0] if isinstance(want, tuple) else want
        L = w["layers"][0]
        n = torch.nn.functional.layer_norm(x, (d,), L["ln1_g"], L["ln1_b"], spec.eps).reshape(-1, d)
        proj = n @ L["wqkv"].t() + L["bqkv"]                                  # the UNPADDED tokens
        src = torch.from_numpy(SC.window_rows(2, g, wd))
        win = torch.where(src[:, None] >= 0, proj[src.clamp(min=0)], L["bqkv"][None])   # pad rows = the raw bias
        NB, T = win.shape[0] // (wd * wd), wd * wd
        q, k, v = (win[:, i * d:(i + 1) * d].reshape(NB, T, H, 64).permute(0, 2, 1, 3) for i in range(3))
        idx = torch.arange(wd)[:, None] - torch.arange(wd)[None, :] + wd - 1
        qg = q.reshape(NB, H, wd, wd, 64)
        rel_h = torch.einsum("bhywc,ykc->bhywk", qg, L["rel_h"][idx]).reshape(NB, H, T, wd)
        rel_w = torch.einsum("bhywc,wkc->bhywk", qg, L["rel_w"][idx]).reshape(NB, H, T, wd)
        key = torch.arange(T)
        logits = 0.125 * q @ k.transpose(-1, -2) + rel_h[..., key // wd] + rel_w[..., key % wd]
        o = (logits.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(NB * T, d)
        rows = torch.full((2 * g * g,), -1, dtype=torch.long)
        rows[src[src >= 0]] = torch.arange(len(src))[src >= 0]
        y = x.reshape(-1, d) + o[rows] @ L["wo"].t() + L["bo"]
        y = y + torch.nn.functional.gelu(torch.nn.functional.layer_norm(y, (d,), L["ln2_g"], L["ln2_b"], spec.eps) @ L["w1"].t() + L["b1"]) @ L["w2"].t() + L["b2"]
    assert (src < 0).sum() == 2 * (4 * 196 - 400)
    assert SC.rel_err(y.reshape(2, g, g, d), want) < 1e-5
    # and the two shortcuts the issue warns about are visibly wrong: the folded bias b + W beta in the pad rows
    Lh = SW.hostile_weights(spec, seed=5)["layers"][0]
    assert float((Lh["wqkv"] @ Lh["ln1_b"]).abs().max()) > 0.05


# ------------------------------------------------------------------------------------------------ twins, bound, rounding model
HOST_CASES = (SC.Case(2, 3, 1, seed=1), SC.Case(9, 3, 2, seed=2), SC.Case(14, 2, 1, seed=3), SC.BIAS30[1], SC.GROWTH[0], SC.GROWTH[1], SC.GROWTH[2])


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: c.id)
def test_rounding_model_and_twin_inside_the_bound(case):
    inp = SC.make_inputs(case)
    O, A, L = SC.oracle(inp, case)
    r = SC.ratio(SC.rounding_model(inp, case), O, A, L)
    M, HD = case.NB * case.T, case.H * 64
    f = lambda n: torch.from_numpy(inp[n].reshape(M, HD).astype(np.float32)).contiguous()
    q, k, v = f("q"), f("k"), f("v")
    rh, rw = (torch.from_numpy(inp[n].astype(np.float32)).contiguous() for n in ("rel_h", "rel_w"))
    out = torch.empty(M, HD)
    rc = _lib.load().visrep_mhsa_relpos_cpu(_lib.ptr(q), HD, _lib.ptr(k), HD, _lib.ptr(v), HD, _lib.ptr(rh), _lib.ptr(rw), _lib.ptr(out), HD, case.NB,
                                            case.S, case.H, 64, 0.125, 0)
    assert rc == 0, _lib.last_error()
    rt = SC.ratio(out.double().numpy().reshape(O.shape), O, A, L)
    print(f"[sam] {case.id}: rounding model at {r:.3f} of the bound, host twin at {rt:.3f} (L = {L:.1f})")
    assert r <= 1.0 and rt <= 1.0


@pytest.mark.parametrize("case", SC.GRID + (SC.GLOBAL,) + SC.BIAS30 + SC.GROWTH, ids=lambda c: c.id)
def test_cases_keep_their_components_within_twice_L(case):
    """The precondition of the bound's constant, from the inputs alone (tests/_sam_cases.py)."""
    L, Lc = SC.components(SC.make_inputs(case), case)
    assert Lc <= 2.0 * L, (case.id, L, Lc)


def test_growth_cases_straddle_the_threshold():
    for case in SC.GROWTH[:2]:
        E = SC.exponents(SC.make_inputs(case), case, 0)[0]
        tmax = np.stack([E[:, sl].max(1) for sl in SC.key_tiles(case, 0)], 1)
        steps = np.diff(tmax, axis=1)
        assert (steps > SC.THR).all() if case.param[0] > SC.THR else ((steps < SC.THR).all() and (steps > SC.THR - 1.5).all()), case.id
    inp, case = SC.make_inputs(SC.BIAS30[0]), SC.BIAS30[0]
    b = SC.bias_full(inp, case, 0)
    assert 20 < np.abs(b).max() <= 30 and np.abs(SC.exponents(inp, case, 0) / SC.LOG2E - b).max() < 8


@pytest.mark.parametrize("S", [9, 14, 64])
def test_tables_twin_against_float64(S):
    NB, H = (1, 1) if S == 64 else (3, 2)
    rs = np.random.RandomState(S)
    ld = 2 * H * 64 + 24
    q = AC.bf16_round(rs.standard_normal((NB * S * S, H * 64)))
    buf = np.full((NB * S * S, ld), AC.NAN_BITS, dtype=np.uint16)
    buf[:, :H * 64] = AC.bf16_bits(q)
    qk = torch.from_numpy(buf.view(np.int16)).view(torch.bfloat16)
    Rh, Rw = (torch.from_numpy(rs.standard_normal((2 * S - 1, 64)).astype(np.float32)) for _ in range(2))
    rel_h, rel_w = engine.relpos_tables(qk, Rh, Rw, NB, S, H)
    wh, ww, bh, bw = SC.tables_oracle(q, Rh.double().numpy(), Rw.double().numpy(), NB, S, H)
    assert np.all(np.abs(rel_h.double().numpy() - wh) <= bh) and np.all(np.abs(rel_w.double().numpy() - ww) <= bw)
    # orientation against the reference's own get_rel_pos indexing
    qi, kh = 5 * S + 2, 3
    assert abs(float(rel_h[0, 0, qi, kh]) - float(q[qi, :64] @ Rh.double().numpy()[5 - kh + S - 1])) <= bh[0, 0, qi, kh]
    assert abs(float(rel_w[0, 0, qi, kh]) - float(q[qi, :64] @ Rw.double().numpy()[2 - kh + S - 1])) <= bw[0, 0, qi, kh]


def test_index_cases_are_what_they_claim():
    for S in (9, 14):
        for mode in ("h", "w", "hw"):
            inp, want = SC.index_case(S, mode)
            case = SC.Case(S, 1, 1)
            O, _, _ = SC.oracle(inp, case)
            assert np.abs(O[0, :, 0] - want).max() < 1e-12, (S, mode)


def test_abi_additions_only():
    lib = _lib.load()
    assert lib.visrep_version() == 650 and _lib.SAM_ROUTES == ("attn_relpos", "relpos_tables", "sam_partition", "sam_neck")
    assert list(_lib.sam_routes()) == list(_lib.SAM_ROUTES) and len(_lib.routes()) == 23
    for n in ("visrep_mhsa_relpos_fwd", "visrep_relpos_tables", "visrep_sam_window_partition", "visrep_sam_window_unpartition", "visrep_mhsa_relpos_cpu",
              "visrep_relpos_tables_cpu", "visrep_sam_forward", "visrep_sam_workspace_bytes"):
        assert hasattr(lib, n), n


def test_plugin_refusals_without_a_gpu():
    from types import SimpleNamespace
    from law_of_vision_representation_in_mllms_amd.llava.model.multimodal_encoder import builder
    args = dict(mm_vision_tower="facebook/sam-vit-base", mm_vision_select_layer=-1, synthetic_weights=True)
    with pytest.raises(ValueError, match="Unexpected select feature"):
        builder.build_sam_vision_tower(SimpleNamespace(**args, mm_vision_select_feature="cls_patch"), delay_load=True)
    with pytest.raises(ValueError, match="vit_img_size"):
        builder.build_sam_vision_tower(SimpleNamespace(**args, mm_vision_select_feature="patch", vit_img_size=512), delay_load=True)
    t = builder.build_sam_vision_tower(SimpleNamespace(**args, mm_vision_select_feature="patch"), delay_load=True)
    assert (t.hidden_size, t.num_patches) == (256, 4096)
    t = builder.build_sam_vision_tower(SimpleNamespace(**dict(args, mm_vision_select_layer=-2), mm_vision_select_feature="patch"), delay_load=True)
    assert (t.hidden_size, t.num_patches) == (768, 4096)
