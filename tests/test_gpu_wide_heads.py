"""ViT towers whose heads are not 64 wide on the bf16 engine (SigLIP-so400m 16 x 72 / MLP 4304, ViT-H/14 16 x 80, 16 x 88, 4 x 96): the
width-96 flash kernel (attn_fwd96, csrc/attention.hip) through the C ABI against the float64 oracle and the per-element bound of
tests/_attention_cases.py (`ratio = max |got - O| / bound <= 1`, no tolerance of its own), its isolation properties, its agreement with the
route it replaces (attn_fwd<2> on heads padded to 128), and the composed forward / packing / plug-in path above it against oracle/vit.py
under the rule of tests/test_gpu_fullsize.py.  `[wide-heads]` lines (pytest -s) carry the measured figures."""
import ctypes as C
import json
import os
import sys
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _attention_cases as AC  # noqa: E402

from law_of_vision_representation_in_mllms_amd import _lib, engine  # noqa: E402
from law_of_vision_representation_in_mllms_amd import vit_weights as VW  # noqa: E402
from oracle import vit as OV  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SO400M = "google/siglip-so400m-patch14-384"
VITH = "laion/CLIP-ViT-H-14-laion2B-s32B-b79K"


# ------------------------------------------------------------------------------------------------ kernel contract at width 96
class WCase(AC.Case):
    """A case of _attention_cases whose buffers are `pad` wide per head (96: attn_fwd96; 128: attn_fwd<2>) and whose true head width is
    param[0]: lanes [true, pad) of Q, K and V are zero, the softmax scale is true^-0.5.  _attention_cases.Case takes its width from a table
    keyed by route; everything else there (oracle, bound, packers, layouts) only reads case.D."""
    __slots__ = ()

    @property
    def D(self):
        return 96 if self.route == "d96" else 128

    @property
    def true(self):
        return self.param[0]

    @property
    def id(self):
        return f"{self.route}-w{self.true}-B{self.B}-Tq{self.Tq}-Tk{self.Tk}-H{self.H}" + "-shared" * self.shared + "-causal" * self.causal


COUNTER = {"d96": "attn_96", "d128": "attn"}


def make_inputs(case):
    rs = np.random.RandomState(3000 + case.seed)
    Bk = 1 if case.shared else case.B
    out = {}
    for n, shape in (("q", (case.B, case.Tq)), ("k", (Bk, case.Tk)), ("v", (Bk, case.Tk))):
        x = np.zeros(shape + (case.H, case.D))
        x[..., :case.true] = rs.standard_normal(shape + (case.H, case.true))
        out[n] = AC.bf16_round(x)
    out["scale"] = float(case.true) ** -0.5
    return out


def launch(case, packed, scale, finite=True):
    lib = _lib.require_gpu()
    t = {n: torch.from_numpy(a.view(np.int16).copy()).to(DEV) for n, (a, _) in packed["bufs"].items()}
    p = lambda n: C.c_void_p(t[n].data_ptr() + 2 * packed["bufs"][n][1])
    d = packed["dims"]
    torch.cuda.synchronize()
    _lib.routes(reset=True)
    rc = lib.visrep_attention_fwd(p("q"), d["ldq"], p("k"), d["ldk"], p("vt"), d["ldvt"], p("out"), d["ldo"], case.B, case.Tq, case.Tk,
                                  case.H, case.D, case.shared, case.causal, scale, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (case.id, _lib.last_error())
    r = _lib.routes(reset=True)
    assert {k: v for k, v in r.items() if v} == {COUNTER[case.route]: 1}, (case.id, r)
    bits = AC.out_window(t["out"].cpu().numpy().view(np.uint16), packed)
    if finite:
        assert AC.finite_bits(bits).all(), case.id
    return bits


def run(case, layout="tight", inp=None, hostile=True, edit=None, finite=True):
    inp = make_inputs(case) if inp is None else inp
    packed = AC.pack(inp, case, layout, hostile)
    if edit is not None:
        edit(packed)
    return launch(case, packed, inp["scale"], finite)


def values(bits, case):
    return AC.bf16_from_bits(bits).reshape(case.B, case.Tq, case.H, case.D)


TQ_OF = {1: 33, 3: 129, 63: 70, 64: 128, 65: 257, 729: 729}        # 729 = 5 * 128 + 89: a query tail of 89 rows (three waves)


def _contract_cases():
    out = []
    for i, (true, tk, sh, ca) in enumerate((w, t, s, c) for w in (72, 80, 96) for t in (1, 3, 63, 64, 65, 729) for s in (0, 1) for c in (0, 1)):
        B = 3 if tk == 729 else 5                                  # start residues b Tk % 64: 0 for every image at Tk = 64 and with shared
        out.append(WCase("d96", B, TQ_OF[tk], tk, 2, sh, ca, "rand", (true,), i))   # keys, non-zero otherwise (729: 0, 25, 50)
    return out


CONTRACT = _contract_cases()


def test_contract_cases_cover_what_they_claim():
    res = {(c.Tk, r) for c in CONTRACT if not c.shared for r in {b * c.Tk % 64 != 0 for b in range(c.B)}}
    assert {(64, False), (1, True), (3, True), (63, True), (65, True), (729, True), (729, False)} <= res
    assert {(c.true, c.Tk, c.shared, c.causal) for c in CONTRACT} == {(w, t, s, a) for w in (72, 80, 96) for t in TQ_OF for s in (0, 1) for a in (0, 1)}


@pytest.mark.parametrize("case", CONTRACT, ids=[c.id for c in CONTRACT])
def test_width_96_kernel_contract(case):
    """True widths 72 / 80 / 96, Tk in {1, 3, 63, 64, 65, 729}, kv_shared and causal on and off, key-tile start residues zero and non-zero,
    the 89-row query tail of 729, tight and windowed buffers (NaN around every window, NaN K rows behind the last key, +-3.4e38 V^T pads).
    The padded lanes of the oracle are exactly 0 and their bound is 0: the kernel must write exact zeros there."""
    inp = make_inputs(case)
    O, A, L = AC.oracle(inp, case)
    assert not O[..., case.true:].any()
    for lay in ("tight", AC.LAYOUTS[1 + case.seed % 3]):
        r = AC.ratio(values(run(case, lay, inp), case), O, A, L)
        print(f"[wide-heads] {case.id} {lay}: ratio {r:.3f} (L = {L:.1f})")
        assert r <= 1.0, (case.id, lay, r)


def test_neighbours_change_nothing():
    """Image 1's output is bitwise the same with its neighbours' Q, K, V scaled to 1e30 (they share its first and last key tile), and the
    whole output is bitwise the same with zero V^T pads and K ending at its last row."""
    case = WCase("d96", 4, 70, 77, 2, 0, 0, "rand", (72,), 90)
    inp = make_inputs(case)
    base = run(case, "window", inp)
    assert np.array_equal(base, run(case, "window", inp, hostile=False))
    loud = {n: inp[n].copy() for n in ("q", "k", "v")}
    for n in loud:
        for b in (0, 2, 3):
            loud[n][b] = AC.bf16_round(np.sign(loud[n][b]) * 1e30 * (1 + np.abs(loud[n][b])))
    loud["scale"] = inp["scale"]
    got = run(case, "window", loud, finite=False)
    assert np.array_equal(got.reshape(4, 70, -1)[1], base.reshape(4, 70, -1)[1])


@pytest.mark.parametrize("which", ["q", "k", "v", "qv", "kv"])
def test_garbage_in_padded_lanes_stays_in_padded_lanes(which):
    """Finite garbage in the padded lanes [72, 96) leaves the true lanes of the output bitwise unchanged (the padded OUTPUT lanes carry
    whatever V^T's padded rows hold: the packer gives the out-projection zero columns there).  Q and K are checked one at a time: a
    padded lane contributes q_pad * k_pad to the score, which is exactly 0 as soon as ONE factor is 0 - the packer zeroes both; garbage in
    both at once is a different attention problem, not an invariant."""
    case = WCase("d96", 3, 70, 77, 2, 0, 0, "rand", (72,), 91)
    inp = make_inputs(case)
    base = run(case, "tight", inp).reshape(-1, case.H, 96)
    rs = np.random.RandomState(92)
    bad = {n: inp[n].copy() for n in ("q", "k", "v")}
    for n in which:
        bad[n][..., 72:] = AC.bf16_round(rs.standard_normal(bad[n][..., 72:].shape) * 50.0)
    bad["scale"] = inp["scale"]
    got = run(case, "tight", bad).reshape(-1, case.H, 96)
    assert np.array_equal(got[..., :72], base[..., :72])
    assert ("v" in which) == bool(got[..., 72:].any())


def test_route_96_agrees_with_the_128_padded_route():
    """A true-72 head through attn_fwd96 and through attn_fwd<2> on buffers padded to 128: both hold the oracle's bound, so they differ by at
    most the sum of the two bounds (the same bound: same oracle, same true lanes)."""
    a = WCase("d96", 3, 729, 729, 2, 0, 0, "rand", (72,), 93)
    b = a._replace(route="d128")
    ia = make_inputs(a)
    ib = {n: np.concatenate([ia[n], np.zeros(ia[n].shape[:-1] + (32,))], -1) for n in ("q", "k", "v")}
    ib["scale"] = ia["scale"]
    O, A, L = AC.oracle(ia, a)
    ba, bb = run(a, "tight", ia), run(b, "tight", ib)
    va, vb = values(ba, a)[..., :72], values(bb, b)[..., :72]
    bnd = AC.bound(O, A, L)[..., :72]
    same = np.array_equal(ba.reshape(-1, 2, 96)[..., :72], bb.reshape(-1, 2, 128)[..., :72])
    print(f"[wide-heads] 96 route vs 128-padded route, true width 72, T = 729: bitwise equal = {same}, "
          f"max |a - b| / (2 bound) = {float((np.abs(va - vb) / (2 * bnd)).max()):.3f}")
    assert (np.abs(va - vb) <= 2 * bnd).all()
    assert not values(ba, a)[..., 72:].any() and not values(bb, b)[..., 72:].any()


def test_unsupported_widths_stay_refused():
    lib = _lib.require_gpu()
    buf = torch.full((1 << 16,), -1, dtype=torch.int16, device=DEV)
    p = buf.data_ptr()
    _lib.routes(reset=True)
    for hd in (72, 256):
        assert lib.visrep_attention_fwd(p, 512, p, 512, p, 128, p, 512, 1, 64, 64, 1, hd, 0, 0, 0.1, _lib.stream_ptr()) == AC.ERR_SHAPE
        assert "head_dim" in _lib.last_error()
        assert lib.visrep_mhsa_fwd(p, 1024, p, 128, p, 512, 1, 64, 1, hd, 0.1, _lib.stream_ptr()) == AC.ERR_SHAPE
        assert "head_dim" in _lib.last_error()
    assert lib.visrep_attention_fwd(p, 96, p, 96, p, 128, p, 96, 1, 64, 64, 1, 96, 0, 0, 0.0, _lib.stream_ptr()) == AC.ERR_ARG
    assert "pre-scaled Q" in _lib.last_error()
    torch.cuda.synchronize()
    assert not any(_lib.routes(reset=True).values()) and bool((buf == -1).all())


def test_mhsa_96_equals_attention_on_split_pointers():
    """visrep_mhsa_fwd(head_dim 96): K starts at column H * 96 of the Q | K buffer."""
    case = WCase("d96", 3, 77, 77, 2, 0, 0, "rand", (80,), 94)
    inp = make_inputs(case)
    HD = 2 * 96
    want = run(case, "tight", inp)
    qk = AC._window(np.concatenate([inp["q"].reshape(-1, HD), inp["k"].reshape(-1, HD)], 1), 2 * HD + 8, 0, 70)
    vt = AC.pack_vt(inp["v"].reshape(-1, HD), AC.round_up(3 * 77, 64))
    t = [torch.from_numpy(a.view(np.int16).copy()).to(DEV) for a in (qk, vt)]
    out = torch.empty(3 * 77, HD, dtype=torch.bfloat16, device=DEV)
    _lib.routes(reset=True)
    rc = _lib.require_gpu().visrep_mhsa_fwd(_lib.ptr(t[0]), 2 * HD + 8, _lib.ptr(t[1]), vt.shape[1], _lib.ptr(out), HD, 3, 77, 2, 96,
                                            inp["scale"], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    assert _lib.routes(reset=True)["attn_96"] == 1
    assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), want)


# ------------------------------------------------------------------------------------------------ towers
def bf(x):
    return x.to(torch.bfloat16)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


def fast_weights(spec, seed, n_layers):
    os.environ["VISREP_FAST_SYNTHETIC"] = "1"
    try:
        return VW.synthetic_weights(spec, seed=seed, n_layers=n_layers)
    finally:
        os.environ.pop("VISREP_FAST_SYNTHETIC", None)


TOWERS = {
    "so400m": VW.SPECS[SO400M],                                                                      # 16 x 72, MLP 4304 -> 4352, 729 tokens, no CLS
    "vit_h14": VW.SPECS[VITH],                                                                       # 16 x 80, CLS + pre-LN, 257 tokens
    "g88": VW.ViTSpec("16x88", 224, 14, 1408, 40, 16, 6144, "gelu", 1e-5, True, True, False, False, "clip"),        # ViT-g/14's widths
    "s96": VW.ViTSpec("4x96", 112, 14, 384, 12, 4, 1536, "gelu_tanh", 1e-6, False, False, True, False, "siglip"),   # a true-96 head, 64 tokens
}
PARITY = [(t, n) for t in ("so400m", "vit_h14") for n in (2, 3)] + [("g88", 2), ("s96", 2)]
_ORACLE = {}


def tower_case(tag, n_layers, n_img=2):
    """(spec, weights, pixels, fp32 oracle, error of the bf16 oracle) - computed once per (tower, depth), shared by the three engine modes."""
    key = (tag, n_layers, n_img)
    if key not in _ORACLE:
        spec = TOWERS[tag]
        w = fast_weights(spec, 3, n_layers)
        px = bf(torch.from_numpy(np.random.RandomState(11).standard_normal((n_img, 3, spec.image_size, spec.image_size)).astype(np.float32)))
        want = OV.vit_hidden_states(spec, w, px.float(), n_layers=n_layers)[n_layers]
        e_ref = rel(OV.vit_hidden_states(spec, w, px.float(), n_layers=n_layers, dtype=torch.bfloat16)[n_layers], want)
        _ORACLE[key] = (spec, w, px, want, e_ref)
    return _ORACLE[key]


@pytest.mark.parametrize("mode", ["fused", "unfused", "fallback"])
@pytest.mark.parametrize("tag,n_layers", PARITY, ids=[f"{t}-{n}" for t, n in PARITY])
def test_tower_parity(tag, n_layers, mode):
    """Each tower with its own activation and CLS setting at full width: LayerNorm folded into the GEMMs / not, and once on the fallback
    route (heads padded to 128, attn_fwd<2>).  Rule of tests/test_gpu_fullsize.py: rel(engine, fp32 oracle) < max(1.5 rel(bf16 oracle,
    fp32 oracle), 2e-2), the same weight dict on both sides.  The route counters say which attention kernel ran."""
    spec, w, px, want, e_ref = tower_case(tag, n_layers)
    eng = engine.VitEngine(spec, w, DEV, fuse_ln=mode != "unfused", head_pad=128 if mode == "fallback" else None)
    assert eng.head_pad == (128 if mode == "fallback" else 96) and eng.mlp_pad % 128 == 0 and eng.mlp_pad - spec.mlp < 128
    _lib.routes(reset=True)
    got = eng.forward(px.to(DEV), n_layers=n_layers)
    torch.cuda.synchronize()
    r = _lib.routes(reset=True)
    assert (r["attn_96"], r["attn"], r["attn_cls"]) == ((0, n_layers, 0) if mode == "fallback" else (n_layers, 0, 0)), r
    assert got.shape == want.shape and torch.isfinite(got.float()).all()
    e_hip = rel(got, want)
    print(f"[wide-heads] {tag} x{n_layers} {mode}: rel {e_hip:.4f} (bf16 oracle {e_ref:.4f})")
    assert e_hip < max(1.5 * e_ref, 2e-2), (tag, mode, e_hip, e_ref)


def test_so400m_full_depth():
    """hidden_states[-2] of the 27-layer tower (26 layers run) at 384 px, 2 images, same rule."""
    spec, w, px, want, e_ref = tower_case("so400m", 26)
    got = engine.VitEngine(spec, w, DEV).forward(px.to(DEV), n_layers=26)
    assert got.shape == (2, 729, 1152) and torch.isfinite(got.float()).all()
    e_hip = rel(got, want)
    print(f"[wide-heads] so400m x26: rel {e_hip:.4f} (bf16 oracle {e_ref:.4f})")
    assert e_hip < max(1.5 * e_ref, 2e-2), (e_hip, e_ref)


def test_fp32_engine_takes_the_exact_route():
    """make_engine(.., 'fp32') on the so400m shape: the split-bf16 route needs 64-wide heads, so the exact-fp32 MFMA route runs, within the
    bar tests/test_gpu_f32.py holds that route to (5e-6 relative)."""
    spec, w, px, want, _ = tower_case("so400m", 2)
    eng = engine.make_engine(spec, w, DEV, "fp32")
    assert isinstance(eng, engine.VitEngineF32) and eng.gemm == "native"
    assert rel(eng.forward(px.float().to(DEV), n_layers=2), want) < 5e-6


def test_nothing_moved_for_64_wide_heads():
    """CLIP-L/14-336, 2 layers, batch 3: the image-aligned kernel runs, the new route does not, heads and MLP are not padded."""
    spec = VW.SPECS["openai/clip-vit-large-patch14-336"]
    w = fast_weights(spec, 1, 2)
    eng = engine.VitEngine(spec, w, DEV)
    assert (eng.head_dim, eng.head_pad, eng.mlp_pad, eng.q_prescaled) == (64, 64, 4096, True)
    px = bf(torch.randn(3, 3, 336, 336, generator=torch.Generator().manual_seed(2)))
    _lib.routes(reset=True)
    got = eng.forward(px.to(DEV), n_layers=2)
    torch.cuda.synchronize()
    r = _lib.routes(reset=True)
    assert r["attn_cls"] == 2 and r["attn_96"] == 0 and r["attn"] == 0, r
    assert rel(got, OV.vit_hidden_states(spec, w, px.float(), n_layers=2)[2]) < 2e-2


def test_abi_refuses_what_is_still_unsupported():
    spec = TOWERS["s96"]
    eng = engine.VitEngine(spec, fast_weights(spec, 1, 1), DEV)
    px = torch.zeros(1, 3, 112, 112, dtype=torch.bfloat16, device=DEV)
    eng.forward(px, n_layers=1)
    for field, value, text in (("head_pad", 192, "head_dim above 128"), ("head_pad", 80, "head_pad must be"), ("mlp", 1536 + 64, "mlp"),
                               ("q_prescaled", 1, "pre-scaled Q")):
        old = getattr(eng._cfg, field)
        setattr(eng._cfg, field, value)
        with pytest.raises(RuntimeError, match=text):
            eng.forward(px, n_layers=1)
        setattr(eng._cfg, field, old)
    eng.forward(px, n_layers=1)
    with pytest.raises(ValueError, match="head_dim"):
        engine.VitEngine(replace(spec, heads=2), fast_weights(replace(spec, heads=2), 1, 1), DEV)          # 192-wide heads
    with pytest.raises(ValueError, match="multiple of 128"):
        engine.VitEngine(replace(spec, d=320, heads=4), fast_weights(replace(spec, d=320, heads=4), 1, 1), DEV)


# ------------------------------------------------------------------------------------------------ plug-in path
def write_siglip_checkpoint(path, spec, w):
    """A transformers-layout checkpoint directory (config.json + model.safetensors) of a SigLIP vision tower, from packed weights."""
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({"model_type": "siglip_vision_model", "hidden_size": spec.d, "num_attention_heads": spec.heads, "intermediate_size": spec.mlp,
                   "image_size": spec.image_size, "patch_size": spec.patch, "num_hidden_layers": spec.layers, "hidden_act": "gelu_pytorch_tanh",
                   "layer_norm_eps": spec.eps, "num_channels": 3}, f)
    d = spec.d
    sd = {"vision_model.embeddings.patch_embedding.weight": w["patch_w"].view(d, 3, spec.patch, spec.patch),
          "vision_model.embeddings.patch_embedding.bias": w["patch_b"], "vision_model.embeddings.position_embedding.weight": w["pos"]}
    for i, L in enumerate(w["layers"]):
        pre = f"vision_model.encoder.layers.{i}."
        for j, c in enumerate("qkv"):
            sd[pre + f"self_attn.{c}_proj.weight"], sd[pre + f"self_attn.{c}_proj.bias"] = L["wqkv"][j * d:(j + 1) * d], L["bqkv"][j * d:(j + 1) * d]
        for hf, (wk, bk) in {"self_attn.out_proj": ("wo", "bo"), "layer_norm1": ("ln1_g", "ln1_b"), "layer_norm2": ("ln2_g", "ln2_b"),
                             "mlp.fc1": ("w1", "b1"), "mlp.fc2": ("w2", "b2")}.items():
            sd[pre + hf + ".weight"], sd[pre + hf + ".bias"] = L[wk], L[bk]
    save_file({k: v.contiguous().clone() for k, v in sd.items()}, os.path.join(path, "model.safetensors"))


@pytest.fixture
def so400m_checkpoint(tmp_path):
    spec = replace(VW.SPECS[SO400M], layers=3)
    w = fast_weights(spec, 8, 3)
    path = str(tmp_path / "siglip-so400m-tiny-depth")
    write_siglip_checkpoint(path, spec, w)
    return path, spec, w


def test_plugin_tower_from_a_checkpoint_directory(so400m_checkpoint):
    from law_of_vision_representation_in_mllms_amd.llava.model.multimodal_encoder.builder import build_siglip_vision_tower
    path, spec, w = so400m_checkpoint
    cfg = SimpleNamespace(mm_vision_tower=path, mm_vision_select_layer=-2, device=DEV)
    tower = build_siglip_vision_tower(cfg)
    assert tower.hidden_size == 1152 and tower.num_patches == 729 and tower.spec == replace(spec, name=path)
    px = bf(torch.randn(2, 3, 384, 384, generator=torch.Generator().manual_seed(3))).to(DEV)
    feats = tower(px)
    assert feats.shape == (2, 729, 1152) and feats.dtype == torch.bfloat16
    direct = engine.VitEngine(spec, w, DEV).forward(px, n_layers=2)
    assert torch.equal(feats, direct)


def test_sweep_scores_a_new_tower(so400m_checkpoint, monkeypatch):
    """The law's two scores for an encoder outside the reference registry: the id (a checkpoint directory) goes into
    build_function_mapping as the README tells users to, the two CLIP reference settings run on tiny specs."""
    from law_of_vision_representation_in_mllms_amd import sweep as S
    from law_of_vision_representation_in_mllms_amd.llava.model import llava_arch as LA
    from law_of_vision_representation_in_mllms_amd.llava.model.multimodal_encoder.builder import build_siglip_vision_tower
    path = so400m_checkpoint[0]
    tiny = {S.CLIP336: VW.tiny_spec("clip", image_size=56, patch=14, d=128, heads=2, mlp=256, layers=3),
            S.CLIP224: VW.tiny_spec("clip", image_size=42, patch=14, d=128, heads=2, mlp=256, layers=3)}
    monkeypatch.setattr(VW, "SPECS", {**VW.SPECS, **tiny})
    monkeypatch.setitem(LA.build_function_mapping, path, build_siglip_vision_tower)
    settings = (S.Setting("CLIP336", "clip336", (S.CLIP336,), 56, 4), S.Setting("CLIP224", "clip224", (S.CLIP224,), 42, 5),
                S.Setting("so400m", "so400m", (path,), 384, 4))
    spair = S.synthetic_spair(n_images=12, n_pairs=30, kmax=8, seed=4, categories=("bird", "cow"))
    build = lambda st: S.SettingModel(st, torch.device(DEV), hidden=256, precision="bf16", fast_weights=False)
    _lib.routes(reset=True)
    out = S.run_sweep(settings, 9, spair, torch.device(DEV), build=build, precision="bf16")
    assert _lib.routes(reset=True)["attn_96"] > 0
    ent = out["per_setting"]["so400m"]
    print(f"[wide-heads] sweep so400m (3 layers, random weights): A {ent['A']:.4f}  PCK {ent['pck']}")
    assert np.isfinite(ent["A"]) and np.isfinite(np.asarray(ent["pck"], dtype=np.float64)).all() and len(ent["pck"]) == 3
