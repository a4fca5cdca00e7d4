"""ConvNeXt towers on the GPU: the depthwise 7x7 + statistics kernel and the LayerNorm + space-to-depth kernel against their host twins and
float64, orientation, isolation, and the composed tower against transformers.ConvNextModel under the project's rule e_hip <= 2 e_ref (e_ref =
the same module run in bf16 against its own fp32 run)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _convnext_cases as CC
from law_of_vision_representation_in_mllms_amd import _lib, convnext_weights as CW, engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def routed(fn):
    _lib.routes(reset=True)
    out = fn()
    torch.cuda.synchronize()
    return out, {k: v for k, v in _lib.routes(reset=True).items() if v}


# ------------------------------------------------------------------------------------------------ 1. kernel contract
@pytest.mark.parametrize("case", CC.DW_CASES, ids=str)
def test_dwconv_against_twin_and_float64(case):
    x, wt, bias = CC.dw_input(case)
    (y, rt), r = routed(lambda: engine.dwconv7x7_stats(x.to(DEV), wt.to(DEV), bias.to(DEV)))
    assert r == {CC.DW_ROUTE[case]: 1, "dwconv_finalize": 1, **({} if (case[3] // 64) % 2 else {"stats_epilogue": 1})}, r
    y, rt = y.cpu(), rt.cpu()
    frac = CC.dw_check_output(y, case)
    worst = CC.dw_check_rt(rt, y, case)
    yt, rtt = engine.dwconv7x7_stats_cpu(x, wt, bias)
    assert torch.equal(y.float(), yt.float()), "the kernel and its host twin run the same fmaf chain"
    _, bound = CC.rt_bound(yt.double().numpy().reshape(-1, case[3]))
    assert np.all(np.abs(rt.double().numpy() - rtt.double().numpy()) <= bound)
    print(f"[convnext] dwconv {case} {r}: {frac:.2e} of the outputs on a rounding boundary, rt at {worst:.3f} of its bound")


def test_dwconv_statistics_come_from_the_rounded_outputs():
    x, wt, bias = CC.rounded_stats_input()
    y, rt = engine.dwconv7x7_stats(x.to(DEV), wt.to(DEV), bias.to(DEV))
    CC.rounded_stats_check(y.cpu(), rt.cpu())


@pytest.mark.parametrize("hw", [(8, 9), (16, 32)], ids=["tile8", "tile16"])
def test_dwconv_orientation(hw):
    """An impulse with a distinct weight per tap reproduces the kernel un-flipped (cross-correlation).  8 x 9: two 8 x 8 tiles compute 128
    outputs where one 16 x 16 tile computes 256; 16 x 32: both shapes compute 512 and the tie goes to 16 x 16 (less halo).  The expected
    route is worked out here by the launcher's documented rule: the smaller padded area."""
    H, W = hw
    C_ = 64
    x = torch.zeros(1, H, W, C_, dtype=torch.bfloat16)
    x[0, 4, 5] = 1.0
    wt = (torch.arange(49, dtype=torch.float32)[:, None] + 1).repeat(1, C_) * (1 + torch.arange(C_) % 2)
    (y, _), r = routed(lambda: engine.dwconv7x7_stats(x.to(DEV), wt.to(DEV), torch.zeros(C_, device=DEV)))
    area16, area8 = -(-H // 16) * -(-W // 16) * 256, -(-H // 8) * -(-W // 8) * 64
    assert ("dwconv_8" in r) == (area8 < area16) and ("dwconv_16" in r) == (area8 >= area16), r
    assert (area8 < area16) == (hw == (8, 9)), "the two cases must take the two tile shapes"
    y = y.cpu()
    for ky in range(7):
        for kx in range(7):
            oy, ox = 4 - ky + 3, 5 - kx + 3
            if 0 <= oy < H and 0 <= ox < W:
                assert torch.equal(y[0, oy, ox].float(), wt[ky * 7 + kx]), (ky, kx)
    assert torch.equal(y, engine.dwconv7x7_stats_cpu(x, wt, torch.zeros(C_))[0])


@pytest.mark.parametrize("case", [(2, 5, 9, 64), (2, 16, 31, 64)], ids=str)     # 8 x 8 tiles; 16 x 16 tiles, ragged
def test_dwconv_isolation(case):
    """Changing image 1 leaves image 0's rows bitwise unchanged; poison in the ldx padding columns is never read; nothing past y's C columns
    or rows is written."""
    B, H, W, C_ = case
    x, wt, bias = CC.dw_input(case)
    xp = torch.full((B, H, W, C_ + 16), float("nan"), dtype=torch.bfloat16)
    xp[..., :C_] = x
    ya, rta = engine.dwconv7x7_stats(xp.to(DEV), wt.to(DEV), bias.to(DEV), C=C_)
    yb, rtb = engine.dwconv7x7_stats(x.to(DEV), wt.to(DEV), bias.to(DEV))
    assert torch.isfinite(ya.float()).all() and torch.equal(ya, yb) and torch.equal(rta, rtb)
    x2 = xp.clone()
    x2[1, ..., :C_] = float("inf")
    yc, rtc = engine.dwconv7x7_stats(x2.to(DEV), wt.to(DEV), bias.to(DEV), C=C_)
    assert torch.equal(yc[0], ya[0]) and torch.equal(rtc[: H * W], rta[: H * W])
    assert not torch.isfinite(yc[1].float()).any()


@pytest.mark.parametrize("case", CC.S2D_CASES, ids=str)
def test_space_to_depth_against_twin_and_float64(case):
    x, g, b = CC.s2d_input(case)
    out, r = routed(lambda: engine.ln_space_to_depth2(x.to(DEV), g.to(DEV), b.to(DEV)))
    assert r == {"ln_s2d": 1}
    CC.s2d_check(out.cpu(), x, g, b)
    twin = engine.ln_space_to_depth2_cpu(x, g, b)
    # both are within one bf16 rounding of the same fp32-accurate value: at most one bf16 step apart
    d = (out.cpu().double() - twin.double()).abs()
    assert (d <= 2.0 ** -7 * twin.double().abs() + 1e-30).all()
    xp = torch.full(tuple(x.shape[:3]) + (case[3] + 8,), float("nan"), dtype=torch.bfloat16)
    xp[..., : case[3]] = x
    assert torch.equal(engine.ln_space_to_depth2(xp.to(DEV), g.to(DEV), b.to(DEV), C=case[3]), out)


# ------------------------------------------------------------------------------------------------ 2. tower parity
def tower_states(eng, px):
    out = []
    for k in range(5):
        got, r = routed(lambda: eng.forward(px.to(DEV), n_stages=k))
        out.append((got.float().cpu(), r))
    return out


def check_tower(tag, spec, w, px, key):
    want, e_ref = CC.oracle_pair(key, spec, w, px)
    eng = engine.ConvNextEngine(spec, w, DEV)
    worst = 0.0
    for k, (got, r) in enumerate(tower_states(eng, px)):
        assert got.shape == want[k].shape == (px.shape[0], spec.grid(k) ** 2, spec.width(k))
        blocks = sum(spec.depths[:k])
        assert r.get("dwconv_16", 0) + r.get("dwconv_8", 0) == blocks and r.get("dwconv_finalize", 0) == blocks and r.get("ln_s2d", 0) == max(k - 1, 0), (k, r)
        e = CC.rel(got, want[k])
        worst = max(worst, e / e_ref[k])
        print(f"[convnext] {tag} state {k}: e_hip {e:.3e} e_ref {e_ref[k]:.3e} ratio {e / e_ref[k]:.2f} {r}")
        assert e <= 2 * e_ref[k], (tag, k, e, e_ref[k])
    print(f"[convnext] {tag}: worst ratio {worst:.2f}")


@pytest.mark.parametrize("kind", ["synthetic", "hostile"])
@pytest.mark.parametrize("image", [64, 96])
def test_tiny_tower_parity(image, kind):
    spec = CW.tiny_spec(image, **CC.TINY)
    w = CW.hostile_weights(spec, seed=6, profile="all") if kind == "hostile" else CW.synthetic_weights(spec, seed=6)
    check_tower(f"tiny {image} {kind}", spec, w, CC.pixels(3, image, image), ("tiny", image, kind))


def test_full_width_few_blocks():
    """ConvNeXt-L widths, one block per stage, 64 px: width 1536 on a 2 x 2 map and the padded width 192 both run."""
    spec = CW.tiny_spec(64, **CC.LARGE_WIDTHS)
    w = CW.synthetic_weights(spec, seed=8)
    check_tower("L widths", spec, w, CC.pixels(2, 64, 5), ("large", 64))


# ------------------------------------------------------------------------------------------------ 3. plug-in
def test_plugin_returns_stage_maps(monkeypatch):
    from law_of_vision_representation_in_mllms_amd.llava.model.multimodal_encoder import convnext_encoder as CE
    spec = CW.tiny_spec(64, **CC.TINY)
    monkeypatch.setitem(CW.SPECS, "tiny-convnext", spec)
    px = CC.pixels(2, 64, 9)
    for layer, grid, width in ((-1, 2, 256), (-2, 4, 192)):
        t = CE.ConvNextVisionTower("tiny-convnext", SimpleNamespace(mm_vision_select_layer=layer, mm_vision_select_feature="patch",
                                                                    synthetic_weights=True, device=DEV))
        assert t.is_loaded and (t.hidden_size, t.num_patches) == (width, grid * grid)
        f = t(px)
        assert f.shape == (2, grid * grid, width) and f.dtype == px.dtype and torch.isfinite(f).all()
        want = engine.ConvNextEngine(spec, CW.synthetic_weights(spec, seed=1), DEV).forward(px.to(DEV), n_stages=5 + layer)
        assert torch.equal(f, want.to(px.dtype))
        assert t.dummy_feature.shape == (1, width)
