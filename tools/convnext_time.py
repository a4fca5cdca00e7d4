"""Per-stage time of the depthwise 7x7 + statistics kernel at a ConvNeXt shape (default ConvNeXt-L, 320 px, batch 64) against torch's own
depthwise F.conv2d plus a separate layer_norm statistics pass on the same box, and whole-tower images/s with synthetic weights.
A comparison only: nothing in the package calls torch's convolution.

Fractions are quoted against the MI355X figures of the microarchitecture guide: 8 TB/s HBM, 157.3 TFLOP/s packed fp32 (v_pk_fma_f32).
Traffic counted: one read and one write of the map (4 bytes per element); FLOP counted: 2 * 49 per output element.

usage: python tools/convnext_time.py [--name SPEC] [--batch 64] [--iters 20] [--no-tower]     -> one JSON line"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from law_of_vision_representation_in_mllms_amd import convnext_weights as CW, engine  # noqa: E402

HBM_BPS, PK_FP32_FLOPS = 8.0e12, 157.3e12


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="laion/CLIP-convnext_large_d_320.laion2B-s29B-b131K-ft-soup")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-tower", action="store_true")
    a = ap.parse_args()
    spec = CW.SPECS[a.name]
    dev = "cuda:0"
    out = {"spec": spec.name, "batch": a.batch, "stages": []}
    for st in range(4):
        side, C = spec.grid(st + 1), spec.hidden_sizes[st]
        g = torch.Generator().manual_seed(st)
        x = torch.randn(a.batch, side, side, C, generator=g).to(torch.bfloat16).to(dev)
        wt = (torch.randn(49, C, generator=g) / 7).to(dev)
        bias = torch.randn(C, generator=g).to(dev)
        t_hip = timed(lambda: engine.dwconv7x7_stats(x, wt, bias), a.iters)
        xc = x.permute(0, 3, 1, 2)                                   # channels-last memory format, as torch would run it
        wc = wt.t().reshape(C, 1, 7, 7).to(torch.bfloat16)
        bc = bias.to(torch.bfloat16)

        def torch_pair():
            y = torch.nn.functional.conv2d(xc, wc, bc, padding=3, groups=C).permute(0, 2, 3, 1).float()
            var, mean = torch.var_mean(y, dim=-1, unbiased=False)
            return (var + 1e-6).rsqrt(), mean

        t_torch = timed(torch_pair, a.iters)
        n = a.batch * side * side * C
        out["stages"].append({"stage": st + 1, "map": side, "C": C, "hip_us": round(t_hip * 1e6, 1), "torch_pair_us": round(t_torch * 1e6, 1),
                              "torch_over_hip": round(t_torch / t_hip, 3), "hbm_fraction": round(4 * n / t_hip / HBM_BPS, 3),
                              "pk_fp32_fraction": round(98 * n / t_hip / PK_FP32_FLOPS, 3)})
    if not a.no_tower:
        eng = engine.ConvNextEngine(spec, CW.synthetic_weights(spec, seed=1), dev)
        px = torch.randn(a.batch, 3, spec.image_size, spec.image_size).to(torch.bfloat16).to(dev)
        t = timed(lambda: eng.forward(px), max(a.iters // 4, 3))
        out["tower_images_per_s"] = round(a.batch / t, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
