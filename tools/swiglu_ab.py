"""A/B of the SwiGLU fc1 on DINOv2-giant shapes: gated GEMM epilogue (visrep_gemm_bf16_gated) against the unfused pair (plain GEMM into
[M, 2 h] + visrep_swiglu), and the whole tower forward with VitEngine(fuse_gate=True / False), in ONE process.  Warm-up, then interleaved
repetitions (fused, unfused, fused, ...), medians and the run-to-run spread (max - min over medians of the two halves) per arm.

usage: python tools/swiglu_ab.py [--res 224 336] [--layers 8] [--reps 15] [--budget-s 240]      -> one JSON line per shape"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from law_of_vision_representation_in_mllms_amd import engine  # noqa: E402
from law_of_vision_representation_in_mllms_amd import vit_weights as VW  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def ab(arms, reps, warm, deadline):
    """arms: {name: callable}; interleaved; returns {name: {"median_ms", "half_medians_ms", "n"}}."""
    for _ in range(warm):
        for f in arms.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(reps):
        if time.time() > deadline:
            break
        for k, f in arms.items():
            t[k].append(timed(f))
    out = {}
    for k, v in t.items():
        h = len(v) // 2
        out[k] = {"median_ms": round(statistics.median(v), 4), "n": len(v),
                  "half_medians_ms": [round(statistics.median(v[:h]), 4), round(statistics.median(v[h:]), 4)] if h else []}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[224, 336])
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--budget-s", type=float, default=240.0, help="time limit per resolution; repetitions stop when it is reached")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.environ["VISREP_FAST_SYNTHETIC"] = "cuda"
    base = VW.SPECS["facebook/dinov2-giant"]
    for res in a.res:
        deadline = time.time() + a.budget_s
        spec = base.at_resolution(res)
        B = engine.best_chunk(spec.tokens, spec.d, 256)          # the batch that fills whole tile rounds of the N = d projections
        M, d, h = B * spec.tokens, spec.d, spec.mlp
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(M, d, generator=g, device=dev).to(torch.bfloat16)
        w_hf = (torch.randn(2 * h, d, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        b_hf = torch.randn(2 * h, generator=g, device=dev) * 0.02
        idx = engine.swiglu_interleave_index(h).to(dev)
        w_il, b_il = w_hf[idx].contiguous(), b_hf[idx].contiguous()
        y = torch.empty(M, h, dtype=torch.bfloat16, device=dev)
        gu = torch.empty(M, 2 * h, dtype=torch.bfloat16, device=dev)
        fc1 = ab({"fused": lambda: engine.gemm_gated(x, w_il, b_il, out=y),
                  "unfused": lambda: engine.swiglu(engine.gemm(x, w_hf, b_hf, out=gu), out=y)}, a.reps, 3, deadline)
        del gu, y, x
        w = VW.synthetic_weights(spec, seed=1, n_layers=a.layers)
        px = torch.randn(B, 3, res, res, generator=g, device=dev).to(torch.bfloat16)
        e1, e0 = engine.VitEngine(spec, w, dev, fuse_gate=True), engine.VitEngine(spec, w, dev, fuse_gate=False)
        out = torch.empty(B, spec.tokens, d, dtype=torch.bfloat16, device=dev)
        fwd = ab({"fused": lambda: e1.forward(px, out=out), "unfused": lambda: e0.forward(px, out=out)}, max(a.reps // 3, 3), 1, deadline)
        print(json.dumps({"tower": base.name, "res": res, "batch": B, "rows": M, "layers": a.layers, "fc1": fc1, "forward": fwd,
                          "fc1_flop": 2.0 * M * 2 * h * d}), flush=True)
        del e1, e0, w
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
