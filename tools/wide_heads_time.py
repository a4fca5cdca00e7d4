"""A/B timing of the width-96 attention route (attn_fwd96) against the route it replaces (attn_fwd<2> on heads zero-padded to 128), at the
attention shapes of SigLIP-so400m (B H = 32 x 16, T = 729, true width 72) and ViT-H/14 (64 x 16, T = 257, true width 80), and of the whole
so400m forward (26 layers, batch 32) with each route.  The two routes alternate launch by launch in one process; every figure is the median
of `--iters` launches timed with a HIP event pair each, after `--warmup` untimed ones.  Prints one JSON line (profiles/wide_heads.md).

usage: python tools/wide_heads_time.py [--iters 20] [--warmup 3] [--out file.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from law_of_vision_representation_in_mllms_amd import _lib, engine  # noqa: E402
from law_of_vision_representation_in_mllms_amd import vit_weights as VW  # noqa: E402

DEV = "cuda:0"


def timed(fns, iters, warmup):
    """fns: {name: callable}; alternates them; returns {name: median ms}."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {n: [] for n in fns}
    for _ in range(iters):
        for n, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[n].append(a.elapsed_time(b))
    return {n: round(statistics.median(v), 4) for n, v in ms.items()}, {n: [round(min(v), 4), round(max(v), 4)] for n, v in ms.items()}


def attention_ab(B, H, T, true, iters, warmup):
    g = torch.Generator(device=DEV).manual_seed(B + T)
    bufs = {}
    for dp in (96, 128):
        qk = torch.zeros(B * T, 2, H, dp, device=DEV)
        qk[..., :true] = torch.randn(B * T, 2, H, true, generator=g, device=DEV)
        vt = torch.zeros(H, dp, (B * T + 63) // 64 * 64 + 64, device=DEV)
        vt[:, :true] = torch.randn(H, true, vt.shape[2], generator=g, device=DEV)
        bufs[dp] = (qk.reshape(B * T, 2 * H * dp).to(torch.bfloat16), vt.reshape(H * dp, -1).to(torch.bfloat16))
    fns = {f"pad{dp}": (lambda dp=dp: engine.mhsa(bufs[dp][0], bufs[dp][1], B, T, H, true ** -0.5, head_dim=dp)) for dp in (96, 128)}
    med, rng = timed(fns, iters, warmup)
    flop = 4.0 * B * H * T * T * true                                    # useful work: the true width
    return {"B": B, "H": H, "T": T, "true_width": true, "median_ms": med, "min_max_ms": rng,
            "useful_tflops": {n: round(flop / (v * 1e-3) / 1e12, 1) for n, v in med.items()}, "speedup_96_over_128": round(med["pad128"] / med["pad96"], 3)}


def forward_ab(batch, iters, warmup):
    spec = VW.SPECS["google/siglip-so400m-patch14-384"]
    os.environ["VISREP_FAST_SYNTHETIC"] = "cuda"
    w = VW.synthetic_weights(spec, seed=1, n_layers=26)
    os.environ.pop("VISREP_FAST_SYNTHETIC")
    px = torch.randn(batch, 3, 384, 384, device=DEV, dtype=torch.bfloat16)
    engs = {"pad96": engine.VitEngine(spec, w, DEV), "pad128": engine.VitEngine(spec, w, DEV, head_pad=128)}
    out = torch.empty(batch, spec.tokens, spec.d, dtype=torch.bfloat16, device=DEV)
    med, rng = timed({n: (lambda e=e: e.forward(px, n_layers=26, out=out)) for n, e in engs.items()}, iters, warmup)
    return {"tower": spec.name, "layers": 26, "batch": batch, "median_ms": med, "min_max_ms": rng,
            "images_per_s": {n: round(batch / (v * 1e-3), 1) for n, v in med.items()}, "speedup_96_over_128": round(med["pad128"] / med["pad96"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "cus": int(_lib.load().visrep_device_cu_count()), "iters": a.iters, "warmup": a.warmup,
           "attention": [attention_ab(32, 16, 729, 72, a.iters, a.warmup), attention_ab(64, 16, 257, 80, a.iters, a.warmup)],
           "forward": forward_ab(32, max(10, a.iters // 2), a.warmup)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
