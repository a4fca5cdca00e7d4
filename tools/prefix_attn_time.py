"""A/B timing of the prefix-key image-aligned attention route (attn_fwd_prefix) against the route the same register tower takes with
VISREP_Q_PRESCALE=1 (attn_fwd on global 64-key tiles, pre-scaled Q), at the attention shapes of DINOv2-with-registers-large (B H = 64 x 16,
T = 261 at 224 px and T = 581 at 336 px, 5 prefix tokens), and of the whole register-large forward (24 layers) with each route.  The two
routes alternate launch by launch in one process; every figure is the median of `--iters` launches timed with a HIP event pair each, after
`--warmup` untimed ones.  Prints one JSON line (profiles/registers.md).

usage: python tools/prefix_attn_time.py [--iters 20] [--warmup 3] [--batch 64] [--out file.json]"""
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
NAME = "facebook/dinov2-with-registers-large"


def timed(fns, iters, warmup):
    """fns: {name: callable}; alternates them; returns ({name: median ms}, {name: [min, max]})."""
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


def attention_ab(B, H, T, NP, iters, warmup):
    """One attention layer: the same Q | K and V values in both routes' layouts (V^T over all tokens / over the patch tokens + prefix rows)."""
    g = torch.Generator(device=DEV).manual_seed(B + T)
    P = T - NP
    qk = torch.randn(B * T, 2 * H * 64, generator=g, device=DEV)
    qk[:, : H * 64] *= 0.125 * 1.4426950408889634
    qk = qk.to(torch.bfloat16)
    v = torch.randn(B, T, H * 64, generator=g, device=DEV).to(torch.bfloat16)
    eye = torch.eye(H * 64, dtype=torch.bfloat16, device=DEV)
    vt_all = engine.linear_vt(v.reshape(B * T, -1), eye, None)
    vt_patch = engine.linear_vt(v[:, NP:].reshape(B * P, -1).contiguous(), eye, None)
    vpre = v[:, :NP].reshape(B * NP, -1).contiguous()
    fns = {"prefix": lambda: engine.mhsa_prefix(qk, vt_patch, vpre, B, T, NP, H), "general": lambda: engine.mhsa(qk, vt_all, B, T, H, 0.0)}
    med, rng = timed(fns, iters, warmup)
    flop = 4.0 * B * H * T * T * 64
    return {"B": B, "H": H, "T": T, "prefix": NP, "median_ms": med, "min_max_ms": rng,
            "tflops": {n: round(flop / (t * 1e-3) / 1e12, 1) for n, t in med.items()}, "speedup_prefix_over_general": round(med["general"] / med["prefix"], 3)}


def forward_ab(size, batch, iters, warmup):
    spec = VW.SPECS[NAME].at_resolution(size)
    os.environ["VISREP_FAST_SYNTHETIC"] = "cuda"
    w = VW.synthetic_weights(spec, seed=1)
    os.environ.pop("VISREP_FAST_SYNTHETIC")
    px = torch.randn(batch, 3, size, size, device=DEV, dtype=torch.bfloat16)
    engs = {}
    for name, mode in (("prefix", "2"), ("general", "1")):       # the knob is read when the engine is built
        os.environ["VISREP_Q_PRESCALE"] = mode
        engs[name] = engine.VitEngine(spec, w, DEV)
    os.environ.pop("VISREP_Q_PRESCALE")
    out = torch.empty(batch, spec.tokens, spec.d, dtype=torch.bfloat16, device=DEV)
    routes = {}
    for name, e in engs.items():
        _lib.routes(reset=True)
        e.forward(px, out=out)
        routes[name] = {k: v for k, v in _lib.routes(reset=True).items() if v and k.startswith("attn")}
    med, rng = timed({n: (lambda e=e: e.forward(px, out=out)) for n, e in engs.items()}, iters, warmup)
    return {"tower": NAME, "image_size": size, "tokens": spec.tokens, "layers": spec.layers, "batch": batch, "attention_routes": routes, "median_ms": med,
            "min_max_ms": rng, "images_per_s": {n: round(batch / (v * 1e-3), 1) for n, v in med.items()},
            "speedup_prefix_over_general": round(med["general"] / med["prefix"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "cus": int(_lib.load().visrep_device_cu_count()), "iters": a.iters, "warmup": a.warmup,
           "attention": [attention_ab(a.batch, 16, T, 5, a.iters, a.warmup) for T in (261, 581)],
           "forward": [forward_ab(size, a.batch, max(10, a.iters // 2), a.warmup) for size in (224, 336)]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
