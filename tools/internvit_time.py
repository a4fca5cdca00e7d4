"""Timing of what the InternViT towers add, at the InternViT-6B shape (d 3200 = 25 heads x 128, MLP 12800, T = 1025):

  qk_norm     the QK-norm pass (qk_rmsnorm_rows, in place on [M, 2 da], M = batch x 1025, da = 3200) against the Q|K GEMM it follows (M x 6400 x 3200,
              LayerNorm-folded epilogue fed with RMS statistics) and against its own byte count (it reads and writes 4 M da bytes) over the HBM
              bandwidth a plain device-to-device copy of the same bytes reaches in this process;
  layer       one 6B-shaped layer with the norms folded into the GEMMs (default) against VISREP_FUSE_LN=0 (visrep_rmsnorm passes).

The timed alternatives alternate launch by launch in one process; every figure is the median of `--iters` launches timed with a HIP event
pair each, after `--warmup` untimed ones.  Shader clock and socket power under the QK-norm pass and the layer come from the sysfs sampler
(telemetry.py) where the board exposes them.  Prints one JSON line (profiles/internvit.md).

usage: python tools/internvit_time.py [--iters 20] [--warmup 3] [--batch 8] [--out file.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from law_of_vision_representation_in_mllms_amd import _lib, engine, telemetry  # noqa: E402
from law_of_vision_representation_in_mllms_amd import vit_weights as VW  # noqa: E402

DEV = "cuda:0"
NAME = "OpenGVLab/InternViT-6B-448px-V2_5"


def timed(fns, iters, warmup):
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


def board(fn):
    """Socket power / shader clock under ~1.5 s of back-to-back launches; {"available": False} where the board's sysfs nodes cannot be read."""
    t = telemetry.measure(fn, 1.5)
    return {k: t[k] for k in ("available", "power_w", "sclk_mhz", "samples") if k in t}


def qk_norm_pass(batch, iters, warmup):
    lib = _lib.require_gpu()
    spec = VW.SPECS[NAME]
    M, d = batch * spec.tokens, spec.d
    da = d
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(M, d, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(2 * da, d, generator=g, device=DEV) * 0.02).to(torch.bfloat16)
    s = w.float().sum(1).contiguous()
    bias = torch.zeros(2 * da, device=DEV)
    rt = torch.empty(M + 8, 2, device=DEV)
    qk = torch.empty(M, 2 * da, dtype=torch.bfloat16, device=DEV)
    src = torch.randn(M, 2 * da, generator=g, device=DEV).to(torch.bfloat16)
    dst = torch.empty_like(src)
    qg, kg = torch.rand(da, generator=g, device=DEV) + 0.5, torch.rand(da, generator=g, device=DEV) + 0.5
    st = _lib.stream_ptr
    _lib.check(lib.visrep_rmsnorm_stats(_lib.ptr(x), d, _lib.ptr(rt), M, d, 1e-6, st()), "rmsnorm_stats")
    fns = {
        "qk_gemm": lambda: _lib.check(lib.visrep_gemm_bf16_ln(_lib.ptr(x), d, _lib.ptr(w), d, _lib.ptr(bias), _lib.ptr(rt), _lib.ptr(s), _lib.ptr(qk), 2 * da, M,
                                                              2 * da, d, _lib.EPI_BIAS, 0, st()), "gemm_ln"),
        "qk_norm": lambda: _lib.check(lib.visrep_qk_rmsnorm(_lib.ptr(src), 2 * da, da, d, _lib.ptr(qg), _lib.ptr(kg), M, 1e-6, st()), "qk_rmsnorm"),
        "copy_same_bytes": lambda: dst.copy_(src),
        "rms_stats": lambda: _lib.check(lib.visrep_rmsnorm_stats(_lib.ptr(x), d, _lib.ptr(rt), M, d, 1e-6, st()), "rmsnorm_stats"),
    }
    med, rng = timed(fns, iters, warmup)
    nbytes = 2 * (M * 2 * da * 2)                                 # [M, 2 da] bf16 read once and written once
    bw = lambda t: round(nbytes / (t * 1e-3) / 1e12, 3)
    return {"M": M, "da": da, "bytes": nbytes, "median_ms": med, "min_max_ms": rng, "qk_norm_tb_s": bw(med["qk_norm"]), "copy_tb_s": bw(med["copy_same_bytes"]),
            "qk_norm_over_copy": round(med["qk_norm"] / med["copy_same_bytes"], 3), "qk_norm_over_qk_gemm": round(med["qk_norm"] / med["qk_gemm"], 4),
            "qk_gemm_tflops": round(2.0 * M * 2 * da * d / (med["qk_gemm"] * 1e-3) / 1e12, 1), "board_under_qk_norm": board(fns["qk_norm"])}


def layer_ab(batch, iters, warmup):
    spec = VW.SPECS[NAME]
    os.environ["VISREP_FAST_SYNTHETIC"] = "cuda"
    w = VW.synthetic_weights(spec, seed=1, n_layers=1)
    os.environ.pop("VISREP_FAST_SYNTHETIC")
    px = torch.randn(batch, 3, spec.image_size, spec.image_size, device=DEV, dtype=torch.bfloat16)
    engs = {"folded": engine.VitEngine(spec, w, DEV, fuse_ln=True), "unfused": engine.VitEngine(spec, w, DEV, fuse_ln=False)}
    out = torch.empty(batch, spec.tokens, spec.d, dtype=torch.bfloat16, device=DEV)
    routes, ms = {}, {}
    for name, e in engs.items():
        _lib.routes(reset=True)
        e.forward(px, n_layers=1, out=out)
        routes[name] = {k: v for k, v in _lib.routes(reset=True).items() if v}
    # a layer = forward(1) - forward(0): the embedding is the same in both
    fns = {f"{n}_{k}": (lambda e=e, k=k: e.forward(px, n_layers=k, out=out)) for n, e in engs.items() for k in (0, 1)}
    med, rng = timed(fns, iters, warmup)
    layer = {n: round(med[f"{n}_1"] - med[f"{n}_0"], 4) for n in engs}
    return {"batch": batch, "tokens": spec.tokens, "routes": routes, "median_ms": med, "min_max_ms": rng, "layer_ms": layer,
            "folded_over_unfused": round(layer["folded"] / layer["unfused"], 4), "board_under_folded_layer": board(fns["folded_1"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    engine.ensure_scratch(DEV)
    res = {"device": torch.cuda.get_device_name(0), "cus": int(_lib.load().visrep_device_cu_count()), "iters": a.iters, "warmup": a.warmup,
           "qk_norm": qk_norm_pass(a.batch, a.iters, a.warmup), "layer": layer_ab(a.batch, a.iters, a.warmup)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
