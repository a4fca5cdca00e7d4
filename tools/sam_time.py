"""Times visrep_mhsa_relpos_fwd at the two real SAM-B shapes (windowed: NB = 16 * 25 grids of 14 x 14, global: NB = 16 grids of 64 x 64, 12
heads) against visrep_mhsa_fwd on the same shapes without the position term (the cost of the bias path) and against torch SDPA with the
bias passed as attn_mask; the table kernel's time (into preallocated tables) and bytes against the HBM roof (8 TB/s: the tables written, Q and the R tables read); and
the whole SAM-B tower at 1024 px in images per second (synthetic weights).  Interleaved launches, median of HIP event pairs.
A comparison only: nothing in the package calls torch's attention.

usage: python tools/sam_time.py [--batch 16] [--iters 10] [--tower-batch 4] [--no-sdpa] [--no-tower]     -> one JSON line"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from law_of_vision_representation_in_mllms_amd import engine, sam_weights as SW  # noqa: E402

HBM_BPS = 8.0e12
DEV = "cuda:0"


def interleaved(fns, iters):
    """{name: median seconds} of fns run round-robin, one event pair per call."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    ts = {n: [] for n in fns}
    for _ in range(iters):
        for n, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); f(); b.record()
            torch.cuda.synchronize()
            ts[n].append(a.elapsed_time(b) * 1e-3)
    return {n: statistics.median(v) for n, v in ts.items()}


def shape(NB, S, H, iters, sdpa):
    T, M = S * S, NB * S * S
    g = torch.Generator().manual_seed(S)
    qk = torch.randn(M, 2 * H * 64, generator=g).to(torch.bfloat16).to(DEV)
    ldvt = (M + 63) // 64 * 64
    vt = torch.randn(H * 64, ldvt, generator=g).to(torch.bfloat16).to(DEV)
    Rh, Rw = (torch.randn(2 * S - 1, 64, generator=g).to(DEV) * 0.2 for _ in range(2))
    rel_h, rel_w = engine.relpos_tables(qk, Rh, Rw, NB, S, H)
    fns = {"relpos": lambda: engine.mhsa_relpos(qk, vt, rel_h, rel_w, NB, S, H), "plain": lambda: engine.mhsa(qk, vt, NB, T, H, scale=0.125),
           "tables": lambda: engine.relpos_tables(qk, Rh, Rw, NB, S, H, out=(rel_h, rel_w))}
    if sdpa:
        q, k = (qk[:, i * H * 64:(i + 1) * H * 64].reshape(NB, T, H, 64).transpose(1, 2) for i in range(2))
        v = torch.randn(NB, H, T, 64, generator=g).to(torch.bfloat16).to(DEV)
        # the [NB, H, T, T] bias in bf16 (6.4 GB at the global shape), built one grid at a time: the fp32 gathers stay at one grid's size
        mask = torch.empty(NB, H, T, T, dtype=torch.bfloat16, device=DEV)
        for n in range(NB):
            mask[n] = (rel_h[n].reshape(H, T, S, 1) + rel_w[n].reshape(H, T, 1, S)).reshape(H, T, T)
        fns["sdpa_mask"] = lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask)
    t = interleaved(fns, iters)
    tab_bytes = 2 * NB * H * T * S * 4 + M * H * 64 * 2 + 2 * (2 * S - 1) * 64 * 4
    r = {"NB": NB, "T": T, "H": H, **{n + "_us": round(v * 1e6, 1) for n, v in t.items()}, "relpos_over_plain": round(t["relpos"] / t["plain"], 3),
         "tables_bytes": tab_bytes, "tables_hbm_fraction": round(tab_bytes / t["tables"] / HBM_BPS, 3)}
    if sdpa:
        r["sdpa_over_relpos"] = round(t["sdpa_mask"] / t["relpos"], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--tower-batch", type=int, default=4)
    ap.add_argument("--no-sdpa", action="store_true")
    ap.add_argument("--no-tower", action="store_true")
    a = ap.parse_args()
    out = {"windowed": shape(a.batch * 25, 14, 12, a.iters, not a.no_sdpa), "global": shape(a.batch, 64, 12, a.iters, not a.no_sdpa)}
    if not a.no_tower:
        spec = SW.SPECS["facebook/sam-vit-base"]
        eng = engine.make_sam_engine(spec, SW.synthetic_weights(spec, seed=1), DEV)
        px = torch.randn(a.tower_batch, 3, 1024, 1024).to(torch.bfloat16).to(DEV)
        t = interleaved({"tower": lambda: eng.forward(px)}, max(a.iters // 2, 3))["tower"]
        out["tower"] = {"batch": a.tower_batch, "ms": round(t * 1e3, 2), "images_per_s": round(a.tower_batch / t, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
