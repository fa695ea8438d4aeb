"""Step-1 power-series term rate in fp32 (POVAR_FLAG_FP32_TERMS: e0_ck_f32) against fp64 (e0_ck, variant 1) on one device.

Both modes run on the same context build: lane-per-landmark rows placed inside povar_create (POVAR_FLAG_PLACEMENT(1)), the
camera-chunk layout of variant 1 (POVAR_FLAG_E0_KERNEL(1)), the per-term kernels in the captured hipGraph (resident series off).
Headline settings: m = 20 terms, lambda = 1e-4, tolerances off.  A block is --series solves of the prepared system (the
power series only: povar_power_series_pose, asynchronous, one synchronize per block); after --warmup blocks, the median of
--blocks blocks is reported as us per term and terms/s.  One JSON line per mode on stdout (and into --out).

  python tools/fp32_term_bench.py --shape venice-1778 --mode both --out profiles/fp32_terms_venice.json
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/fp32_term_bench.py --mode fp32 --blocks 3
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_mode(p, fp32, args):
    from povar_amd import capi
    flags = capi.flag_placement(1) | capi.flag_e0_kernel(1) | capi.flag_series_kernel(0) | (capi.FLAG_FP32_TERMS if fp32 else 0)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, e0_mode=capi.E0_IMPLICIT_LDSACC, flags=flags)
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(args.alpha)
    assert ctx.linearize_pose(args.alpha)
    ctx.prepare_pose(args.lam)
    ctx.power_series_pose(args.m)
    ctx.synchronize()
    times = []
    for b in range(args.warmup + args.blocks):
        t = time.perf_counter()
        for _ in range(args.series):
            ctx.power_series_pose(args.m)
        ctx.synchronize()
        if b >= args.warmup:
            times.append(time.perf_counter() - t)
    li = ctx.layout_info()
    lm_bytes, cam_bytes = ctx.e0_model_bytes()
    inc = ctx.get_increment()
    ctx.close()
    us = [1e6 * t / (args.series * args.m) for t in times]
    med = statistics.median(us)
    return {"mode": "fp32" if fp32 else "fp64", "shape": args.shape, "m": args.m, "lambda": args.lam, "blocks": args.blocks,
            "series_per_block": args.series, "us_per_term_median": med, "us_per_term_blocks": us, "terms_per_s": 1e6 / med,
            "fp32_terms": li.fp32_terms, "e0_kernel": li.e0_kernel, "ck_packed": li.ck_packed, "ck_batches": li.ck_batches,
            "model_bytes_e0_kernel": lm_bytes, "model_bytes_cam_kernel": cam_bytes, "_inc": inc}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="venice-1778")
    ap.add_argument("--mode", choices=["fp32", "fp64", "both"], default="both")
    ap.add_argument("--m", type=int, default=20)
    ap.add_argument("--lam", type=float, default=1e-4)
    ap.add_argument("--alpha", type=float, default=0.01)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--series", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from povar_amd import synth
    import numpy as np
    p = synth.make_bal_problem(args.shape)
    modes = {"fp32": [True], "fp64": [False], "both": [False, True]}[args.mode]
    res = [run_mode(p, m, args) for m in modes]
    if len(res) == 2:
        a, b = res[0].pop("_inc"), res[1].pop("_inc")
        res[1]["rel_inc_vs_fp64"] = float(np.linalg.norm(b - a) / np.linalg.norm(a))
        res[1]["speedup_vs_fp64"] = res[0]["us_per_term_median"] / res[1]["us_per_term_median"]
    for r in res:
        r.pop("_inc", None)
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
