#!/usr/bin/env python3
"""Times the explicit-Schur-complement solvers (PCG / CHOLESKY / RIPCG) on a synthetic BAL shape and checks
them through size-independent properties: |S x + b| / |b| with S applied by the independent
right_mul_e0 entry point, PCG(tight eta) == CHOLESKY.   usage: sc_solvers_bench.py [shape] [lambda]

With --assembly atomics|ordered|both|auto the tool instead times the direct solves of both steps (CHOLESKY on step 1's system,
RICHOLESKY on step 2's, the states of tools/joint_cholesky_bench.py) per assembly of the dense matrix, selected through
set_sc_assembly on ONE context: the assembly's own launches (HIP events around them: povar_profile_info.e0_ms of a dense call)
and the whole solve stage (povar_timings.solve_ms: assembly + factorisation + substitution), one warm-up solve and --reps timed
ones each.  `auto` leaves the library's choice and calls no setter, so it also runs a library from before the switch (POVAR_LIB),
whose assembly interval reads 0.   usage: sc_solvers_bench.py [shape] [lambda] --assembly both [--reps 3]

--free-first K fixes all but the first K cameras (set_fixed_cameras: a window), --compaction 0|1|both selects the layout of the
dense matrix (set_dense_compaction; 1: the free cameras only).  With `both` the two layouts alternate on the one context, --runs
times each (one warm-up solve and --reps timed ones per run), and the device bytes after each are printed.  "rest of the solve
stage" is whole solve - assembly: the all-reduce, the fixing of the cameras, factorisation, substitution and the scatter."""
import argparse
import sys
import time
import os

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from povar_amd import capi, synth  # noqa: E402

ASSEMBLY = {"atomics": 1, "ordered": 2}


def assembly_report(shape, lam, which, reps, free_first=None, compaction="0", runs=1):
    p = synth.make_bal_problem(shape)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs / 500.0, e0_mode=capi.E0_IMPLICIT_LDSACC)
    ctx.layout_finalize()
    ctx.timings_enable(True)
    modes = ["atomics", "ordered"] if which == "both" else [which]
    layouts = [0, 1] if compaction == "both" else [int(compaction)]
    if free_first is not None:
        ctx.set_fixed_cameras(np.arange(min(free_first, p.n_cams), p.n_cams))
        print(f"fixed cameras: all but the first {min(free_first, p.n_cams)} of {p.n_cams}", flush=True)

    def timed(solve):
        solve()  # warm-up: code objects, the dense buffer
        ctx.profile_enable(True)
        t0 = ctx.timings()
        for _ in range(reps):
            x, it, st, rc = solve()
            assert rc == 0 and it == 0
        t1 = ctx.timings()
        pi = ctx.profile_get()
        ctx.profile_enable(False)
        assert t1.solve_calls - t0.solve_calls == reps
        return x, pi.e0_ms / reps, (t1.solve_ms - t0.solve_ms) / reps

    def step(name, dim, solve):
        out = {}
        for m in modes:
            if m != "auto":
                ctx.set_sc_assembly(ASSEMBLY[m])
            for run in range(runs):
                for layout in layouts:
                    if hasattr(ctx.L, "povar_set_dense_compaction"):
                        ctx.set_dense_compaction(layout)
                    x, asm_ms, solve_ms = timed(solve)
                    ran = ctx.sc_assembly() if hasattr(ctx.L, "povar_sc_assembly") else "?"
                    rows = ctx.dense_layout()[0] if hasattr(ctx.L, "povar_dense_layout") else dim * p.n_cams
                    out[m] = (x, asm_ms, solve_ms)
                    print(f"{name} n = {rows}, compaction {layout}, run {run}, assembly {m} (ran {ran}): assembly {asm_ms:.2f} ms, "
                          f"rest of the solve stage {solve_ms - asm_ms:.1f} ms, whole solve {solve_ms:.1f} ms (device, mean of {reps}); "
                          f"device bytes {ctx.device_bytes()}", flush=True)
        if len(out) == 2:
            (xa, aa, sa), (xo, ao, so) = out["atomics"], out["ordered"]
            print(f"{name} ordered / atomics: assembly {ao / aa:.2f} x, whole solve {so / sa:.2f} x, "
                  f"|x_ordered - x_atomics| / |x_atomics| = {np.linalg.norm(xo - xa) / np.linalg.norm(xa):.2e}", flush=True)

    # the states of tools/joint_cholesky_bench.py: step 1 in the units of the normalised observations ...
    cams1 = p.cams.copy()
    cams1[:, :8] /= 500.0
    ctx.set_cameras(cams1)
    ctx.init_landmarks_pose(0.01)
    ctx.set_jl_col_scaling(False)
    assert ctx.linearize_pose(0.01)
    step("step 1 CHOLESKY  ", 12, lambda: ctx.solve_pose_sc(lam, capi.SC_CHOLESKY))
    # ... step 2 at random normalised cameras and X_w = 1 landmarks
    rng = np.random.default_rng(11)
    cams = rng.normal(size=(p.n_cams, 12))
    cams[:, 8:11] *= 0.1
    cams[:, 11] = 5 + rng.random(p.n_cams)
    cams /= np.linalg.norm(cams, axis=1, keepdims=True)
    lms_h = np.concatenate([rng.normal(size=(p.n_lms, 3)), np.ones((p.n_lms, 1))], 1)
    ctx.set_cameras(cams)
    ctx.set_landmarks_homogeneous(lms_h)
    assert ctx.linearize_homogeneous()
    step("step 2 RICHOLESKY", 11, lambda: ctx.solve_joint_sc(lam, method=capi.SC_CHOLESKY))
    print("device MiB:", ctx.device_bytes() >> 20)
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shape", nargs="?", default="venice-1778")
    ap.add_argument("lam", nargs="?", type=float, default=None)
    ap.add_argument("--assembly", choices=["atomics", "ordered", "both", "auto"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--free-first", type=int, default=None, metavar="K", help="fix all but the first K cameras")
    ap.add_argument("--compaction", choices=["0", "1", "both"], default="0", help="layout of the dense matrix (set_dense_compaction)")
    ap.add_argument("--runs", type=int, default=3, help="with --compaction both: alternations of the two layouts")
    a = ap.parse_args()
    if a.assembly or a.free_first is not None or a.compaction != "0":
        return assembly_report(a.shape, 1e-2 if a.lam is None else a.lam, a.assembly or "auto", a.reps, a.free_first, a.compaction,
                               a.runs if a.compaction == "both" else 1)
    shape, lam = a.shape, 1e-4 if a.lam is None else a.lam
    p = synth.make_bal_problem(shape)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, e0_mode=capi.E0_IMPLICIT_LDSACC)
    ctx.layout_finalize()
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(0.01)
    ctx.set_jl_col_scaling(False)
    assert ctx.linearize_pose(0.01)

    def residual(x):
        bm = ctx.get_buffer(capi.BUF_SC_BLOCKDIAG).reshape(p.n_cams, 12, 12)
        b = ctx.get_buffer(capi.BUF_B)
        Sx = np.einsum("cij,cj->ci", bm, x.reshape(-1, 12)).ravel() - ctx.right_mul_e0_pose(x)
        return np.linalg.norm(Sx + b) / np.linalg.norm(b)

    out = {}
    for eta, mx in [(1e-2, 500), (1e-6, 500)]:
        ctx.solve_pose_sc(lam, capi.SC_PCG, 0, mx, eta)  # warm
        t0 = time.perf_counter()
        inc, it, st, rc = ctx.solve_pose_sc(lam, capi.SC_PCG, 0, mx, eta)
        dt = time.perf_counter() - t0
        out[eta] = inc
        print(f"PCG eta={eta:g}: {it} iterations, status {st}, {dt*1e3:.1f} ms total, {dt/it*1e6:.0f} us/iteration, "
              f"|Sx+b|/|b| = {residual(inc):.3e}", flush=True)
    t0 = time.perf_counter()
    inc_c, it, st, rc = ctx.solve_pose_sc(lam, capi.SC_CHOLESKY)
    dt1 = time.perf_counter() - t0
    t0 = time.perf_counter()
    inc_c, it, st, rc = ctx.solve_pose_sc(lam, capi.SC_CHOLESKY)
    dt = time.perf_counter() - t0
    n = 12 * p.n_cams
    print(f"CHOLESKY n={n}: first {dt1*1e3:.1f} ms, then {dt*1e3:.1f} ms ({n**3/3/dt/1e12:.2f} TFLOP/s incl. assembly), rc {rc}, "
          f"|Sx+b|/|b| = {residual(inc_c):.3e}", flush=True)
    print("PCG(1e-6) vs CHOLESKY:", np.linalg.norm(out[1e-6] - inc_c) / np.linalg.norm(inc_c))
    print("device MiB:", ctx.device_bytes() >> 20)
    ctx.close()


if __name__ == "__main__":
    main()
