#!/usr/bin/env python3
"""Times step 2's direct solve (povar_solve_joint_sc_method with POVAR_SC_CHOLESKY, `bal --solver-type-step-2 RICHOLESKY`) on a
synthetic BAL shape, with step 1's CHOLESKY on the same context beside it, and checks both through the residual
|S x + b| / |b| with E0 applied by the independent right_mul_e0 entry points.  The times are device times
(povar_timings.solve_ms: hipEvents around assembly + factorisation + substitution), one warm-up solve and REPS timed ones.
usage: joint_cholesky_bench.py [shape] [lambda] [reps]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from povar_amd import capi, synth  # noqa: E402


def main():
    shape = sys.argv[1] if len(sys.argv) > 1 else "venice-1778"
    lam = float(sys.argv[2]) if len(sys.argv) > 2 else 1e-2
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    p = synth.make_bal_problem(shape)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs / 500.0, e0_mode=capi.E0_IMPLICIT_LDSACC)
    ctx.layout_finalize()
    ctx.timings_enable(True)

    def timed(solve):
        solve()  # warm-up: code objects, the dense buffer
        t0 = ctx.timings()
        for _ in range(reps):
            x, it, st, rc = solve()
            assert rc == 0 and it == 0
        t1 = ctx.timings()
        assert t1.solve_calls - t0.solve_calls == reps
        return x, (t1.solve_ms - t0.solve_ms) / reps

    def residual(x, dim, b, e0):
        bm = ctx.get_buffer(capi.BUF_SC_BLOCKDIAG, joint=dim == 11).reshape(p.n_cams, dim, dim)
        rhs = ctx.get_buffer(b)
        Sx = np.einsum("cij,cj->ci", bm, x.reshape(-1, dim)).ravel() - e0(x)
        return np.linalg.norm(Sx + rhs) / np.linalg.norm(rhs)

    # step 1 in the units of the normalised observations (the first two rows of every P divided by 500)
    cams1 = p.cams.copy()
    cams1[:, :8] /= 500.0
    ctx.set_cameras(cams1)
    ctx.init_landmarks_pose(0.01)
    ctx.set_jl_col_scaling(False)
    assert ctx.linearize_pose(0.01)
    x1, ms1 = timed(lambda: ctx.solve_pose_sc(lam, capi.SC_CHOLESKY))
    print(f"step 1 CHOLESKY   n = {12 * p.n_cams}: {ms1:.1f} ms per solve (device), |Sx+b|/|b| = "
          f"{residual(x1, 12, capi.BUF_B, ctx.right_mul_e0_pose):.3e}", flush=True)
    # step 2: the state of the at-size tests (random normalised cameras, X_w = 1 landmarks)
    rng = np.random.default_rng(11)
    cams = rng.normal(size=(p.n_cams, 12))
    cams[:, 8:11] *= 0.1
    cams[:, 11] = 5 + rng.random(p.n_cams)
    cams /= np.linalg.norm(cams, axis=1, keepdims=True)
    lms_h = np.concatenate([rng.normal(size=(p.n_lms, 3)), np.ones((p.n_lms, 1))], 1)
    ctx.set_cameras(cams)
    ctx.set_landmarks_homogeneous(lms_h)
    assert ctx.linearize_homogeneous()
    x2, ms2 = timed(lambda: ctx.solve_joint_sc(lam, method=capi.SC_CHOLESKY))
    print(f"step 2 RICHOLESKY n = {11 * p.n_cams}: {ms2:.1f} ms per solve (device), |Sx+b|/|b| = "
          f"{residual(x2, 11, capi.BUF_B_JOINT, ctx.right_mul_e0_joint):.3e}", flush=True)
    x, it, st, rc = ctx.solve_joint_sc(lam, 0, 500, 1e-6)
    print(f"RIPCG eta=1e-6: {it} iterations, |Sx+b|/|b| = {residual(x, 11, capi.BUF_B_JOINT, ctx.right_mul_e0_joint):.3e}, "
          f"|x - x_direct| / |x_direct| = {np.linalg.norm(x - x2) / np.linalg.norm(x2):.3e}")
    print("device MiB:", ctx.device_bytes() >> 20)
    ctx.close()


if __name__ == "__main__":
    main()
