#!/usr/bin/env python3
"""Times the camera covariance (povar_camera_covariance_pose / _joint), the landmark covariance of every landmark
(povar_landmark_covariance_pose / _joint) and the leverage / predicted-point covariance of every observation
(povar_observation_covariance_pose / _joint) against the direct solve they share their factorisation
with (povar_solve_pose_sc / povar_solve_joint_sc_method with POVAR_SC_CHOLESKY) on a synthetic BAL shape, one process, one
context.  Device times (povar_timings.solve_ms: hipEvents on the context's stream around assembly + factorisation + back
substitution, or assembly + factorisation + inverse + per-camera Gram, or -- the landmark call -- assembly + factorisation +
inverse + W W^T + per-landmark contraction + the copy of the blocks to the host; the observation call: the landmark call's stages with
Sigma_l kept on the device, + the per-observation contraction + the copy of the rows); every call is warmed once, then timed REPS times,
the median is reported.  The hat call (povar_observation_hat_pose / _joint: residuals and hat blocks, the same walk with another row) is
timed beside the observation call of the same run, with |tr P - h| against that call's rows and rank(I - P) of the first 200 000
observations (capi.deletion_statistics).  The covariance is timed in both modes: free gauge (lambda = 0) and damped (lambda as given); a shape
that is singular beyond its gauge returns after the factorisation, which the line then says.
At this size a dense reference is out of reach; the two size-independent checks are printed instead: bitwise symmetry of every
block, (step 2, camera coordinates) the null-vector residual |block (h0 / sigma_c)| / (|block| |h0 / sigma_c|), and for the
observation rows of the free gauge sum_i h_i against rank J = dim n_cams + 3 n_lms - nq.
--pairs: instead, the covariance blocks of parameter pairs (povar_covariance_blocks_pose / _joint) beside the landmark call of the
same run: every camera with itself and with its successor, the (camera, landmark) pair of every observation of the first
100 000 landmarks, 100 000 seeded landmark-landmark pairs.
--free-first K fixes all but the first K cameras (a window; the undamped mode is then POVAR_COV_FIXED_GAUGE), --compaction 0|1|both
selects the layout of the dense matrix (set_dense_compaction; both: the two layouts alternate on the one context, three runs
each, device bytes printed after each), --short stops every report after the landmark call.
usage: bench_covariance.py [--pairs] [--free-first K] [--compaction 0|1|both] [--short] [shape] [lambda] [reps]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from povar_amd import capi, synth  # noqa: E402


def main():
    argv, opts = [], {"--free-first": None, "--compaction": "0"}
    flags = set()
    it = iter(sys.argv[1:])
    for a in it:
        if a in opts:
            opts[a] = next(it)
        elif a in ("--pairs", "--short"):
            flags.add(a)
        else:
            argv.append(a)
    pairs_mode, short = "--pairs" in flags, "--short" in flags
    free_first = None if opts["--free-first"] is None else int(opts["--free-first"])
    assert opts["--compaction"] in ("0", "1", "both"), "--compaction 0|1|both"
    layouts = [0, 1] * 3 if opts["--compaction"] == "both" else [int(opts["--compaction"])]
    shape = argv[0] if len(argv) > 0 else "venice-1778"
    lam = float(argv[1]) if len(argv) > 1 else 1e-2
    reps = int(argv[2]) if len(argv) > 2 else 3
    p = synth.make_bal_problem(shape)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs / 500.0, e0_mode=capi.E0_IMPLICIT_LDSACC)
    ctx.layout_finalize()
    ctx.timings_enable(True)
    undamped = ("free gauge", capi.COV_FREE_GAUGE, 0.0)
    if free_first is not None and free_first < p.n_cams:
        ctx.set_fixed_cameras(np.arange(free_first, p.n_cams))
        undamped = ("fixed gauge", capi.COV_FIXED_GAUGE, 0.0)
        print(f"fixed cameras: all but the first {free_first} of {p.n_cams}", flush=True)

    def timed(call):
        out = call()  # warm-up: code objects, the dense buffer
        ms = []
        for _ in range(reps):
            t0 = ctx.timings()
            out = call()
            t1 = ctx.timings()
            assert t1.solve_calls - t0.solve_calls == 1
            ms.append(t1.solve_ms - t0.solve_ms)
        return out, float(np.median(ms))

    def report(step, dim, solver, solve):
        (x, it, st, rc), ms_solve = timed(solve)
        assert rc == 0 and it == 0
        rows_now = ctx.dense_layout()[0] if hasattr(ctx.L, "povar_dense_layout") else dim * p.n_cams
        print(f"step {step} {solver} n = {rows_now} (dense rows; {p.n_cams} cameras): {ms_solve:.1f} ms per factorisation + solve (device, median of {reps})", flush=True)
        for name, gauge, lm in (undamped, ("damped", capi.COV_DAMPED, lam)):
            (cov, rc), ms = timed(lambda: ctx.camera_covariance(step=step, lam=lm, gauge=gauge, coords=capi.COV_CAMERA_COORDS))
            line = f"step {step} covariance, {name} (lambda {lm:g}): {ms:.1f} ms per call, ratio to {solver} {ms / ms_solve:.2f}"
            if rc != 0:
                print(line + f" -- rc {rc}: singular beyond the gauge, the call ended after the factorisation", flush=True)
                assert np.all(np.isnan(cov))
                continue
            sym = np.array_equal(cov, cov.transpose(0, 2, 1))
            ev = np.linalg.eigvalsh(cov[:free_first])  # (the blocks of fixed cameras are zero)
            line += f"; blocks bitwise symmetric: {sym}; smallest eigenvalue / largest, worst camera: {(ev[:, 0] / ev[:, -1]).min():.2e}"
            if step == 2 and free_first is None:
                sigma = ctx.get_buffer(capi.BUF_POSE_SCALING).reshape(-1, 12)
                ncw = ctx.get_buffer(capi.BUF_NC_HOUSEHOLDER).reshape(-1, 13)
                h0 = -ncw[:, 12:13] * ncw[:, :12] * ncw[:, 0:1]
                h0[:, 0] += 1.0
                v = h0 / sigma
                r = np.linalg.norm(np.einsum("cij,cj->ci", cov, v), axis=1) / (np.linalg.norm(cov, axis=(1, 2)) * np.linalg.norm(v, axis=1))
                line += f"; null-vector residual, worst camera: {r.max():.2e}"
            print(line, flush=True)
            mib_cam = ctx.device_bytes() >> 20
            (blocks, rc), ms_lm = timed(lambda: ctx.landmark_covariance(step=step, lam=lm, gauge=gauge, coords=capi.COV_LANDMARK_COORDS))
            assert rc == 0
            ev = np.linalg.eigvalsh(blocks)
            print(f"step {step} landmark covariance, all {p.n_lms} landmarks, {name} (lambda {lm:g}): {ms_lm:.1f} ms per call, ratio to the "
                  f"camera call {ms_lm / ms:.2f}, to {solver} {ms_lm / ms_solve:.2f}; blocks bitwise symmetric: "
                  f"{np.array_equal(blocks, blocks.transpose(0, 2, 1))}; eigenvalue {1 if step == 1 else 2} / largest, worst landmark: "
                  f"{(ev[:, 0 if step == 1 else 1] / ev[:, -1]).min():.2e}; device MiB {mib_cam} -> {ctx.device_bytes() >> 20}", flush=True)
            if short:
                continue
            mib_lm = ctx.device_bytes() >> 20
            (rows, rc), ms_obs = timed(lambda: ctx.observation_covariance(step=step, lam=lm, gauge=gauge))
            assert rc == 0
            line = (f"step {step} observation covariance, all {rows.shape[0]} observations, {name} (lambda {lm:g}): {ms_obs:.1f} ms per call, "
                    f"ratio to the landmark call {ms_obs / ms_lm:.2f}, to {solver} {ms_obs / ms_solve:.2f}; leverage in "
                    f"[{rows[:, 0].min():.3g}, {rows[:, 0].max():.3g}] (d = {4 if step == 1 else 2})")
            if gauge == capi.COV_FREE_GAUGE:
                rank = dim * p.n_cams + 3 * p.n_lms - (12 if step == 1 else 15)  # (fixed gauge: the line is not printed)
                line += f"; sum h = {np.sum(rows[:, 0].astype(np.longdouble)):.6f}, rank J = {rank}"
            print(line + f"; finite c_*: {bool(np.all(np.isfinite(rows[:, 1:])))}; device MiB {mib_lm} -> {ctx.device_bytes() >> 20}", flush=True)
            # the hat call beside the observation call of the same run: the same walk, another row (14 or 5 numbers instead of 4)
            mib_obs = ctx.device_bytes() >> 20
            (r, P, rc), ms_hat = timed(lambda: ctx.observation_hat(step=step, lam=lm, gauge=gauge))
            assert rc == 0
            d = r.shape[1]
            tr = np.trace(P, axis1=1, axis2=2)
            n_stat = min(200000, r.shape[0])
            t, rk = capi.deletion_statistics(r[:n_stat], P[:n_stat])
            print(f"step {step} observation hat, all {r.shape[0]} observations, {name} (lambda {lm:g}): {ms_hat:.1f} ms per call, ratio to the "
                  f"observation call {ms_hat / ms_obs:.2f}, to {solver} {ms_hat / ms_solve:.2f}; worst |tr P - h| {np.abs(tr - rows[:, 0]).max():.2e}; "
                  f"blocks bitwise symmetric: {np.array_equal(P, P.transpose(0, 2, 1))}; rank(I - P) of the first {n_stat}: "
                  f"{np.bincount(rk, minlength=d + 1).tolist()}; device MiB {mib_obs} -> {ctx.device_bytes() >> 20}", flush=True)

    def pair_requests():
        """The three requests of --pairs: every camera with itself and with its successor; the (camera, landmark) pair of every
        observation of the first 100 000 landmarks; 100 000 seeded landmark-landmark pairs."""
        cam = np.arange(p.n_cams)
        cc = np.zeros((2 * p.n_cams, 4), dtype=np.int32)
        cc[:, 1] = np.repeat(cam, 2)
        cc[0::2, 3], cc[1::2, 3] = cam, (cam + 1) % p.n_cams
        n_l = min(100000, p.n_lms)
        n_o = int(p.lm_off[n_l])
        cl = np.zeros((n_o, 4), dtype=np.int32)
        cl[:, 1], cl[:, 2], cl[:, 3] = p.cam_idx[:n_o], capi.COV_BLOCK_LANDMARK, np.repeat(np.arange(n_l), np.diff(p.lm_off[:n_l + 1]))
        ll = np.full((100000, 4), capi.COV_BLOCK_LANDMARK, dtype=np.int32)
        ll[:, 1::2] = np.random.default_rng(17).integers(0, p.n_lms, size=(100000, 2))
        return (("camera-camera", cc), ("camera-landmark", cl), ("landmark-landmark", ll))

    def report_pairs(step, dim, solver, solve):
        """--pairs: the three requests beside the landmark call of the same run (it shares the factorisation, the inversion and
        cov_lauum with them: the difference is the pair kernels and the copy of the blocks)."""
        for name, gauge, lm in (undamped, ("damped", capi.COV_DAMPED, lam)):
            (blocks, rc), ms_lm = timed(lambda: ctx.landmark_covariance(step=step, lam=lm, gauge=gauge, coords=capi.COV_LANDMARK_COORDS))
            line = f"step {step} landmark covariance, all {p.n_lms} landmarks, {name} (lambda {lm:g}): {ms_lm:.1f} ms per call"
            if rc != 0:
                print(line + f" -- rc {rc}: singular beyond the gauge, the call ended after the factorisation", flush=True)
                continue
            print(line, flush=True)
            for kind, pairs in pair_requests():
                fn = ctx.L.povar_covariance_blocks_pose if step == 1 else ctx.L.povar_covariance_blocks_joint
                side = np.array([12, 3 if step == 1 else 4])
                n_out = int((side[pairs[:, 0]] * side[pairs[:, 2]]).sum())
                out = np.zeros(n_out)

                def call():  # (the raw call: capi.Context.covariance_blocks would cut a list of 10^5 arrays on the host)
                    return out, fn(ctx.h, capi.C.c_double(lm), capi.C.c_int32(gauge), capi.C.c_int32(capi.COV_CAMERA_COORDS),
                                   capi.C.c_void_p(pairs.ctypes.data), capi.C.c_int32(pairs.shape[0]), capi.C.c_void_p(out.ctypes.data),
                                   capi.C.c_int64(n_out))

                (_, rc), ms = timed(call)
                assert rc == 0 and np.all(np.isfinite(out))
                print(f"step {step} covariance blocks, {pairs.shape[0]} {kind} pairs ({n_out} numbers), {name}: {ms:.1f} ms per call, ratio to "
                      f"the landmark call {ms / ms_lm:.2f}, difference {ms - ms_lm:+.1f} ms; device MiB {ctx.device_bytes() >> 20}", flush=True)

    if pairs_mode:
        report = report_pairs
    report_one = report

    def report(step, dim, solver, solve):  # every layout of --compaction in turn, on the one context
        new = hasattr(ctx.L, "povar_set_dense_compaction")  # (POVAR_LIB may name a library from before the switch)
        for layout in layouts:
            if new:
                ctx.set_dense_compaction(layout)
            print(f"step {step} compaction {layout}:", flush=True)
            report_one(step, dim, solver, solve)
            print(f"step {step} compaction {layout}: dense rows {ctx.dense_layout()[0] if new else dim * p.n_cams}, "
                  f"device bytes {ctx.device_bytes()}", flush=True)
    # step 1 in the units of the normalised observations (the first two rows of every P divided by 500)
    cams1 = p.cams.copy()
    cams1[:, :8] /= 500.0
    ctx.set_cameras(cams1)
    ctx.init_landmarks_pose(0.01)
    ctx.set_jl_col_scaling(False)
    assert ctx.linearize_pose(0.01)
    report(1, 12, "CHOLESKY", lambda: ctx.solve_pose_sc(lam, capi.SC_CHOLESKY))
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
    report(2, 11, "RICHOLESKY", lambda: ctx.solve_joint_sc(lam, method=capi.SC_CHOLESKY))
    print("device MiB:", ctx.device_bytes() >> 20)
    ctx.close()


if __name__ == "__main__":
    main()
