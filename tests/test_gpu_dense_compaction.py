"""The compacted dense system (povar_set_dense_compaction) on the device, through the C ABI: in mode 1 the dense matrix of
CHOLESKY / RICHOLESKY and of every covariance family spans the free cameras only.

References and bounds are the existing ones (tests/compaction_reference.py): sc_bounds.factor_check on the system restricted
to the free coordinates for the factor and the solve, fixed_cameras_reference.CovCase -- whose outputs do not depend on the
layout -- for the covariance calls, with the bounds of tests/test_gpu_fixed_cameras.py::test_covariance.  The cases and what
each of them hits are listed in compaction_reference; tests/test_dense_compaction_cpu.py holds every S_ff to cond_2 <= 1e4.
Every figure is printed before it is asserted.
"""
import os
import subprocess
import threading

import numpy as np
import pytest

import compaction_reference as CR
import covariance_reference as R
import fixed_cameras_reference as FR
import landmark_covariance_reference as L
import sc_bounds as SB
from test_gpu_sharded import HostAllReduce

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = CR.LAM


def _solver_context(p, mode, F, assembly=2):
    """A context on an sc_bounds case (OB.Pose / OB.Joint), as tests/test_gpu_fixed_cameras.py::test_cholesky sets it."""
    from povar_amd import capi
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    ctx.set_sc_assembly(assembly)
    ctx.set_dense_compaction(mode)
    ctx.set_fixed_cameras(F)
    ctx.set_cameras(p.cams)
    return ctx


def _solve(ctx, p, step):
    from povar_amd import capi
    if step == 1:
        ctx.set_landmarks(p.lms)
        ctx.set_jl_col_scaling(False)
        assert ctx.linearize_pose(p.alpha)
        return ctx.solve_pose_sc(p.lam, capi.SC_CHOLESKY)
    ctx.set_landmarks_homogeneous(p.lms)
    assert ctx.linearize_homogeneous()
    return ctx.solve_joint_sc(p.lam, method=capi.SC_CHOLESKY)


def _check_factor(tag, sy, buf, inc, F):
    """(5) of the factor and the solve on the compact buffer: the bounds of sc_bounds.factor_check on the restricted system, exact
    padding, inc[free] == x[:n] bit for bit, inc exactly zero on F."""
    fc = SB.factor_check(sy, buf)
    pad = fc.pop("padding")
    print(f"SCBOUND compact {tag} padding messages: {pad}")
    assert not pad
    for what, (err, bound) in fc.items():
        r, i, over = SB.worst(err, bound)
        print(f"SCBOUND compact {tag} {what}={r:.3g}")
        assert not over, (tag, what, r, i)
    x = buf[:, sy.N + 1]
    k = FR.fixed_coords(sy.p.n_cams, sy.dim, F)
    assert np.array_equal(inc[sy.free], x[:sy.n])
    assert np.all(inc[k] == 0.0) and not np.any(np.signbit(inc[k]))


# ------------------------------------------------------------------------------------------ 5. factor and solve
@pytest.mark.parametrize("assembly", [1, 2], ids=["atomic", "ordered"])
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("case", list(CR.CASES))
def test_factor_and_solve(case, step, assembly):
    from povar_amd import capi
    sy = CR.dense_case(case, step)
    p, F, dim = sy.p, CR.fixed_of(case), sy.dim
    assert sy.n == CR.rows_of(case, step)
    ctx = _solver_context(p, 1, F, assembly)
    assert ctx.dense_compaction() == 1 and ctx.dense_layout()[0] == 0
    inc, it, status, rc = _solve(ctx, p, step)
    assert rc == 0 and it == 0 and status == capi.SUCCESS and ctx.sc_assembly() == assembly
    n, rows = ctx.dense_layout()
    n_want, rows_want = CR.expected_map(p.n_cams, dim, F, 1)
    print(f"{case} step {step}: compact rows {n} (full {dim * p.n_cams}), N = {sy.N}")
    assert n == n_want == sy.n and np.array_equal(rows, rows_want)
    buf = ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
    assert buf.shape == (sy.N, sy.N + 2)
    _check_factor(f"{case} step {step} assembly {assembly}", sy, buf, inc, F)
    if assembly == 2:
        inc2, _, _, rc2 = _solve(ctx, p, step)
        assert rc2 == 0 and np.array_equal(inc2, inc)
        assert np.array_equal(ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2), buf)
    ctx.close()


# ------------------------------------------------------------------------------------------ 6. F empty
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("case", ["small", "p22"])
def test_empty_set_is_mode_0(case, step):
    """No fixed camera: mode 1 returns the bits of mode 0 for the increment, POVAR_BUF_SC_FACTOR and a free-gauge camera +
    landmark call; the map is dim c."""
    from povar_amd import capi
    sy = CR.full_system(CR.problem_of(case), step)
    p = sy.p
    got = []
    for mode in (0, 1):
        ctx = _solver_context(p, mode, [])
        inc, it, status, rc = _solve(ctx, p, step)
        assert rc == 0
        n, rows = ctx.dense_layout()
        assert n == sy.dim * p.n_cams and np.array_equal(rows, sy.dim * np.arange(p.n_cams))
        buf = ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
        lm, cam, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=capi.COV_FREE_GAUGE, with_cameras=True)
        assert rc == 0
        got.append((inc, buf, lm, cam))
        ctx.close()
    for a, b in zip(*got):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------ 7. suffix F
@pytest.mark.parametrize("step", [1, 2])
def test_suffix_set_is_a_leading_block(step):
    """F the last four cameras of p24, ordered assembly: R[:n, :n] and y[:n] of mode 1 are mode 0's leading rows and columns bit
    for bit (every entry's arithmetic depends on its position and the rows above it)."""
    from povar_amd import capi
    sy = CR.dense_case("p24s", step)
    p, F, n = sy.p, CR.fixed_of("p24s"), sy.n
    bufs = []
    for mode in (0, 1):
        ctx = _solver_context(p, mode, F)
        inc, it, status, rc = _solve(ctx, p, step)
        assert rc == 0
        bufs.append(ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2))
        ctx.close()
    full, compact = bufs
    N0, N1 = full.shape[0], compact.shape[0]
    print(f"p24s step {step}: n = {n}, N = {N1} (mode 0: {N0})")
    assert N1 == sy.N and N0 == SB.padded(sy.dim * p.n_cams)
    assert np.array_equal(np.triu(compact[:n, :n]), np.triu(full[:n, :n]))
    assert np.array_equal(compact[:n, N1], full[:n, N0])


# ------------------------------------------------------------------------------------------ 8. covariance
def _cov_context(case, step, mode, F):
    """As tests/test_gpu_fixed_cameras.py::_cov_context."""
    from povar_amd import capi
    p = CR.synth_problem(CR.problem_of(case))
    cams, lms, obs = L.state(p, step)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs)
    ctx.set_dense_compaction(mode)
    ctx.set_fixed_cameras(F)
    ctx.set_cameras(cams)
    if step == 1:
        ctx.set_landmarks(lms)
        assert ctx.linearize_pose(L.ALPHA)
    else:
        ctx.set_landmarks_homogeneous(lms)
        assert ctx.linearize_homogeneous()
    return ctx


def _block_err(got, want):
    return np.linalg.norm((np.asarray(got).astype(np.longdouble) - want).astype(np.float64), axis=(-2, -1))


def _pairs_of(case, step, s, F, rows):
    """Sampled pairs of every kind, pairs with members in F, a camera pair across two 64-blocks of the compact matrix and one
    inside a single block, both orders of some; for the window also landmarks without a free camera."""
    import pair_covariance_reference as PC
    rng = np.random.default_rng(step)
    cc, cl, ll = PC.sample_pairs(rng, s.n_cams, s.n_lms, 10)
    free = [c for c in range(s.n_cams) if c not in F]
    l0 = int(rng.integers(0, s.n_lms))
    extra = [(0, F[0], 0, F[-1]), (0, F[0], 0, free[0]), (0, free[0], 0, F[-1]), (0, F[0], 1, l0), (1, l0, 0, F[-1]), (0, F[-1], 0, F[-1]),
             (0, free[0], 0, free[0]), (0, free[-1], 1, l0), (1, l0, 0, free[0])]
    blk = lambda c, e: (int(rows[c]) + e) >> 6
    inside = [(a, b) for a in free for b in free if a < b and blk(a, 0) == blk(a, s.dim - 1) == blk(b, 0) == blk(b, s.dim - 1)]
    across = [(a, b) for a in free for b in free if a < b and blk(a, s.dim - 1) < blk(b, 0)]
    assert inside, case
    extra += [(0, inside[0][0], 0, inside[0][1]), (0, inside[0][1], 0, inside[0][0])]
    if s.dim * len(free) > 64:
        assert across, case
        extra += [(0, across[-1][0], 0, across[-1][1]), (0, across[-1][1], 0, across[-1][0])]
    return cc + cl + ll + extra


@pytest.mark.parametrize("gauge_mode", ["fixed", "damped"])
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("case", ["small", "p22", "p40", "p40w"])
def test_covariance(case, step, gauge_mode):
    """Camera, landmark, pair, observation and hat outputs of mode 1 against the references and bounds of
    tests/test_gpu_fixed_cameras.py::test_covariance: n u cond_2(S_ff) |S_ff^-1|_2 per camera block, the reference modules' rule
    for the others; blocks with a member in F exactly zero; every block symmetric bit for bit, (b, a) the bitwise transpose of
    (a, b); in the fixed gauge sum h_i = DIM (n_cams - |F|) + 3 n_lms inside the summed bound."""
    from povar_amd import capi
    F = CR.fixed_of(case)
    lam, gauge = (0.0, capi.COV_FIXED_GAUGE) if gauge_mode == "fixed" else (LAM, capi.COV_DAMPED)
    ref = CR.cov_case(case, step, lam)
    s = ref.sys
    ctx = _cov_context(case, step, 1, F)
    tag = f"compact {gauge_mode} step {step} {case}"
    n_want, rows_want = CR.expected_map(s.n_cams, s.dim, F, 1)
    pairs = _pairs_of(case, step, s, F, rows_want)
    for coords in (capi.COV_SOLVER_COORDS, capi.COV_CAMERA_COORDS):
        lm, cam, rc = ctx.landmark_covariance(step=step, lam=lam, gauge=gauge, coords=coords, with_cameras=True)
        n, rows = ctx.dense_layout()
        cam_only, rc2 = ctx.camera_covariance(step=step, lam=lam, gauge=gauge, coords=coords)
        print(f"{tag} coords {coords}: rc {rc} {rc2}, compact rows {n}")
        assert rc == 0 and rc2 == 0, tag
        assert n == n_want == CR.rows_of(case, step) and np.array_equal(rows, rows_want)
        param = coords == capi.COV_CAMERA_COORDS
        want = R.to_camera_coords(ref.cam_blocks, s.sigma, step, s.cams) if param else ref.cam_blocks
        bound = ref.cam_bound * (float(s.sigma.max() ** 2) if param else 1.0)
        for got in (cam, cam_only):
            assert got.shape == want.shape and np.all(np.isfinite(got))
            err = _block_err(got, want)
            print(f"{tag} coords {coords}: camera blocks worst {err.max():.3e} (bound {bound:.3e})")
            assert np.all(err <= bound), (tag, err.max(), bound)
            assert np.all(got[F] == 0.0) and np.array_equal(got, got.transpose(0, 2, 1))
        want = s.to_landmark_coords(ref.lm_blocks) if param else ref.lm_blocks
        scale = float(s.s.max() ** 2) if param else 1.0
        err = _block_err(lm, want)
        print(f"{tag} coords {coords}: landmark blocks worst {err.max():.3e} (bound {ref.full_bound * scale:.3e})")
        assert lm.shape == want.shape and np.all(err <= ref.full_bound * scale), (tag, err.max())
        assert np.array_equal(lm, lm.transpose(0, 2, 1))
        blocks, rc = ctx.covariance_blocks(pairs, step=step, lam=lam, gauge=gauge, coords=coords)
        assert rc == 0
        worst, seen = 0.0, {}
        for pair, got in zip(pairs, blocks):
            want = ref.pairs.want(pair, param)
            bound = ref.full_bound * ref.pairs.scale(pair, param)
            e = float(_block_err(got, want))
            worst = max(worst, e / bound)
            assert got.shape == want.shape and e <= bound, (tag, pair, e, bound)
            if (pair[0] == 0 and pair[1] in F) or (pair[2] == 0 and pair[3] in F):
                assert np.all(got == 0.0), (tag, pair)
            if pair[:2] == pair[2:]:
                assert np.array_equal(got, got.T), (tag, pair)
            seen[tuple(pair)] = got
            back = seen.get((pair[2], pair[3], pair[0], pair[1]))
            if back is not None:
                assert np.array_equal(got, back.T), (tag, pair)
        print(f"{tag} coords {coords}: pair blocks worst err / bound {worst:.3g}")
    rows_o, rc = ctx.observation_covariance(step=step, lam=lam, gauge=gauge)
    assert rc == 0 and rows_o.shape == ref.obs_rows.shape and np.all(np.isfinite(rows_o[:, 0]))
    err = np.abs((rows_o.astype(np.longdouble) - ref.obs_rows).astype(np.float64))
    print(f"{tag}: observation rows worst err / bound {np.max(err / np.maximum(ref.obs_bound, 1e-300)):.3g}; sum h = {rows_o[:, 0].sum():.12f}, "
          f"free parameters {ref.rank}, summed bound {ref.obs_bound[:, 0].sum():.3e}")
    assert np.all(err <= ref.obs_bound), tag
    if gauge_mode == "fixed":
        assert ref.rank == s.dim * (s.n_cams - len(F)) + 3 * s.n_lms
        assert abs(rows_o[:, 0].sum() - ref.rank) <= ref.obs_bound[:, 0].sum(), tag
    r, P, rc = ctx.observation_hat(step=step, lam=lam, gauge=gauge)
    assert rc == 0 and P.shape == ref.hat_blocks.shape and np.all(np.isfinite(P))
    err = np.abs((P.astype(np.longdouble) - ref.hat_blocks).astype(np.float64))
    print(f"{tag}: hat blocks worst err / bound {np.max(err / np.maximum(ref.hat_bound, 1e-300)):.3g}")
    assert np.all(err <= ref.hat_bound) and np.array_equal(P, P.transpose(0, 2, 1)), tag
    if case == "p40w":
        # landmarks without a free camera: every entry of C they read is zero, so the block is Hll^-1 alone (solver coordinates)
        # and their observations' rows come from the landmark alone: the covariance of (camera, landmark) is diag(0, Hll^-1)
        osys = ref.osys
        free = np.setdiff1d(np.arange(s.n_cams), F)
        lone = [l for l in range(s.n_lms) if not np.isin(osys.cam_idx[osys.lm_off[l]:osys.lm_off[l + 1]], free).any()]
        assert len(lone) == 148
        lm1, rc = ctx.landmark_covariance(step=step, lam=lam, gauge=gauge, coords=capi.COV_SOLVER_COORDS, ids=lone)
        hi_all = s.hll_inv(lam)
        hi = np.stack([hi_all[l] for l in lone])
        err = _block_err(lm1, hi)
        print(f"{tag}: {len(lone)} landmarks without a free camera against Hll^-1: worst {err.max():.3e} (bound {ref.full_bound:.3e})")
        assert rc == 0 and np.all(err <= ref.full_bound)
        rows_l, rc = ctx.observation_covariance(step=step, lam=lam, gauge=gauge, lm_ids=lone)
        r_l, P_l, rc2 = ctx.observation_hat(step=step, lam=lam, gauge=gauge, lm_ids=lone)
        assert rc == 0 and rc2 == 0
        idx = np.concatenate([np.arange(osys.lm_off[l], osys.lm_off[l + 1]) for l in lone])
        assert rows_l.shape[0] == idx.shape[0] == P_l.shape[0]
        want_rows = np.zeros((idx.shape[0], 4), dtype=np.longdouble)
        want_hat = np.zeros((idx.shape[0], osys.d, osys.d), dtype=np.longdouble)
        for k, i in enumerate(idx):
            cov = np.zeros((s.dim + 3, s.dim + 3), dtype=np.longdouble)
            cov[s.dim:, s.dim:] = hi_all[osys.lm_of[i]]
            want_rows[k] = osys._row(i, cov)
            Jw = osys.rows(i).astype(np.longdouble)
            want_hat[k] = Jw @ cov @ Jw.T
        e_rows = np.abs((rows_l.astype(np.longdouble) - want_rows).astype(np.float64))
        e_hat = np.abs((P_l.astype(np.longdouble) - want_hat).astype(np.float64))
        print(f"{tag}: rows of those landmarks from the landmark alone: observation rows worst err / bound "
              f"{np.max(e_rows / np.maximum(ref.obs_bound[idx], 1e-300)):.3g}, hat blocks {np.max(e_hat / np.maximum(ref.hat_bound[idx], 1e-300)):.3g}")
        assert np.all(e_rows <= ref.obs_bound[idx]) and np.all(e_hat <= ref.hat_bound[idx])
        assert np.array_equal(rows_l, rows_o[idx]) and np.array_equal(P_l, P[idx])  # (the request by ids returns the same rows)
    with pytest.raises(capi.PovarError):  # no gauge basis was built
        ctx.get_buffer(capi.BUF_COV_GAUGE, joint=step == 2)
    ctx.close()


# ------------------------------------------------------------------------------------------ 9. every camera fixed
@pytest.mark.parametrize("step", [1, 2])
def test_every_camera_fixed(step):
    """n = 0: no matrix and no factorisation; the solve returns +0.0 with status 0 and SUCCESS; the covariance calls return mode
    0's status, zero camera blocks and mode 0's landmark, observation, hat and pair outputs; the dense buffers are argument errors."""
    from povar_amd import capi
    sy = CR.full_system("small", step)
    p = sy.p
    F = list(range(p.n_cams))
    ctx = _solver_context(p, 1, F)
    bytes0 = ctx.device_bytes()
    inc, it, status, rc = _solve(ctx, p, step)
    assert rc == 0 and it == 0 and status == capi.SUCCESS
    assert np.all(inc == 0.0) and not np.any(np.signbit(inc))
    n, rows = ctx.dense_layout()
    assert n == 0 and np.all(rows == -1)
    with pytest.raises(capi.PovarError, match="POVAR_BUF_SC_FACTOR"):
        ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
    # nothing of the size of a dense matrix was allocated (the full one: 8 (N + 64) (N + 128) bytes)
    N = SB.padded(sy.dim * p.n_cams)
    grown = ctx.device_bytes() - bytes0
    print(f"every camera fixed, step {step}: device bytes grew by {grown} (a full matrix: {8 * (N + 64) * (N + 128)})")
    assert grown < 8 * (N + 64) * (N + 128)
    ctx.close()
    pairs = [(0, 0, 0, 1), (0, 2, 1, 3), (1, 3, 0, 2), (1, 4, 1, 4), (1, 5, 1, 9), (0, 3, 0, 3)]
    for lam, gauge in ((0.0, capi.COV_FIXED_GAUGE), (LAM, capi.COV_DAMPED)):
        out = []
        for mode in (0, 1):
            ctx = _cov_context("small", step, mode, F)
            lm, cam, rc = ctx.landmark_covariance(step=step, lam=lam, gauge=gauge, with_cameras=True)
            cam_only, rc1 = ctx.camera_covariance(step=step, lam=lam, gauge=gauge)
            rows_o, rc2 = ctx.observation_covariance(step=step, lam=lam, gauge=gauge)
            r, P, rc3 = ctx.observation_hat(step=step, lam=lam, gauge=gauge)
            blocks, rc4 = ctx.covariance_blocks(pairs, step=step, lam=lam, gauge=gauge)
            print(f"every camera fixed, step {step}, gauge {gauge}, mode {mode}: status {rc} {rc1} {rc2} {rc3} {rc4}")
            assert np.all(cam == 0.0) and np.all(cam_only == 0.0)
            if mode == 1:
                assert ctx.dense_layout()[0] == 0
                for w in (capi.BUF_COV_INVERSE, capi.BUF_COV_PANEL, capi.BUF_COV_FACTOR):
                    with pytest.raises(capi.PovarError, match="POVAR_BUF_COV"):
                        ctx.get_buffer(w, joint=step == 2)
            out.append(((rc, rc1, rc2, rc3, rc4), [lm, cam, cam_only, rows_o, r, P] + list(blocks)))
            ctx.close()
        assert out[0][0] == out[1][0] == (0, 0, 0, 0, 0)
        for a, b in zip(out[0][1], out[1][1]):
            assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------ 10. switching on one context
def test_switching_on_one_context():
    """One context, at the covariance tests' state of p22 (step 1): mode 0 solve -> mode 1 solve -> new F -> mode 1 covariance ->
    mode 0 covariance -> mode 1 solve.  Each call answers for the mode and the set in force, inside the bounds of (5) (the
    solver reference built at this state: compaction_reference.cov_state_system) and of (8); the dense buffers follow the layout
    of the call before them."""
    from povar_amd import capi
    step = 1
    F1, F2 = CR.fixed_of("p22"), [0, 7, 21]
    full = CR.cov_state_system("p22")
    p = full.p
    ctx = _cov_context("p22", step, 0, F1)
    solve = lambda: ctx.solve_pose_sc(LAM, capi.SC_CHOLESKY)
    inc0, _, _, rc = solve()
    n, rows = ctx.dense_layout()
    assert rc == 0 and n == 12 * p.n_cams and ctx.get_buffer(capi.BUF_SC_FACTOR).shape[0] == SB.padded(n)
    ctx.set_dense_compaction(1)
    assert ctx.dense_layout()[0] == n  # (the layout of the last dense call, not of the next)
    inc1, _, _, rc = solve()
    assert rc == 0
    _check_factor("switch p22 mode 1", CR.restrict(full, F1), ctx.get_buffer(capi.BUF_SC_FACTOR), inc1, F1)
    err = np.abs(inc1 - inc0).max() / np.abs(inc0).max()
    print(f"switching: mode 1 against mode 0 increment, relative {err:.3e}")
    assert err < 1e-8  # (tests/test_gpu_sc_solvers.py::test_cholesky_pose's tolerance between two solves of one system)
    ctx.set_fixed_cameras(F2)
    ref = FR.cov_case("p22", step, 0.0, F2)
    for mode in (1, 0):
        ctx.set_dense_compaction(mode)
        lm, cam, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=capi.COV_FIXED_GAUGE, coords=capi.COV_SOLVER_COORDS, with_cameras=True)
        n, rows = ctx.dense_layout()
        e_cam, e_lm = _block_err(cam, ref.cam_blocks).max(), _block_err(lm, ref.lm_blocks).max()
        print(f"switching: covariance mode {mode}: rows {n}, camera {e_cam:.3e} (bound {ref.cam_bound:.3e}), landmark {e_lm:.3e} (bound {ref.full_bound:.3e})")
        assert rc == 0 and np.array_equal(rows, CR.expected_map(ref.n_cams, 12, F2, mode)[1])
        assert e_cam <= ref.cam_bound and e_lm <= ref.full_bound and np.all(cam[F2] == 0.0)
        assert ctx.get_buffer(capi.BUF_COV_INVERSE).shape == (SB.padded(n), SB.padded(n))
        assert ctx.get_buffer(capi.BUF_COV_PANEL).shape == (SB.padded(n), 64)
        with pytest.raises(capi.PovarError, match="POVAR_BUF_SC_FACTOR"):
            ctx.get_buffer(capi.BUF_SC_FACTOR)
        rows_o, rc = ctx.observation_covariance(step=step, lam=0.0, gauge=capi.COV_FIXED_GAUGE)
        e_obs = np.abs((rows_o.astype(np.longdouble) - ref.obs_rows).astype(np.float64))
        print(f"switching: covariance mode {mode}: observation rows worst err / bound {np.max(e_obs / np.maximum(ref.obs_bound, 1e-300)):.3g}")
        assert rc == 0 and np.all(e_obs <= ref.obs_bound)
    # and back to a compact solve with the new set: the factor is handed out again, the covariance buffers are not
    ctx.set_dense_compaction(1)
    inc2, _, _, rc = solve()
    assert rc == 0 and np.array_equal(ctx.dense_layout()[1], CR.expected_map(p.n_cams, 12, F2, 1)[1])
    _check_factor("switch p22 new F", CR.restrict(full, F2), ctx.get_buffer(capi.BUF_SC_FACTOR), inc2, F2)
    with pytest.raises(capi.PovarError, match="POVAR_BUF_COV"):
        ctx.get_buffer(capi.BUF_COV_INVERSE)
    ctx.close()


# ------------------------------------------------------------------------------------------ 11. failure modes carried over
@pytest.mark.parametrize("step", [1, 2])
def test_failure_modes(step):
    import ctypes as C
    from povar_amd import capi
    ctx = _cov_context("small", step, 1, [0])
    got, rc = ctx.camera_covariance(step=step, lam=0.0, gauge=capi.COV_FIXED_GAUGE)
    assert rc == capi.NUMERIC_FAILURE and np.all(np.isnan(got))
    lm, cam, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=capi.COV_FIXED_GAUGE, with_cameras=True)
    assert rc == capi.NUMERIC_FAILURE and np.all(np.isnan(lm)) and np.all(np.isnan(cam))
    blocks, rc = ctx.covariance_blocks([(0, 1, 0, 2), (0, 0, 1, 3)], step=step, lam=0.0, gauge=capi.COV_FIXED_GAUGE)
    assert rc == capi.NUMERIC_FAILURE and all(np.all(np.isnan(b)) for b in blocks)
    for bad in (2, -1, 7):
        assert ctx.L.povar_set_dense_compaction(ctx.h, C.c_int32(bad)) < 0
        assert b"povar_set_dense_compaction" in ctx.L.povar_last_error() and ctx.dense_compaction() == 1
    ctx.set_fixed_cameras([0, 1])
    got, rc = ctx.camera_covariance(step=step, lam=0.0, gauge=capi.COV_FIXED_GAUGE)
    assert rc == 0 and np.all(np.isfinite(got)) and np.all(got[[0, 1]] == 0.0)
    with pytest.raises(capi.PovarError, match="POVAR_BUF_SC_FACTOR"):
        ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
    ctx.close()


# ------------------------------------------------------------------------------------------ 12. memory
def test_memory_follows_the_window():
    """Two fresh contexts on p40w that differ in the mode alone, after the same CHOLESKY call: the compact one holds at least
    8 (count(N0) - count(N1)) bytes less (count: the doubles dense_dims allocates for N), less the bytes of the map."""
    sy = CR.dense_case("p40w", 1)
    p, F = sy.p, CR.fixed_of("p40w")
    held = []
    for mode in (0, 1):
        ctx = _solver_context(p, mode, F)
        inc, _, _, rc = _solve(ctx, p, 1)
        assert rc == 0
        held.append(ctx.device_bytes())
        ctx.close()
    count = lambda N: (N + 64) * (N + 128)
    N0, N1 = SB.padded(12 * p.n_cams), sy.N
    want = 8 * (count(N0) - count(N1)) - 4 * p.n_cams
    print(f"p40w: device bytes {held[0]} (mode 0, N = {N0}) and {held[1]} (mode 1, N = {N1}): saved {held[0] - held[1]}, at least {want}")
    assert held[0] - held[1] >= want


# ------------------------------------------------------------------------------------------ 13. two shards
def test_two_shards():
    """p22 split by povar_shard_range, two contexts on one device over the host hook, mode 1, ordered assembly: both ranks return
    the same bits, inside the bounds of (5) for two shards."""
    from povar_amd import capi
    step = 1
    sy = CR.dense_case("p22", step, shards=2)
    p, F = sy.p, CR.fixed_of("p22")
    world = 2
    ar = HostAllReduce(world)
    out = [None] * world

    def worker(rank):
        try:
            lb, le = capi.shard_range(p.lm_off, world, rank)
            ob, oe = int(p.lm_off[lb]), int(p.lm_off[le])
            ctx = capi.Context(p.n_cams, p.lm_off[lb:le + 1] - p.lm_off[lb], p.cam_idx[ob:oe], p.obs[ob:oe])
            ctx.comm_init_host(world, rank, ar.fn(rank))
            ctx.set_sc_assembly(2)
            ctx.set_dense_compaction(1)
            ctx.set_fixed_cameras(F)
            ctx.set_cameras(p.cams)
            ctx.set_landmarks(p.lms[lb:le])
            ctx.set_jl_col_scaling(False)
            assert ctx.linearize_pose(p.alpha)
            inc, _, _, rc = ctx.solve_pose_sc(p.lam, capi.SC_CHOLESKY)
            assert rc == 0
            out[rank] = (inc, ctx.get_buffer(capi.BUF_SC_FACTOR), ctx.dense_layout())
            ctx.close()
        except BaseException:
            ar.bar.abort()  # a failed rank must not leave the other one waiting
            raise

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert all(o is not None for o in out)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert out[0][2][0] == out[1][2][0] == sy.n and np.array_equal(out[0][2][1], out[1][2][1])
    _check_factor("two shards p22", sy, out[0][1], out[0][0], F)


# ------------------------------------------------------------------------------------------ 14. bal
def test_bal_compact_fixed_cameras(tmp_path):
    """`bal --fixed-cameras 0,1 --compact-fixed-cameras` with the direct solvers of both steps on the problem of
    tests/test_gpu_fixed_cameras.py::test_bal_fixed_cameras: the accept / reject sequence of the run without the flag, a final
    cost that agrees with it, finite covariance blocks, zero on the fixed cameras."""
    import json
    from povar_amd import synth
    p = synth.make_problem(10, 300, 1300, seed=21, init="gt", init_noise=0.01)
    p.cams[:2] = synth.make_problem(10, 300, 1300, seed=21, init="gt", init_noise=0.0).cams[:2]
    f = str(tmp_path / "problem-10-300.txt")
    synth.write_data_custom(f, p)
    runs = []
    for tag, extra in (("full", []), ("compact", ["--compact-fixed-cameras"])):
        out, log = str(tmp_path / f"cov-{tag}.txt"), str(tmp_path / f"log-{tag}.json")
        cmd = [os.path.join(ROOT, "bin/bal"), "--input", f, "--quiet", "--max-num-iterations-step-1", "6", "--max-num-iterations-step-2", "3",
               "--log-log-path", log, "--fixed-cameras", "0,1", "--solver-type-step-1", "CHOLESKY",
               "--solver-type-step-2", "RICHOLESKY", "--camera-covariance-path", out] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "fixed cameras: 2 of 10\n" in r.stdout and ("dense system: compacted to the 8 free cameras\n" in r.stdout) == bool(extra)
        assert "[WARN]" not in r.stdout
        lines = open(out).read().split("\n")
        head = lines[0].split()
        assert int(head[0]) == p.n_cams and "fixed-gauge" in head[1:]
        blocks = np.array([[float(x) for x in ln.split()] for ln in lines[1:1 + p.n_cams]]).reshape(p.n_cams, 12, 12)
        assert np.all(blocks[:2] == 0.0)
        assert np.all(np.isfinite(blocks[2:])) and np.array_equal(blocks, blocks.transpose(0, 2, 1))
        assert np.all(np.linalg.norm(blocks[2:], axis=(1, 2)) > 0)
        runs.append((json.load(open(log)), blocks))
    (d0, blocks0), (d1, blocks1) = runs
    c0, c1 = float(d0["cost"][-1]), float(d1["cost"][-1])
    print(f"bal: accept sequence {d0['step_is_successful']} / {d1['step_is_successful']}, final cost {c0:.12e} / {c1:.12e}")
    assert d0["iteration"] == d1["iteration"] and d0["step_is_successful"] == d1["step_is_successful"]
    # (the tolerance tests/test_gpu_baseline_sizes.py holds the costs of two programs on one problem to)
    assert abs(c0 - c1) <= 1e-6 * abs(c0)
    rel = np.abs(blocks1 - blocks0).max() / np.abs(blocks0).max()
    print(f"bal: covariance blocks, compact against full: {rel:.3e}")
    assert rel < 1e-6
