"""CPU tests of the per-observation residuals, hat blocks and deletion statistics: the long-double reference of
tests/hat_reference.py, the identity behind capi.deletion_statistics by brute force, the eigenvalue gap the rank decision rests
on, an fp64 emulation of the new row held to the bounds of the GPU tests (and five mistakes that leave them), and the header and
binding.  The device is held to the same references by tests/test_gpu_observation_hat.py.
"""
import os

import numpy as np
import pytest

import cov_bounds as CB
import hat_bounds as HB
import hat_reference as H
import landmark_covariance_reference as L
import observation_covariance_reference as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float64


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("name,norm", [("small", "NONE"), ("small", "HUBER"), ("p22", "NONE")])
@pytest.mark.parametrize("step", [1, 2])
def test_reference_blocks(step, name, norm):
    """sum_i tr P_ii = rank J, the eigenvalues of P_ii lie in [0, 1], tr P_ii is the leverage of the observation reference and,
    in step 2, P_ii = w_i [[c_uu, c_uv], [c_uv, c_vv]] of that reference (the same long-double route: to its rounding)."""
    ref = H.reference(name, step, norm, 0.0, True)
    oref = O.reference(name, step, norm, 0.0, True)
    P = ref.P
    assert np.array_equal(P, P.transpose(0, 2, 1)) or np.abs(P - P.transpose(0, 2, 1)).max() < 1e-15
    total = float(np.trace(P, axis1=1, axis2=2).sum())
    assert abs(total - ref.rank) <= ref.bound[:, np.arange(ref.d), np.arange(ref.d)].sum(), (total, ref.rank)
    ev = np.linalg.eigvalsh(P.astype(F))
    assert ev.min() > -1e-12 and ev.max() < 1 + 1e-12, (ev.min(), ev.max())
    tr = np.trace(P, axis1=1, axis2=2)
    assert np.abs((tr - oref.rows[:, 0]).astype(F)).max() < 1e-15 * ref.d
    if step == 2:
        w = ref.osys.w.astype(np.longdouble)
        want = np.stack([w * oref.rows[:, 1], w * oref.rows[:, 2], w * oref.rows[:, 2], w * oref.rows[:, 3]], 1).reshape(-1, 2, 2)
        assert np.abs((P - want).astype(F)).max() < 1e-15
    # the residuals are those of the step's cost: 1/2 sum r^2 with norm NONE
    if norm == "NONE":
        assert np.all(ref.osys.w == 1.0)


def test_residuals_are_the_oracles():
    """r of the reference is the r of dense_pose / dense_homogeneous, weighted: 1/2 |r|^2 is the cost with norm NONE."""
    from oracle import povar_numpy as PN
    for step in (1, 2):
        ref = H.reference("small", step, "NONE", 0.0, True)
        p = L.problem("small")
        cams, lms, obs = L.state(p, step)
        if step == 1:
            e = PN.dense_pose(L.ALPHA, p.n_cams, ref.osys.lm_off, ref.osys.cam_idx, obs, cams, lms)[3]
        else:
            e = PN.dense_homogeneous(p.n_cams, ref.osys.lm_off, ref.osys.cam_idx, obs, cams, lms)[3]
        assert abs(0.5 * np.sum(ref.r ** 2) - e.sum()) <= 1e-13 * e.sum()


# ---------------------------------------------------------------- the deletion identity by brute force
def _projected(J, r):
    """r without its component in range J: J^T r = 0 afterwards."""
    return r - J @ np.linalg.lstsq(J, r, rcond=None)[0]


def _brute_force(J, r, rows_of, picks):
    """Cost decrease |r|^2 - min_delta |r' + J' delta|^2 with the rows of each picked observation removed."""
    total = float(r @ r)
    out = []
    for i in picks:
        keep = np.ones(J.shape[0], dtype=bool)
        keep[rows_of(i)] = False
        Jk, rk = J[keep], r[keep]
        res = rk - Jk @ np.linalg.lstsq(Jk, rk, rcond=None)[0]
        out.append(total - float(res @ res))
    return np.array(out)


@pytest.mark.parametrize("norm", ["NONE", "HUBER"])
@pytest.mark.parametrize("step", [1, 2])
def test_deletion_identity_by_brute_force(step, norm):
    """At J^T r = 0, t_i = r_i^T (I - P_ii)^+ r_i is the decrease of the linearised cost when observation i is deleted and
    everything is re-estimated: every seventh observation of `small`, re-solved with lstsq, to 1e-9 relative (measured: 1.5e-12;
    the room is for another BLAS).  The two-view observations among them go through the pseudo-inverse."""
    from povar_amd import capi
    ref = H.reference("small", step, norm, 0.0, True)
    osys, d = ref.osys, ref.d
    J = osys.dense()
    r = _projected(J, ref.r.reshape(-1))
    assert np.abs(J.T @ r).max() < 1e-10
    t, rank = capi.deletion_statistics(r.reshape(-1, d), ref.P.astype(F))
    picks = np.arange(0, osys.n_obs, 7)
    want = _brute_force(J, r, lambda i: slice(d * i, d * i + d), picks)
    rel = np.abs(t[picks] - want) / np.abs(want)
    print(f"step {step} {norm}: deletion identity, worst relative difference {rel.max():.2e} over {len(picks)} observations")
    assert rel.max() < 1e-9
    assert np.array_equal(rank, ref.rank_i) and np.all(rank[ref.two_view] == d - 1) and np.all(rank[~ref.two_view] == d)
    assert ref.two_view[picks].any()
    # at a stationary point the residual has no component in the null direction of a two-view observation
    low = ref.mu < H.TOL_NULL
    proj = np.einsum("nkj,nk->nj", ref.V, r.reshape(-1, d))
    assert np.abs(proj[low]).max() <= 1e-10 * np.abs(r).max()


@pytest.mark.parametrize("step", [1, 2])
def test_deletion_identity_damped(step):
    """POVAR_COV_DAMPED: P = J H(lambda)^-1 J^T is the hat block of the augmented system [J; sqrt(lambda) I] (step 1: the cameras'
    columns only, as H(lambda) has it) and the statistic is that system's."""
    from povar_amd import capi
    lam = 1e-4
    ref = H.reference("small", step, "NONE", lam, False)
    osys, d = ref.osys, ref.d
    J = osys.dense()
    m = J.shape[1]
    damp = np.full(m, np.sqrt(lam))
    damp[osys.sys.n:] = np.sqrt(osys.sys.lam_l(lam))
    keep = damp > 0
    Ja = np.concatenate([J, np.diag(damp)[keep]], 0)
    ra = _projected(Ja, np.concatenate([ref.r.reshape(-1), np.zeros(int(keep.sum()))]))
    n_r = d * osys.n_obs
    t, rank = capi.deletion_statistics(ra[:n_r].reshape(-1, d), ref.P.astype(F))
    picks = np.arange(0, osys.n_obs, 7)
    want = _brute_force(Ja, ra, lambda i: slice(d * i, d * i + d), picks)
    rel = np.abs(t[picks] - want) / np.abs(want)
    print(f"step {step} damped: deletion identity, worst relative difference {rel.max():.2e}")
    assert rel.max() < 1e-9
    mu = np.linalg.eigvalsh(np.eye(d)[None] - ref.P.astype(F))
    print(f"step {step} damped: smallest eigenvalue of I - P_ii {mu.min():.3g}")
    # step 2 damps the landmarks too: I - P_ii is nonsingular.  Step 1 leaves them undamped (lambda_l = 0) and the null direction
    # of a two-view observation lives in its landmark: it stays null (about 1e-16) whatever lambda is
    assert np.all(rank[~ref.two_view] == d) and np.all(rank[ref.two_view] == (d - 1 if step == 1 else d))


# ---------------------------------------------------------------- the condition the rank test rests on
@pytest.mark.parametrize("name", ["small", "p22", "long"])
@pytest.mark.parametrize("step", [1, 2])
def test_eigenvalue_gap(step, name):
    """Every reference eigenvalue of I - P_ii is below 1e-9 or above 1e-4, and the ones below sit exactly on the observations of
    two-view tracks, one each: what makes "the device's rank equals the reference's for every observation" a fair demand."""
    ref = H.reference(name, step, "NONE", 0.0, True)
    low = ref.mu < H.TOL_NULL
    assert np.all(low | (ref.mu > H.GAP)), float(ref.mu[~low].min())
    assert np.array_equal(low.sum(1), ref.two_view.astype(np.int64))
    assert ref.two_view.sum() == {"small": 10, "p22": 8, "long": 82}[name]
    print(f"step {step} {name}: {int(low.sum())} null directions, smallest other eigenvalue {ref.mu[~low].min():.3g}")


def test_deletion_statistics_shapes_and_tolerance():
    from povar_amd import capi
    t, rank = capi.deletion_statistics(np.zeros((0, 4)), np.zeros((0, 4, 4)))
    assert t.shape == (0,) and rank.shape == (0,)
    P = np.array([np.diag([1.0, 0.5]), np.diag([0.25, 0.5])])
    r = np.array([[0.0, 1.0], [1.0, 1.0]])
    t, rank = capi.deletion_statistics(r, P)
    assert np.allclose(t, [2.0, 1 / 0.75 + 2.0]) and rank.tolist() == [1, 2]
    t, rank = capi.deletion_statistics(r, P, tol=0.6)
    assert rank.tolist() == [0, 1] and np.allclose(t, [0.0, 1 / 0.75])
    rows = np.arange(10.0).reshape(2, 5)
    rr, PP = capi.unpack_hat_rows(rows, 2)
    assert rr.tolist() == [[0, 1], [5, 6]] and PP[1].tolist() == [[7, 8], [8, 9]]


# ---------------------------------------------------------------- fp64 emulation of the new row, and five mistakes
EMU_CASES = [(1, "NONE"), (2, "NONE"), (1, "HUBER"), (2, "HUBER")]


def _emulation(step, norm, mutation=None):
    ref = H.reference("small", step, norm, 0.0, True)
    osys = ref.osys
    C, hi = osys.emulation_operands(0.0, True)
    p = L.problem("small")
    obs = L.state(p, step)[2]
    r_unw = ref.r / np.sqrt(osys.w)[:, None]
    return ref, H.emulate(osys, r_unw, C, hi, np.asarray(obs), mutation)


def _residual_bound(step, norm):
    return HB.hat_operands(CB.system("small", step, norm, 0.0)).Er


@pytest.mark.parametrize("step,norm", EMU_CASES)
def test_emulated_row_within_the_gpu_bounds(step, norm):
    """The row as the device evaluates it (Syy_i by obs_cov's route, then A_i Syy_i A_i^T and the weighted residual) in fp64:
    every entry of P_ii inside the end-to-end bound of the GPU test, every residual entry inside its componentwise bound."""
    ref, (r, P) = _emulation(step, norm)
    err = np.abs((P.astype(np.longdouble) - ref.P).astype(F))
    er = np.abs(r - ref.r)
    br = _residual_bound(step, norm)
    print(f"emulation step {step} {norm}: worst P err / bound {(err / ref.bound).max():.3g}, worst r err / bound {(er / br).max():.3g}")
    assert np.all(err <= ref.bound) and np.all(er <= br)
    assert np.array_equal(P, P.transpose(0, 2, 1))


@pytest.mark.parametrize("mutation", ["no_offdiag", "unweighted_a", "unweighted_r", "uv_kept", "half_factor"])
def test_mistakes_leave_the_bounds(mutation):
    """Each mistake a kernel could make in the new row leaves the bound somewhere (HUBER, where a weight matters; step 2 where
    uv does)."""
    for step in ((2,) if mutation == "uv_kept" else (1, 2)):
        ref, (r, P) = _emulation(step, "HUBER", mutation)
        assert np.any(ref.osys.w < 1.0)
        err = np.abs((P.astype(np.longdouble) - ref.P).astype(F))
        er = np.abs(r - ref.r)
        over = np.any(err > ref.bound) or np.any(er > _residual_bound(step, "HUBER"))
        assert over, (mutation, step)


@pytest.mark.parametrize("name,step,robust,lam", [c for c in CB.OBS_CASES if c[0] == "small"])
def test_condition_free_bounds_hold_on_the_emulated_chain(name, step, robust, lam):
    """hat_bounds on the buffers of cov_bounds' fp64 emulation of the whole chain: every residual and every block entry inside its
    condition-free bound, as the GPU test asks of the device's buffers."""
    sy = CB.system(name, step, robust, lam)
    d = CB.emulated(name, step, robust, lam, 0)
    Cs = CB.c_symmetric(d["inv"], d["panel"])[:sy.n, :sy.n]
    r, P = HB.emulate_hat(sy.p, d["q"], d["inv"], d["panel"], d["sig0"], d["dim"])
    out = HB.hat_check(sy, Cs, r, P)
    bad = out.pop("exact")
    CB.report(f"{name} step {step} {robust} lambda {lam:g} hat rows (emulated)", out, bad)
    assert np.abs(np.trace(P, axis1=1, axis2=2) - d["obs"][:, 0]).max() < 1e-10


# ---------------------------------------------------------------- header, map and binding
def test_header_map_and_binding():
    from povar_amd import capi
    header = open(os.path.join(ROOT, "include", "povar_hip.h")).read()
    for name in ("povar_observation_hat_pose", "povar_observation_hat_joint"):
        assert f"int {name}(povar_ctx* ctx, double lambda, int32_t gauge," in header, name
        assert hasattr(capi.lib(), name), name
    assert "stride 14" in header and "stride  5" in header
    assert "global: povar_*" in open(os.path.join(ROOT, "povar_amd", "csrc", "povar.map")).read()
    assert hasattr(capi.Context, "observation_hat") and callable(capi.deletion_statistics)
