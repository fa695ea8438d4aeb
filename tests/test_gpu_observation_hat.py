"""Per-observation residuals, hat blocks and deletion statistics (povar_observation_hat_pose / _joint,
capi.deletion_statistics, bal --observation-diagnostics-path) on the device.

End to end, against the long-double reference of tests/hat_reference.py: every entry (p, q) of P_ii within
    m u cond_2(K) |K^-1|_2 |b_p| |b_q|       (b_p, b_q the weighted rows of J_i; K, m, u as in tests/landmark_covariance_reference.py),
and in the free gauge sum_i tr P_ii = rank J within the summed bound.  Every case prints its worst error / bound; the bound is
not tightened to it.
Condition-free, on the device's own C and Sigma_l (povar_set_cov_inspect), by tests/hat_bounds.py: every entry of P_ii and
every residual entry inside a componentwise bound built from the caller's inputs and the kernel's operation counts.
The statistic: capi.deletion_statistics on the device's rows gives the reference's rank for EVERY observation (the eigenvalue
gap that makes this fair is asserted by tests/test_hat_reference.py and again here), and t within the first-order propagation
of the entry bounds (hat_reference.propagate, from the reference's eigenpairs).
The rest is what tests/test_gpu_observation_covariance.py asks of the call this one is modelled on.

Two calls on one context do not invert the same bits (the assembly of S adds with atomics), so rows of different calls are
compared inside the bound; rows of one call are compared bit for bit.
"""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import cov_bounds as CB
import hat_bounds as HB
import hat_reference as H
import landmark_covariance_reference as L
import observation_covariance_reference as O
from conftest import rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float64
LAM = 1e-4


def _linearise(ctx, step, cams, lms):
    ctx.set_cameras(cams)
    if step == 1:
        ctx.set_landmarks(lms)
        assert ctx.linearize_pose(L.ALPHA)
    else:
        ctx.set_landmarks_homogeneous(lms)
        assert ctx.linearize_homogeneous()


def _context(name, step, norm="NONE", inspect=False):
    from povar_amd import capi
    p = L.problem(name)
    cams, lms, obs = L.state(p, step)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs, robust_norm=norm, huber=L.HUBER[step])
    if inspect:
        ctx.set_cov_inspect(True)
    _linearise(ctx, step, cams, lms)
    return ctx


def _obs_of(lm_off, ids):
    return np.concatenate([np.arange(lm_off[l], lm_off[l + 1]) for l in ids]) if len(ids) else np.zeros(0, dtype=np.int64)


def _check(tag, P, rc, ref, rows=None):
    """The end-to-end bound on every entry of the returned blocks (rows: the observations they belong to)."""
    assert rc == 0, tag
    want, bound = (ref.P, ref.bound) if rows is None else (ref.P[rows], ref.bound[rows])
    assert P.shape == want.shape and np.all(np.isfinite(P)), tag
    assert np.array_equal(P, P.transpose(0, 2, 1)), tag
    err = np.abs((P.astype(np.longdouble) - want).astype(F))
    ratio = err / bound
    print(f"{tag}: m {ref.lm_ref.m} cond {ref.lm_ref.cond:.3g} |K^-1| {ref.lm_ref.inv_norm:.3g} worst P err / bound "
          f"{ratio.max():.3g} (worst |err| {err.max():.3e})")
    assert np.all(err <= bound), (tag, float(ratio.max()))


def _check_sum(tag, P, ref):
    dd = np.arange(ref.d)
    total = float(np.sum(P[:, dd, dd].astype(np.longdouble)))
    summed = ref.bound[:, dd, dd].sum()
    print(f"{tag}: sum tr P = {total:.12f}, rank J = {ref.rank}, summed bound {summed:.3e}")
    assert abs(total - ref.rank) <= summed, tag


def test_library_exports_the_calls():
    from povar_amd import capi
    lib = capi.lib()
    assert hasattr(lib, "povar_observation_hat_pose") and hasattr(lib, "povar_observation_hat_joint")
    assert hasattr(capi.Context, "observation_hat") and hasattr(capi, "deletion_statistics")


def _case_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-{c[3]:g}-{'free' if c[4] else 'damped'}"


@pytest.mark.parametrize("step,name,norm,lam,free", O.GPU_CASES, ids=[_case_id(c) for c in O.GPU_CASES])
def test_end_to_end(step, name, norm, lam, free):
    """The cases of the observation call: small (a camera straddles the 64-edge), p22 (a group owns more than one observation),
    long (both staging chunks take more than one trip), HUBER, and the damped system on small and medium."""
    ref = H.reference(name, step, norm, lam, free)
    ctx = _context(name, step, norm)
    tag = f"hat step {step} {name} {norm} lambda {lam:g}"
    r, P, rc = ctx.observation_hat(step=step, lam=lam, gauge=0 if free else 1)
    _check(tag, P, rc, ref)
    assert r.shape == ref.r.shape and np.all(np.isfinite(r))
    if free:
        _check_sum(tag, P, ref)
    ev = np.linalg.eigvalsh(P)
    slack = np.linalg.norm(ref.bound, axis=(1, 2))
    assert np.all(ev[:, 0] >= -slack) and np.all(ev[:, -1] <= 1 + slack)
    ctx.close()


# ---------------------------------------------------------------- the condition-free stage
def _buffers(ctx, sy, free):
    from povar_amd import capi
    j = sy.joint
    return dict(inv=ctx.get_buffer(capi.BUF_COV_INVERSE, joint=j), panel=ctx.get_buffer(capi.BUF_COV_PANEL, joint=j))


def _hat_call(ctx, sy, label, ids=None):
    p = sy.p
    free = p.lam == 0.0
    r, P, rc = ctx.observation_hat(step=2 if sy.joint else 1, lam=p.lam, gauge=0 if free else 1, lm_ids=ids)
    assert rc == 0, label
    d = _buffers(ctx, sy, free)
    n_rows = len(p.cam_idx) if ids is None else int(p.n_l[np.asarray(ids)].sum())
    dd = 2 if sy.joint else 4
    assert r.shape == (n_rows, dd) and P.shape == (n_rows, dd, dd)  # none skipped
    out = HB.hat_check(sy, CB.c_symmetric(d["inv"], d["panel"])[:sy.n, :sy.n], r, P, ids)
    bad = out.pop("exact")
    CB.report(label, out, bad)
    return r, P


def _cb_context(sy):
    from povar_amd import capi
    p = sy.p
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=p.robust, huber=p.huber, eps=p.eps)
    ctx.set_cov_inspect(True)
    _linearise(ctx, 2 if sy.joint else 1, p.cams, p.lms)
    return ctx


def _cb_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-{c[3]:g}"


@pytest.mark.parametrize("name,step,robust,lam", CB.OBS_CASES, ids=[_cb_id(c) for c in CB.OBS_CASES])
def test_rows_within_condition_free_bounds(name, step, robust, lam):
    """Every entry of P_ii and every residual entry of one call against the C that call left on the device (the cases of the
    OBSERVATION stage of tests/cov_bounds.py: every loop edge of the walk, the robust weight, the damped system); then an id list
    in reversed order with one landmark twice: each row against its own landmark, the landmark asked for twice the same bits."""
    sy = CB.system(name, step, robust, lam)
    p = sy.p
    ctx = _cb_context(sy)
    label = f"{name} step {step} {robust} lambda {lam:g} hat rows"
    r, P = _hat_call(ctx, sy, label)
    k = p.n_l
    pick = sorted({int(np.argmax(k)), int(np.argmin(k)), p.n_lms - 1, 0, int(np.flatnonzero(k >= 3)[0])})
    ids = np.array(pick[::-1] + [pick[-1]], dtype=np.int32)
    _hat_call(ctx, sy, label + " id list", ids)
    ctx.close()


# ---------------------------------------------------------------- consistency with what exists
@pytest.mark.parametrize("step", [1, 2])
def test_trace_is_the_leverage_and_residuals_are_the_cost(step):
    """On one context: tr P_ii against h of povar_observation_covariance_* inside the sum of the two end-to-end bounds (two calls:
    two assemblies), and with norm NONE 1/2 sum r_i^2 against all_error of povar_error_pose / _homogeneous inside the summed
    residual bound: both sides evaluate the same residual entries, each inside Er, so the difference of the two sums is at most
    2 sum |r| Er to first order, plus the n-term sums' own g(n) on the total."""
    ref = H.reference("small", step, "NONE", 0.0, True)
    ctx = _context("small", step)
    r, P, rc = ctx.observation_hat(step=step, lam=0.0, gauge=0)
    rows, rc2 = ctx.observation_covariance(step=step, lam=0.0, gauge=0)
    assert rc == 0 and rc2 == 0
    dd = np.arange(ref.d)
    both = ref.bound[:, dd, dd].sum(1) + ref.osys.bound(ref.lm_ref)[:, 0]
    diff = np.abs(np.trace(P, axis1=1, axis2=2) - rows[:, 0])
    print(f"step {step}: tr P against h, worst difference / summed bound {(diff / both).max():.3g}")
    assert np.all(diff <= both)
    ri = ctx.error_pose(L.ALPHA) if step == 1 else ctx.error_homogeneous()
    Er = HB.hat_operands(CB.system("small", step, "NONE", 0.0)).Er
    half = 0.5 * float(np.sum(r.astype(np.longdouble) ** 2))
    tol = 2 * float(np.sum(np.abs(r) * Er)) + 2 * r.size * L.U * half
    print(f"step {step}: 1/2 sum r^2 = {half:.15g}, all_error = {ri.all_error:.15g}, difference {abs(half - ri.all_error):.3e}, bound {tol:.3e}")
    assert ri.all_num_obs == r.shape[0] and abs(half - ri.all_error) <= tol
    ctx.close()


# ---------------------------------------------------------------- statistic and rank
@pytest.mark.parametrize("name", ["small", "p22", "long"])
@pytest.mark.parametrize("step", [1, 2])
def test_statistic_and_rank(step, name):
    """Free gauge: the rank of every observation is the reference's (nothing left out), t inside the first-order propagation of
    the entry bounds of r (componentwise, tests/hat_bounds.py) and P (end to end) through sum (v^T r)^2 / mu."""
    from povar_amd import capi
    ref = H.reference(name, step, "NONE", 0.0, True)
    low = ref.mu < H.TOL_NULL
    assert np.all(low | (ref.mu > H.GAP)) and np.array_equal(low.sum(1), ref.two_view.astype(np.int64))
    ctx = _context(name, step)
    r, P, rc = ctx.observation_hat(step=step, lam=0.0, gauge=0)
    assert rc == 0
    t, rank = capi.deletion_statistics(r, P)
    assert rank.shape == (ref.osys.n_obs,) and np.array_equal(rank, ref.rank_i)
    Er = HB.hat_operands(CB.system(name, step, "NONE", 0.0)).Er
    bound = H.propagate(ref.r, ref.mu, ref.V, Er, ref.bound)
    # the reference's own residuals are the oracle's fp64 ones: inside Er as well
    bound = bound + H.propagate(ref.r, ref.mu, ref.V, Er, np.zeros_like(ref.bound))
    err = np.abs(t - ref.t)
    print(f"step {step} {name}: rank equal for all {rank.shape[0]} observations ({int(ref.two_view.sum())} two-view), "
          f"worst t err / bound {(err / bound).max():.3g}, worst relative t err {(err / np.maximum(ref.t, 1e-300)).max():.3e}")
    assert np.all(t >= 0) and np.all(err <= bound)
    ctx.close()


# ---------------------------------------------------------------- the behaviour of the observation call
@pytest.mark.parametrize("step", [1, 2])
def test_id_list(step):
    """A list with a duplicate and a reversed order, served by the same call as every landmark in order: bit for bit with the
    all-landmarks rows on the same C; an empty list works."""
    ref = H.reference("small", step, "NONE", 0.0, True)
    lm_off, n_lms = ref.osys.lm_off, ref.osys.sys.n_lms
    ctx = _context("small", step)
    ids = np.array([n_lms - 1, 7, 3, 7, 0, 3], dtype=np.int32)
    both = np.concatenate([np.arange(n_lms, dtype=np.int32), ids])
    r, P, rc = ctx.observation_hat(step=step, lam=0.0, gauge=0, lm_ids=both)
    n_obs = int(lm_off[-1])
    rows = _obs_of(lm_off, ids)
    assert rc == 0 and r.shape == (n_obs + rows.shape[0], ref.d)
    _check(f"hat id list step {step}: every landmark in order", P[:n_obs], rc, ref)
    assert np.array_equal(P[n_obs:], P[:n_obs][rows]) and np.array_equal(r[n_obs:], r[:n_obs][rows])
    r1, P1, rc = ctx.observation_hat(step=step, lam=0.0, gauge=0, lm_ids=ids)
    _check(f"hat id list step {step}: the list alone", P1, rc, ref, rows)
    assert np.array_equal(r1, r[:n_obs][rows])  # the residuals do not depend on C
    r0, P0, rc = ctx.observation_hat(step=step, lam=0.0, gauge=0, lm_ids=np.zeros(0, dtype=np.int32))
    assert rc == 0 and r0.shape == (0, ref.d) and P0.shape == (0, ref.d, ref.d)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_sharded_matches_single(step):
    """Two shard contexts on one device through the host all-reduce hook: each rank returns its shard's observations."""
    from povar_amd import capi
    from test_gpu_sharded import HostAllReduce
    p = L.problem("p22")
    ref = H.reference("p22", step, "NONE", 0.0, True)
    cams, lms, obs = L.state(p, step)
    single = _context("p22", step)
    r_all, P_all, rc = single.observation_hat(step=step, lam=0.0, gauge=0)
    single.close()
    _check(f"hat sharded step {step}: the single context", P_all, rc, ref)
    world = 2
    ar = HostAllReduce(world)
    out = [None] * world

    def worker(rank):
        try:
            lb, le = capi.shard_range(p.lm_off, world, rank)
            ob, oe = int(p.lm_off[lb]), int(p.lm_off[le])
            ctx = capi.Context(p.n_cams, p.lm_off[lb:le + 1] - p.lm_off[lb], p.cam_idx[ob:oe], obs[ob:oe])
            ctx.comm_init_host(world, rank, ar.fn(rank))
            _linearise(ctx, step, cams, lms[lb:le])
            r, P, rc = ctx.observation_hat(step=step, lam=0.0, gauge=0)
            out[rank] = (ob, oe, r, P, rc)
            ctx.close()
        except BaseException:
            ar.bar.abort()  # a failed rank must not leave the other one waiting
            raise

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert all(o is not None for o in out)
    covered = 0
    for rank, (ob, oe, r, P, rc) in enumerate(out):
        rows = np.arange(ob, oe)
        _check(f"hat sharded step {step} rank {rank}", P, rc, ref, rows)
        assert np.all(np.abs(P - P_all[rows]) <= ref.bound[rows])
        assert np.array_equal(r, r_all[rows])
        covered += oe - ob
    assert covered == ref.osys.n_obs


@pytest.mark.parametrize("step", [1, 2])
def test_free_gauge_reports_degeneracy_beyond_the_gauge(step):
    """medium: null dimension 21 / 30 instead of 12 / 15: POVAR_NUMERIC_FAILURE and every entry NaN."""
    from povar_amd import capi
    ctx = _context("medium", step)
    r, P, rc = ctx.observation_hat(step=step, lam=0.0, gauge=0)
    assert rc == capi.NUMERIC_FAILURE == 1 and r.size > 0 and np.all(np.isnan(r)) and np.all(np.isnan(P))
    ctx.close()


def test_argument_errors():
    from povar_amd import capi
    p = L.problem("small")
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(L.ALPHA)
    n_lms, n_obs = p.lm_off.shape[0] - 1, int(p.lm_off[-1])
    out = np.zeros(14 * (n_obs + 8))
    track = np.diff(p.lm_off)

    def call(step, lam, gauge, ids=None, n_rows=None, null_out=False):
        fn = ctx.L.povar_observation_hat_pose if step == 1 else ctx.L.povar_observation_hat_joint
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        if n_rows is None:
            n_rows = n_obs if ids is None else int(sum(track[i] for i in ids if 0 <= i < n_lms))
        return fn(ctx.h, C.c_double(lam), C.c_int32(gauge), None if ids is None else C.c_void_p(ids.ctypes.data),
                  C.c_int32(0 if ids is None else ids.shape[0]), None if null_out else C.c_void_p(out.ctypes.data), C.c_int64(n_rows))

    assert call(1, 0.0, 0) < 0 and call(2, 0.0, 0) < 0  # no linearisation in force
    assert ctx.linearize_pose(L.ALPHA)
    assert call(2, 0.0, 0) < 0  # step 1's linearisation does not serve step 2
    assert call(1, 1e-4, capi.COV_FREE_GAUGE) < 0   # free gauge with lambda != 0
    assert call(1, 0.0, capi.COV_DAMPED) < 0 and call(1, -1.0, capi.COV_DAMPED) < 0  # damped with lambda <= 0
    assert call(1, 0.0, 2) < 0 and call(1, 0.0, -1) < 0  # unknown gauge
    assert call(1, 0.0, 0, ids=[0, n_lms]) < 0 and call(1, 0.0, 0, ids=[-1]) < 0  # id out of range
    assert call(1, 0.0, 0, n_rows=n_obs - 1) < 0 and call(1, 0.0, 0, n_rows=n_obs + 1) < 0  # wrong n_rows, all landmarks
    assert call(1, 0.0, 0, ids=[0, 1], n_rows=int(track[0])) < 0 and call(1, 0.0, 0, ids=[0, 0], n_rows=int(track[0])) < 0
    assert call(1, 0.0, 0, ids=[0, 1], null_out=True) < 0 and call(1, 0.0, 0, null_out=True) < 0  # null rows, rows > 0
    assert b"povar_observation_hat_pose" in ctx.L.povar_last_error()
    with pytest.raises(capi.PovarError):
        ctx.observation_hat(step=1, lam=1.0, gauge=capi.COV_FREE_GAUGE)
    with pytest.raises(capi.PovarError):
        ctx.observation_hat(step=2, lam=0.0, gauge=capi.COV_FREE_GAUGE)
    with pytest.raises(capi.PovarError):
        ctx.observation_hat(step=1, lm_ids=[n_lms])
    with pytest.raises(ValueError):
        ctx.observation_hat(step=3)
    assert call(1, 0.0, 0) == 0 and call(1, 0.0, 0, ids=[n_lms - 1, 0, 0]) == 0
    ctx.close()


def test_no_side_effects_on_solvers_and_landmark_blocks():
    """A hat call leaves the dense matrix as an observation call does: CHOLESKY / RICHOLESKY increments after it match those
    before it (the assembly adds with atomics: 1e-8, the tolerance of the camera test), POVAR_BUF_SC_FACTOR is an argument error
    until the next direct solve, the landmark call returns the blocks it returned before, and the scratch is allocated once:
    device_bytes is stable after the first call."""
    from povar_amd import capi
    for step in (1, 2):
        lref = L.reference("small", step, "NONE", 0.0, True)
        ctx = _context("small", step)

        def solve():
            if step == 1:
                inc, it, status, rc = ctx.solve_pose_sc(LAM, capi.SC_CHOLESKY)
            else:
                inc, it, status, rc = ctx.solve_joint_sc(LAM, method=capi.SC_CHOLESKY)
            assert rc == 0 and it == 0
            return inc

        before = solve()
        ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
        blocks_before, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=1)
        assert rc == 0
        bytes_before = None
        for gauge, lam in ((capi.COV_FREE_GAUGE, 0.0), (capi.COV_DAMPED, 1.0)):
            _, _, rc = ctx.observation_hat(step=step, lam=lam, gauge=gauge)
            assert rc == 0
            with pytest.raises(capi.PovarError):
                ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
            after = solve()
            assert rel(after, before) < 1e-8, (step, gauge)
            ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
            if bytes_before is None:
                bytes_before = ctx.device_bytes()
            assert ctx.device_bytes() == bytes_before
        blocks_after, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=1)
        assert rc == 0
        assert np.all(np.linalg.norm(blocks_after - blocks_before, axis=(1, 2)) <= lref.bound)
        ctx.close()


# ---------------------------------------------------------------- bal
def _read_file(path, lm_off, cam_idx, d):
    lines = open(path).read().split("\n")
    n_obs = cam_idx.shape[0]
    assert int(lines[0]) == n_obs and len([ln for ln in lines[1:] if ln.strip()]) == n_obs
    tab = np.array([[float(x) for x in ln.split()] for ln in lines[1:1 + n_obs]])
    assert tab.shape == (n_obs, 4 + d + d * (d + 1) // 2) and np.all(np.isfinite(tab))
    assert np.array_equal(tab[:, 0], np.repeat(np.arange(lm_off.shape[0] - 1), np.diff(lm_off)))
    assert np.array_equal(tab[:, 1], cam_idx)
    return tab[:, 2], tab[:, 3].astype(np.int64), tab[:, 4:]


def _file_statistics_agree(t, rank, raw, d, tol=1e-8):
    """t and rank of the file against capi.deletion_statistics on the file's own raw numbers: the rank exactly, t to 1e-9
    relative -- u / mu_min with mu_min >= 1e-4 (asserted) is 2e-12, with margin for two different eigen-solvers."""
    from povar_amd import capi
    r, P = capi.unpack_hat_rows(raw, d)
    want_t, want_rank = capi.deletion_statistics(r, P, tol)
    mu = np.linalg.eigvalsh(np.eye(d)[None] - P)
    assert np.all((mu <= tol) | (mu >= 1e-4)), float(mu[mu > tol].min())
    assert np.array_equal(rank, want_rank)
    assert np.all(np.abs(t - want_t) <= 1e-9 * np.abs(want_t))


def test_bal_writes_the_observation_diagnostics(tmp_path):
    """`bal --observation-diagnostics-path`: n_obs, then per observation `landmark camera t rank` and the raw row, at the final
    state of the last step that ran.  With no LM iteration the raw part equals the ABI call (1e-9, the existing file tests'
    tolerance); t and rank equal capi.deletion_statistics on the file's own numbers; --gpus 2 writes the same file; the flag is
    independent of the other covariance flags.  After iterations of both steps: n_obs lines, t >= 0, 0 <= rank <= 2."""
    from povar_amd import capi, synth
    p = synth.make_problem(10, 300, 1300, seed=21)
    f = str(tmp_path / "problem-10-300.txt")
    synth.write_data_custom(f, p)
    q = synth.read_data_custom(f)
    base = [os.path.join(ROOT, "bin/bal"), "--input", f, "--quiet", "--power-sc-iterations", "20", "--log-disable-all"]

    def run(extra):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]

    out, obs_out = str(tmp_path / "diag.txt"), str(tmp_path / "obs.txt")
    still = ["--max-num-iterations-step-1", "0", "--max-num-iterations-step-2", "0"]
    run(still + ["--observation-diagnostics-path", out])
    t, rank, raw = _read_file(out, q.lm_off, q.cam_idx, 4)
    ctx = capi.Context(q.n_cams, q.lm_off, q.cam_idx, q.obs)
    ctx.set_cameras(q.cams)
    ctx.init_landmarks_pose(L.ALPHA)
    assert ctx.linearize_pose(L.ALPHA)
    r, P, rc = ctx.observation_hat(step=1, lam=0.0, gauge=0)
    ctx.close()
    assert rc == 0
    iu = np.triu_indices(4)
    want = np.concatenate([r, P[:, iu[0], iu[1]]], 1)
    print(f"bal against the ABI call: {rel(raw, want):.2e}; ranks {np.bincount(rank, minlength=5).tolist()}")
    assert rel(raw, want) < 1e-9
    _file_statistics_agree(t, rank, raw, 4)
    os.remove(out)
    # another tolerance, with the observation file, and from two shards
    run(still + ["--observation-diagnostics-path", out, "--observation-diagnostics-tol", "0.5", "--observation-covariance-path", obs_out])
    t5, rank5, raw5 = _read_file(out, q.lm_off, q.cam_idx, 4)
    assert rel(raw5, want) < 1e-9 and os.path.exists(obs_out)
    _, want_rank5 = capi.deletion_statistics(*capi.unpack_hat_rows(raw5, 4), 0.5)
    assert np.array_equal(rank5, want_rank5) and np.any(rank5 < rank)
    os.remove(out)
    run(still + ["--observation-diagnostics-path", out, "--gpus", "2"])
    t2, rank2, raw2 = _read_file(out, q.lm_off, q.cam_idx, 4)
    assert rel(raw2, want) < 1e-9 and np.array_equal(rank2, rank)
    _file_statistics_agree(t2, rank2, raw2, 4)
    os.remove(out)
    # after both steps
    run(["--max-num-iterations-step-1", "8", "--max-num-iterations-step-2", "4", "--observation-diagnostics-path", out])
    t, rank, raw = _read_file(out, q.lm_off, q.cam_idx, 2)
    print(f"after both steps: sum t = {t.sum():.6g}, ranks {np.bincount(rank, minlength=3).tolist()}")
    assert np.all(t >= 0) and np.all(rank >= 0) and np.all(rank <= 2)
