"""Per-observation leverage and predicted-point covariance (povar_observation_covariance_pose / _joint) against the
long-double reference of tests/observation_covariance_reference.py, through the C ABI.

Tolerance, both modes, per entry of a row (h, c_uu, c_uv, c_vv): |err| <= m u cond_2(K) |K^-1|_2 |b_p| |b_q| summed over the
rows b of the quadratic form the entry is -- the d weighted rows J_i for h, the two unweighted rows of the predicted image
point for c_* -- with K, m, u as in tests/landmark_covariance_reference.py (the matrix that is actually inverted).
tests/test_observation_covariance_reference.py holds an fp64 emulation of the kernel to the same bound and shows that five
mistakes a kernel could make leave it.  Every case prints its worst error / bound (DESIGN.md section 3 records them); the
bound is not tightened to it.  In the free gauge every case also checks sum_i h_i = rank J inside the summed bound.

Two calls on one context do not invert the same bits (the assembly of S adds with atomics), so rows of different calls are
compared inside the bound; rows of one call are compared bit for bit.
The kernel itself (obs_cov) is held entry by entry to a condition-free bound on the C of its own call by the OBSERVATION stage
of tests/cov_bounds.py (tests/test_gpu_cov_bounds.py); this module stays the end-to-end check against an independent route.
"""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import landmark_covariance_reference as L
import observation_covariance_reference as O
from conftest import rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 1e-4


def _linearise(ctx, step, cams, lms):
    ctx.set_cameras(cams)
    if step == 1:
        ctx.set_landmarks(lms)
        assert ctx.linearize_pose(L.ALPHA)
    else:
        ctx.set_landmarks_homogeneous(lms)
        assert ctx.linearize_homogeneous()


def _context(name, step, norm="NONE"):
    from povar_amd import capi
    p = L.problem(name)
    cams, lms, obs = L.state(p, step)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs, robust_norm=norm, huber=L.HUBER[step])
    _linearise(ctx, step, cams, lms)
    return ctx


def _obs_of(lm_off, ids):
    """Observation indices of the tracks of `ids`, concatenated in list order."""
    return np.concatenate([np.arange(lm_off[l], lm_off[l + 1]) for l in ids]) if len(ids) else np.zeros(0, dtype=np.int64)


def _check(tag, got, rc, ref, rows=None):
    """The bound on every entry of the returned rows (rows: the observations they belong to); worst error / bound."""
    assert rc == 0, tag
    want, bound = (ref.rows, ref.bound) if rows is None else (ref.rows[rows], ref.bound[rows])
    assert got.shape == want.shape and np.all(np.isfinite(got)), tag
    err = np.abs((got.astype(np.longdouble) - want).astype(np.float64))
    ratio = err / bound
    print(f"{tag}: m {ref.lm_ref.m} cond {ref.lm_ref.cond:.3g} |K^-1| {ref.lm_ref.inv_norm:.3g} worst err / bound: "
          f"h {ratio[:, 0].max():.3g}, c_* {ratio[:, 1:].max():.3g} (worst |err| {err.max():.3e})")
    assert np.all(err <= bound), (tag, float(ratio.max()))
    return float(ratio.max())


def _check_sum(tag, got, ref):
    total = float(np.sum(got[:, 0].astype(np.longdouble)))
    print(f"{tag}: sum h = {total:.12f}, rank J = {ref.rank}, summed bound {ref.bound[:, 0].sum():.3e}")
    assert abs(total - ref.rank) <= ref.bound[:, 0].sum(), tag
    assert np.all(got[:, 0] >= 0) and np.all(got[:, 0] <= ref.osys.d), tag


def test_library_exports_the_calls():
    from povar_amd import capi
    lib = capi.lib()
    assert hasattr(lib, "povar_observation_covariance_pose") and hasattr(lib, "povar_observation_covariance_joint")
    assert hasattr(capi.Context, "observation_covariance")


@pytest.mark.parametrize("step,name,norm", [(1, "small", "NONE"), (2, "small", "NONE"), (1, "p22", "NONE"), (2, "p22", "NONE"),
                                            (1, "small", "HUBER"), (2, "small", "HUBER")])
def test_free_gauge(step, name, norm):
    """small: 6 cameras, n = 72 / 66, N = 128: camera 5 straddles the 64-edge in both steps; p22: several 64-blocks, tracks of
    more than 16 observations (a group owns more than one observation).  HUBER: the weighted rows for h, the unweighted for c_*."""
    ref = O.reference(name, step, norm, 0.0, True)
    ctx = _context(name, step, norm)
    tag = f"free gauge step {step} {name} {norm}"
    got, rc = ctx.observation_covariance(step=step, lam=0.0, gauge=0)
    _check(tag, got, rc, ref)
    _check_sum(tag, got, ref)
    if step == 2:  # h = w (c_uu + c_vv): each side inside its bound, and w (bound_uu + bound_vv) = bound_h
        assert np.all(np.abs(got[:, 0] - ref.osys.w * (got[:, 1] + got[:, 3])) <= 2 * ref.bound[:, 0])
    if name == "p22":
        assert np.diff(ref.osys.lm_off).max() > 16
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_long_tracks(step):
    """66 cameras, two tracks of >= 65 observations and three of 33..64: both chunk loops of both stagings (chunks of 64 and
    32) take more than one trip, in i and in j."""
    s = L.system("long", step)
    assert s.n_cams == 66 and np.sum(s.track >= 65) == 2 and np.sum((s.track >= 33) & (s.track <= 64)) == 3
    ref = O.reference("long", step, "NONE", 0.0, True)
    ctx = _context("long", step)
    got, rc = ctx.observation_covariance(step=step, lam=0.0, gauge=0)
    _check(f"long tracks step {step}", got, rc, ref)
    _check_sum(f"long tracks step {step}", got, ref)
    ids = np.flatnonzero(s.track >= 33)[::-1]
    sub, rc = ctx.observation_covariance(step=step, lam=0.0, gauge=0, lm_ids=ids)
    _check(f"long tracks step {step}: the five long ones", sub, rc, ref, _obs_of(ref.osys.lm_off, ids))
    ctx.close()


@pytest.mark.parametrize("lam", [1e-4, 1.0])
@pytest.mark.parametrize("name", ["small", "medium"])
@pytest.mark.parametrize("step", [1, 2])
def test_damped(step, name, lam):
    """h = tr(J_i H(lambda)^-1 J_i^T); medium: n = 588 / 539, N = 640 / 576."""
    ref = O.reference(name, step, "NONE", lam, False)
    ctx = _context(name, step)
    got, rc = ctx.observation_covariance(step=step, lam=lam, gauge=1)
    _check(f"damped step {step} {name} lambda {lam:g}", got, rc, ref)
    assert np.all(got[:, 0] > 0) and np.all(got[:, 0] < ref.osys.d)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_id_list(step):
    """A list with a duplicate and a reversed order.  One call serves every landmark in order and then the list, so the rows
    of the list are compared bit for bit with those of the all-landmarks request on the same C; against a separate
    lm_ids = NULL call (another assembly: other bits of C) the rows agree inside the bound."""
    ref = O.reference("small", step, "NONE", 0.0, True)
    lm_off, n_lms = ref.osys.lm_off, ref.osys.sys.n_lms
    ctx = _context("small", step)
    ids = np.array([n_lms - 1, 7, 3, 7, 0, 3], dtype=np.int32)
    both = np.concatenate([np.arange(n_lms, dtype=np.int32), ids])
    got, rc = ctx.observation_covariance(step=step, lam=0.0, gauge=0, lm_ids=both)
    n_obs = int(lm_off[-1])
    rows = _obs_of(lm_off, ids)
    assert rc == 0 and got.shape == (n_obs + rows.shape[0], 4)
    _check(f"id list step {step}: every landmark in order", got[:n_obs], rc, ref)
    assert np.array_equal(got[n_obs:], got[:n_obs][rows])
    alone, rc = ctx.observation_covariance(step=step, lam=0.0, gauge=0, lm_ids=ids)
    _check(f"id list step {step}: the list alone", alone, rc, ref, rows)
    k7, k3 = int(lm_off[8] - lm_off[7]), int(lm_off[4] - lm_off[3])
    a7 = int(lm_off[n_lms] - lm_off[n_lms - 1])
    assert np.array_equal(alone[a7:a7 + k7], alone[a7 + k7 + k3:a7 + 2 * k7 + k3])  # the two copies of landmark 7
    every, rc = ctx.observation_covariance(step=step, lam=0.0, gauge=0)
    _check(f"id list step {step}: lm_ids = NULL", every, rc, ref)
    assert np.all(np.abs(alone - every[rows]) <= ref.bound[rows])
    none, rc = ctx.observation_covariance(step=step, lam=0.0, gauge=0, lm_ids=np.zeros(0, dtype=np.int32))
    assert rc == 0 and none.shape == (0, 4)
    ctx.close()


def test_step1_does_not_depend_on_the_column_scaling():
    """povar_set_jl_col_scaling(0) against the default: the same rows inside the bound."""
    from povar_amd import capi
    p = L.problem("small")
    ref = O.reference("small", 1, "NONE", 0.0, True)
    cams, lms, obs = L.state(p, 1)
    out = []
    for scaling in (True, False):
        ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs)
        ctx.set_jl_col_scaling(scaling)
        _linearise(ctx, 1, cams, lms)
        got, rc = ctx.observation_covariance(step=1, lam=0.0, gauge=0)
        assert rc == 0
        out.append(got)
        ctx.close()
    _check("step 1, default column scaling", out[0], 0, ref)
    diff = np.abs(out[1] - out[0])
    print(f"column scaling off against on: worst difference / bound {(diff / ref.bound).max():.3g}")
    assert np.all(diff <= ref.bound)


@pytest.mark.parametrize("step", [1, 2])
def test_two_calls_agree_within_the_bound(step):
    """Not bit for bit: the assembly of S adds with atomics; given C the rows are reproducible (test_id_list)."""
    ref = O.reference("small", step, "NONE", 0.0, True)
    ctx = _context("small", step)
    a, rc_a = ctx.observation_covariance(step=step, lam=0.0, gauge=0)
    b, rc_b = ctx.observation_covariance(step=step, lam=0.0, gauge=0)
    assert rc_a == 0 and rc_b == 0
    diff = np.abs(a - b)
    print(f"step {step}: two calls differ by at most {(diff / ref.bound).max():.3g} of the bound")
    assert np.all(diff <= ref.bound)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_sharded_matches_single(step):
    """Two shard contexts on one device through the host all-reduce hook: each rank returns its shard's observations."""
    from povar_amd import capi
    from test_gpu_sharded import HostAllReduce
    p = L.problem("p22")
    ref = O.reference("p22", step, "NONE", 0.0, True)
    cams, lms, obs = L.state(p, step)
    single = _context("p22", step)
    whole, rc = single.observation_covariance(step=step, lam=0.0, gauge=0)
    single.close()
    _check(f"sharded step {step}: the single context", whole, rc, ref)
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
            got, rc = ctx.observation_covariance(step=step, lam=0.0, gauge=0)
            some = np.arange(le - lb)[::-3]
            sub, rc_sub = ctx.observation_covariance(step=step, lam=0.0, gauge=0, lm_ids=some)
            out[rank] = (lb, le, ob, oe, got, rc, some, sub, rc_sub)
            ctx.close()
        except BaseException:
            ar.bar.abort()  # a failed rank must not leave the other one waiting
            raise

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert all(o is not None for o in out)
    covered = 0
    for rank, (lb, le, ob, oe, got, rc, some, sub, rc_sub) in enumerate(out):
        rows = np.arange(ob, oe)
        _check(f"sharded step {step} rank {rank}", got, rc, ref, rows)
        assert np.all(np.abs(got - whole[rows]) <= ref.bound[rows])
        _check(f"sharded step {step} rank {rank} subset", sub, rc_sub, ref, _obs_of(p.lm_off, lb + some))
        covered += oe - ob
    assert covered == ref.osys.n_obs


@pytest.mark.parametrize("step", [1, 2])
def test_free_gauge_reports_degeneracy_beyond_the_gauge(step):
    """medium_problem: null dimension 21 / 30 instead of 12 / 15: POVAR_NUMERIC_FAILURE and every entry NaN."""
    from povar_amd import capi
    ctx = _context("medium", step)
    got, rc = ctx.observation_covariance(step=step, lam=0.0, gauge=0)
    assert rc == capi.NUMERIC_FAILURE == 1 and got.size > 0 and np.all(np.isnan(got))
    ctx.close()


def test_argument_errors():
    from povar_amd import capi
    p = L.problem("small")
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(L.ALPHA)
    n_lms, n_obs = p.lm_off.shape[0] - 1, int(p.lm_off[-1])
    out = np.zeros(4 * (n_obs + 8))
    track = np.diff(p.lm_off)

    def call(step, lam, gauge, ids=None, n_rows=None, null_out=False):
        fn = ctx.L.povar_observation_covariance_pose if step == 1 else ctx.L.povar_observation_covariance_joint
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        if n_rows is None:
            n_rows = n_obs if ids is None else int(sum(track[i] for i in ids if 0 <= i < n_lms))
        return fn(ctx.h, C.c_double(lam), C.c_int32(gauge), None if ids is None else C.c_void_p(ids.ctypes.data),
                  C.c_int32(0 if ids is None else ids.shape[0]), None if null_out else C.c_void_p(out.ctypes.data), C.c_int64(n_rows))

    # no linearisation in force
    assert call(1, 0.0, 0) < 0 and call(2, 0.0, 0) < 0
    assert ctx.linearize_pose(L.ALPHA)
    assert call(2, 0.0, 0) < 0  # step 1's linearisation does not serve step 2
    assert call(1, 1e-4, capi.COV_FREE_GAUGE) < 0   # free gauge with lambda != 0
    assert call(1, 0.0, capi.COV_DAMPED) < 0 and call(1, -1.0, capi.COV_DAMPED) < 0  # damped with lambda <= 0
    assert call(1, 0.0, 2) < 0 and call(1, 0.0, -1) < 0  # unknown gauge
    assert call(1, 0.0, 0, ids=[0, n_lms]) < 0 and call(1, 0.0, 0, ids=[-1]) < 0  # id out of range
    assert call(1, 0.0, 0, n_rows=n_obs - 1) < 0 and call(1, 0.0, 0, n_rows=n_obs + 1) < 0  # wrong n_rows, all landmarks
    assert call(1, 0.0, 0, ids=[0, 1], n_rows=int(track[0])) < 0 and call(1, 0.0, 0, ids=[0, 0], n_rows=int(track[0])) < 0
    assert call(1, 0.0, 0, ids=[0, 1], null_out=True) < 0 and call(1, 0.0, 0, null_out=True) < 0  # null obs_cov, rows > 0
    with pytest.raises(capi.PovarError):
        ctx.observation_covariance(step=1, lam=1.0, gauge=capi.COV_FREE_GAUGE)
    with pytest.raises(capi.PovarError):
        ctx.observation_covariance(step=2, lam=0.0, gauge=capi.COV_FREE_GAUGE)
    with pytest.raises(ValueError):
        ctx.observation_covariance(step=3)
    assert call(1, 0.0, 0) == 0 and call(1, 0.0, 0, ids=[n_lms - 1, 0, 0]) == 0
    ctx.close()


def test_no_side_effects_on_solvers_and_landmark_blocks():
    """An observation call leaves the dense matrix as a landmark call does: CHOLESKY / RICHOLESKY increments after it match
    those before it (the assembly adds with atomics: 1e-8, the tolerance of the camera test), POVAR_BUF_SC_FACTOR is an
    argument error until the next direct solve, and the landmark call returns the blocks it returned before (with their gauge
    correction: the observation call's nq = 0 pass does not stick)."""
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
            _, rc = ctx.observation_covariance(step=step, lam=lam, gauge=gauge)
            assert rc == 0
            with pytest.raises(capi.PovarError):
                ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
            after = solve()
            assert rel(after, before) < 1e-8, (step, gauge)
            ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
            # the scratch is allocated once and counted
            if bytes_before is None:
                bytes_before = ctx.device_bytes()
            assert ctx.device_bytes() == bytes_before
        blocks_after, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=1)
        assert rc == 0
        diff = np.linalg.norm(blocks_after - blocks_before, axis=(1, 2))
        assert np.all(diff <= lref.bound)
        assert np.all(np.linalg.norm((blocks_after.astype(np.longdouble) - lref.blocks).astype(np.float64), axis=(1, 2)) <= lref.bound)
        ctx.close()


def _read_rows(path, lm_off, cam_idx):
    lines = open(path).read().split("\n")
    n_obs = cam_idx.shape[0]
    assert int(lines[0]) == n_obs and len([ln for ln in lines[1:] if ln.strip()]) == n_obs
    tab = np.array([[float(x) for x in ln.split()] for ln in lines[1:1 + n_obs]])
    assert tab.shape == (n_obs, 6) and np.all(np.isfinite(tab))
    assert np.array_equal(tab[:, 0], np.repeat(np.arange(lm_off.shape[0] - 1), np.diff(lm_off)))
    assert np.array_equal(tab[:, 1], cam_idx)
    return tab[:, 2:]


def test_bal_writes_the_observation_covariance(tmp_path):
    """`bal --observation-covariance-path`: n_obs, then one line per observation: landmark camera h c_uu c_uv c_vv at the
    final state of the last step that ran.  With no LM iteration in either step the final state is the one a caller can set
    up too: there the file agrees with the ABI call; --gpus 2 writes the same file, and the flag is independent of the other
    two.  After iterations of both steps: n_obs lines, leverages in (0, 2)."""
    from povar_amd import capi, synth
    p = synth.make_problem(10, 300, 1300, seed=21)
    f = str(tmp_path / "problem-10-300.txt")
    synth.write_data_custom(f, p)
    q = synth.read_data_custom(f)
    n_lms = q.lm_off.shape[0] - 1
    base = [os.path.join(ROOT, "bin/bal"), "--input", f, "--quiet", "--power-sc-iterations", "20", "--log-disable-all"]

    def run(extra):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]

    out, lm_out = str(tmp_path / "obs.txt"), str(tmp_path / "lm.txt")
    still = ["--max-num-iterations-step-1", "0", "--max-num-iterations-step-2", "0"]
    run(still + ["--observation-covariance-path", out])
    rows = _read_rows(out, q.lm_off, q.cam_idx)
    ctx = capi.Context(q.n_cams, q.lm_off, q.cam_idx, q.obs)
    ctx.set_cameras(q.cams)
    ctx.init_landmarks_pose(L.ALPHA)
    assert ctx.linearize_pose(L.ALPHA)
    want, rc = ctx.observation_covariance(step=1, lam=0.0, gauge=0)
    want_lm, rc_lm = ctx.landmark_covariance(step=1, lam=0.0, gauge=0, coords=0)
    ctx.close()
    assert rc == 0 and rc_lm == 0
    print(f"bal against the ABI call: {rel(rows, want):.2e}; sum h = {rows[:, 0].sum():.9f}, rank {12 * q.n_cams + 3 * n_lms - 12}")
    assert rel(rows, want) < 1e-9
    os.remove(out)
    # with the landmark file, and from two shards
    run(still + ["--observation-covariance-path", out, "--landmark-covariance-path", lm_out])
    assert rel(_read_rows(out, q.lm_off, q.cam_idx), want) < 1e-9
    lm_lines = open(lm_out).read().split("\n")
    assert int(lm_lines[0]) == n_lms
    lm_blocks = np.array([[float(x) for x in ln.split()] for ln in lm_lines[1:1 + n_lms]]).reshape(n_lms, 3, 3)
    assert rel(lm_blocks, want_lm) < 1e-9
    os.remove(out)
    run(still + ["--observation-covariance-path", out, "--gpus", "2"])
    assert rel(_read_rows(out, q.lm_off, q.cam_idx), want) < 1e-9
    os.remove(out)
    # after both steps
    run(["--max-num-iterations-step-1", "8", "--max-num-iterations-step-2", "4", "--observation-covariance-path", out])
    rows = _read_rows(out, q.lm_off, q.cam_idx)
    print(f"after both steps: sum h = {rows[:, 0].sum():.9f}, rank {11 * q.n_cams + 3 * n_lms - 15}")
    assert np.all(rows[:, 0] > 0) and np.all(rows[:, 0] < 2) and np.all(rows[:, 1] > 0) and np.all(rows[:, 3] > 0)
