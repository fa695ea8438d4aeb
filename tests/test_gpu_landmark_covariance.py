"""Per-landmark marginal covariance (povar_landmark_covariance_pose / _joint) against the long-double reference of
tests/landmark_covariance_reference.py, through the C ABI.

Tolerance, both modes, per block: |Sigma^_l - Sigma_l|_F <= m u cond_2(K) |K^-1|_2 with K the full matrix that is actually
inverted (H0 + Cg Cg^T with Cg = [Q; 0] in the free gauge, H(lambda) damped), m its dimension, u = 2^-53: the camera test's
first-order rule carried to the full system; times max s_l^2 in landmark coordinates.  tests/test_landmark_covariance_reference.py
holds every case here to bound <= 1e-4 |Sigma_l|_F.  Every case prints its worst ratio error / (u cond_2 |K^-1|_2) (DESIGN.md
section 3 records them); the bound is not tightened to it.  The camera blocks of a with_cameras call are held to the camera
test's own bound.  Step 1 runs with the Jl column scaling on (the library's default), so both coordinate systems differ.
"""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import covariance_reference as R
import landmark_covariance_reference as L
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


def _check(tag, got, rc, ref, coords, ids=None):
    """The bound and the properties of one returned set of landmark blocks; the worst error in units of u cond |K^-1|."""
    assert rc == 0, tag
    landmark_coords = coords == 0
    want = ref.want(landmark_coords)
    if ids is not None:
        want = want[np.asarray(ids)]
    d = 4 if (ref.sys.step == 2 and landmark_coords) else 3
    assert got.shape == (want.shape[0], d, d) and np.all(np.isfinite(got)), tag
    scale = ref.scale(landmark_coords)
    err = np.linalg.norm((got.astype(np.longdouble) - want).astype(np.float64), axis=(1, 2))
    print(f"{tag}: m {ref.m} cond {ref.cond:.3g} |K^-1| {ref.inv_norm:.3g} worst block error {err.max():.3e} "
          f"= {err.max() / (ref.unit * scale):.3g} x u cond |K^-1| (bound: {ref.m} x)")
    assert np.all(err <= ref.bound * scale), (tag, err.max(), ref.bound * scale)
    assert np.array_equal(got, got.transpose(0, 2, 1)), tag  # symmetric bit for bit
    return float(err.max() / (ref.unit * scale))


def _check_cameras(tag, got, ref, coords):
    """The camera blocks of the same call, under the bound of tests/test_gpu_camera_covariance.py."""
    cref, s = ref.cameras, ref.sys
    want, bound = cref.blocks, cref.bound
    if coords == 0:
        want = R.to_camera_coords(want, s.sigma, s.step, s.cams)
        bound = bound * float(s.sigma.max() ** 2)
    assert got.shape == want.shape and np.all(np.isfinite(got)), tag
    err = np.linalg.norm((got.astype(np.longdouble) - want).astype(np.float64), axis=(1, 2))
    print(f"{tag}: camera blocks, worst error {err.max():.3e} (bound {bound:.3e})")
    assert np.all(err <= bound), (tag, err.max(), bound)
    assert np.array_equal(got, got.transpose(0, 2, 1)), tag


FREE_CASES = [(1, "small", "NONE"), (2, "small", "NONE"), (1, "p22", "NONE"), (2, "p22", "NONE"), (1, "p24", "NONE"),
              (2, "p24", "NONE"), (1, "small", "HUBER"), (2, "small", "HUBER")]


@pytest.mark.parametrize("coords", [0, 1], ids=["landmark", "solver"])
@pytest.mark.parametrize("step,name,norm", FREE_CASES)
def test_free_gauge(step, name, norm, coords):
    """small: n = 72 / 66, N = 128: two block rows, camera 5 straddles the 64-edge in both steps; p22, p24: N = 320 (step 2
    of p22: 256): the K loop of cov_lauum and its off-diagonal tiles run."""
    ref = L.reference(name, step, norm, 0.0, True)
    ctx = _context(name, step, norm)
    tag = f"free gauge step {step} {name} {norm} coords {coords}"
    got, cam, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=coords, with_cameras=True)
    _check(tag + " all", got, rc, ref, coords)
    _check_cameras(tag, cam, ref, coords)
    rng = np.random.default_rng(step + 10 * coords)
    ids = rng.permutation(ref.sys.n_lms)[:ref.sys.n_lms // 3]
    sub, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=coords, ids=ids)
    _check(tag + " shuffled subset", sub, rc, ref, coords, ids)
    dup = np.array([7, 3, 7, 0, ref.sys.n_lms - 1, 3])
    twice, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=coords, ids=dup)
    _check(tag + " duplicates", twice, rc, ref, coords, dup)
    # given C a block is reproducible: the rows of one id in one call are the same bits
    assert np.array_equal(twice[0], twice[2]) and np.array_equal(twice[1], twice[5])
    # no landmark, cameras only
    none, cam2, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=coords, ids=np.zeros(0, dtype=np.int32),
                                             with_cameras=True)
    assert rc == 0 and none.shape[0] == 0
    _check_cameras(tag + " n_ids = 0", cam2, ref, coords)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_free_gauge_after_a_lane_per_landmark_linearisation(step, monkeypatch):
    """POVAR_E0_V1=0: the per-slot arrays the staging reads come from the lane-per-landmark linearisation (ensure_legacy)."""
    monkeypatch.setenv("POVAR_E0_V1", "0")
    ref = L.reference("small", step, "NONE", 0.0, True)
    ctx = _context("small", step)
    assert ctx.layout_info().lane_per_landmark == 1
    for coords in (1, 0):
        got, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=coords)
        _check(f"free gauge step {step} small lane-per-landmark coords {coords}", got, rc, ref, coords)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_long_tracks(step):
    """Two landmarks of >= 65 observations and three of 33..64: both chunk loops of both stagings (chunks of 64 and 32) take
    more than one trip; N = 832 / 768."""
    s = L.system("long", step)
    assert np.sum(s.track >= 65) == 2 and np.sum((s.track >= 33) & (s.track <= 64)) == 3
    assert (s.n + 63) // 64 * 64 == (832 if step == 1 else 768)
    ref = L.reference("long", step, "NONE", 0.0, True)
    ctx = _context("long", step)
    for coords in (1, 0):
        got, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=coords)
        _check(f"long tracks step {step} coords {coords}", got, rc, ref, coords)
    ids = np.flatnonzero(s.track >= 33)[::-1]
    got, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=1, ids=ids)
    _check(f"long tracks step {step}: the five long ones", got, rc, ref, 1, ids)
    ctx.close()


@pytest.mark.parametrize("lam", [1e-4, 1.0])
@pytest.mark.parametrize("name", ["small", "medium"])
@pytest.mark.parametrize("step", [1, 2])
def test_damped(step, name, lam):
    """medium: n = 588 / 539, N = 640 / 576."""
    ref = L.reference(name, step, "NONE", lam, False)
    ctx = _context(name, step)
    for coords in (1, 0):
        got, cam, rc = ctx.landmark_covariance(step=step, lam=lam, gauge=1, coords=coords, with_cameras=True)
        _check(f"damped step {step} {name} lambda {lam:g} coords {coords}", got, rc, ref, coords)
        _check_cameras(f"damped step {step} {name} lambda {lam:g} coords {coords}", cam, ref, coords)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_step1_scaling_off_and_step2_null_vector(step):
    """Step 1 with povar_set_jl_col_scaling(0): D = I, both coordinate systems give the same block.  Step 2, landmark
    coordinates: rank 3 with null vector X_l / s_l."""
    from povar_amd import capi
    p = L.problem("small")
    if step == 1:
        s = L.System(p, 1, jl_scaling=False)
        ref = L.Reference(s, 0.0, True)
        ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs)
        ctx.set_jl_col_scaling(False)
        _linearise(ctx, 1, s.cams, s.lms)
        a, rc_a = ctx.landmark_covariance(step=1, lam=0.0, gauge=0, coords=1)
        b, rc_b = ctx.landmark_covariance(step=1, lam=0.0, gauge=0, coords=0)
        _check("step 1, column scaling off, solver coords", a, rc_a, ref, 1)
        _check("step 1, column scaling off, landmark coords", b, rc_b, ref, 0)
    else:
        ref = L.reference("small", 2, "NONE", 0.0, True)
        s = ref.sys
        ctx = _context("small", 2)
        got, rc = ctx.landmark_covariance(step=2, lam=0.0, gauge=0, coords=0)
        _check("step 2 landmark coords", got, rc, ref, 0)
        bound = ref.bound * ref.scale(True)
        x = s.lms / s.s
        resid = np.einsum("lij,lj->li", got, x)
        assert np.all(np.linalg.norm(resid, axis=1) <= bound * np.linalg.norm(x, axis=1))
        ev = np.linalg.eigvalsh(got)
        assert np.all(np.abs(ev[:, 0]) <= bound) and np.all(ev[:, 1] > bound)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_two_calls_agree_within_the_bound(step):
    """Not bit for bit: the assembly of S adds with atomics."""
    ref = L.reference("small", step, "NONE", 0.0, True)
    ctx = _context("small", step)
    a, rc_a = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=1)
    b, rc_b = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=1)
    assert rc_a == 0 and rc_b == 0
    diff = np.linalg.norm(a - b, axis=(1, 2))
    print(f"step {step}: two calls differ by at most {diff.max():.3e} (bound {ref.bound:.3e})")
    assert np.all(diff <= ref.bound)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_free_gauge_reports_degeneracy_beyond_the_gauge(step):
    """medium_problem: null dimension 21 / 30 instead of 12 / 15: POVAR_NUMERIC_FAILURE and every output NaN."""
    from povar_amd import capi
    ctx = _context("medium", step)
    for coords in (0, 1):
        got, cam, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=coords, with_cameras=True)
        assert rc == capi.NUMERIC_FAILURE and got.size > 0 and np.all(np.isnan(got)) and np.all(np.isnan(cam))
    ctx.close()


def test_argument_errors():
    from povar_amd import capi
    p = L.problem("small")
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(L.ALPHA)
    n_lms = p.lm_off.shape[0] - 1
    out = np.zeros(16 * n_lms)

    def call(step, lam, gauge, coords, ids=None, null_out=False):
        fn = ctx.L.povar_landmark_covariance_pose if step == 1 else ctx.L.povar_landmark_covariance_joint
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        return fn(ctx.h, C.c_double(lam), C.c_int32(gauge), C.c_int32(coords), None if ids is None else C.c_void_p(ids.ctypes.data),
                  C.c_int32(0 if ids is None else ids.shape[0]), None if null_out else C.c_void_p(out.ctypes.data), None)

    # no linearisation in force
    assert call(1, 0.0, 0, 0) < 0 and call(2, 0.0, 0, 0) < 0
    assert ctx.linearize_pose(L.ALPHA)
    assert call(2, 0.0, 0, 0) < 0  # step 1's linearisation does not serve step 2
    assert call(1, 1e-4, capi.COV_FREE_GAUGE, 0) < 0   # free gauge with lambda != 0
    assert call(1, 0.0, capi.COV_DAMPED, 0) < 0 and call(1, -1.0, capi.COV_DAMPED, 0) < 0  # damped with lambda <= 0
    assert call(1, 0.0, 2, 0) < 0 and call(1, 0.0, 0, 2) < 0 and call(1, 0.0, -1, 0) < 0  # unknown enum values
    assert call(1, 0.0, 0, 0, ids=[0, n_lms]) < 0 and call(1, 0.0, 0, 0, ids=[-1]) < 0  # id out of range
    assert call(1, 0.0, 0, 0, ids=[0, 1], null_out=True) < 0 and call(1, 0.0, 0, 0, null_out=True) < 0  # null lm_cov, n > 0
    with pytest.raises(capi.PovarError):
        ctx.landmark_covariance(step=1, lam=1.0, gauge=capi.COV_FREE_GAUGE)
    assert capi.COV_LANDMARK_COORDS == capi.COV_CAMERA_COORDS == 0
    assert call(1, 0.0, 0, 0) == 0 and call(1, 0.0, 0, 0, ids=[n_lms - 1, 0]) == 0
    ctx.close()


def test_solvers_unchanged_after_a_landmark_covariance_call():
    """cov_lauum writes the strictly lower blocks and the scratch panel, the Q Q^T add and the inverse the upper ones: nothing
    leaks into the next assembly.  CHOLESKY / RICHOLESKY increments after the call match those before it (the assembly adds
    with atomics: 1e-8, the tolerance of the camera test), and POVAR_BUF_SC_FACTOR is an argument error until the next
    direct solve."""
    from povar_amd import capi
    for step in (1, 2):
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
        for gauge, lam in ((capi.COV_FREE_GAUGE, 0.0), (capi.COV_DAMPED, 1.0)):
            _, rc = ctx.landmark_covariance(step=step, lam=lam, gauge=gauge)
            assert rc == 0
            with pytest.raises(capi.PovarError):
                ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
            after = solve()
            assert rel(after, before) < 1e-8, (step, gauge)
            ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
        ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_sharded_matches_single(step):
    """Two shard contexts on one device through the host all-reduce hook: every rank calls with ids of its own shard."""
    from povar_amd import capi
    from test_gpu_sharded import HostAllReduce
    p = L.problem("p22")
    ref = L.reference("p22", step, "NONE", 0.0, True)
    cams, lms, obs = L.state(p, step)
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
            got, cam, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=0, with_cameras=True)
            some = np.arange(le - lb)[::-3]
            sub, rc_sub = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=1, ids=some)
            out[rank] = (lb, le, got, cam, rc, some, sub, rc_sub)
            ctx.close()
        except BaseException:
            ar.bar.abort()  # a failed rank must not leave the other one waiting
            raise

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert all(o is not None for o in out)
    covered = 0
    for rank, (lb, le, got, cam, rc, some, sub, rc_sub) in enumerate(out):
        ids = np.arange(lb, le)
        _check(f"sharded step {step} rank {rank}", got, rc, ref, 0, ids)
        _check(f"sharded step {step} rank {rank} subset", sub, rc_sub, ref, 1, ids[some])
        _check_cameras(f"sharded step {step} rank {rank}", cam, ref, 0)
        covered += le - lb
    assert covered == ref.sys.n_lms


def _read_blocks(path, count, width):
    lines = open(path).read().split("\n")
    assert int(lines[0]) == count
    blocks = np.array([[float(x) for x in ln.split()] for ln in lines[1:1 + count]])
    assert blocks.shape == (count, width) and np.all(np.isfinite(blocks))
    d = int(round(width ** 0.5))
    blocks = blocks.reshape(count, d, d)
    assert np.array_equal(blocks, blocks.transpose(0, 2, 1))
    return blocks


def test_bal_writes_the_landmark_covariance(tmp_path):
    """`bal --landmark-covariance-path`: n_lms, then one line per landmark (9 numbers after step 1, 16 after step 2): the
    free-gauge blocks in landmark coordinates at the final state of the last step that ran.  With no LM iteration in either
    step the final state is the one a caller can set up too (the file's cameras, the initialised landmarks): there the file
    agrees with the ABI call, and so does the camera file written by the same call.  After iterations of both steps: n_lms
    4 x 4 blocks of rank 3.  --gpus 2: every shard writes its own landmarks, the same file."""
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

    out, cam_out = str(tmp_path / "lm.txt"), str(tmp_path / "cam.txt")
    still = ["--max-num-iterations-step-1", "0", "--max-num-iterations-step-2", "0"]
    run(still + ["--landmark-covariance-path", out, "--camera-covariance-path", cam_out])
    blocks, cam_blocks = _read_blocks(out, n_lms, 9), _read_blocks(cam_out, q.n_cams, 144)
    ctx = capi.Context(q.n_cams, q.lm_off, q.cam_idx, q.obs)
    ctx.set_cameras(q.cams)
    ctx.init_landmarks_pose(L.ALPHA)
    assert ctx.linearize_pose(L.ALPHA)
    want, want_cam, rc = ctx.landmark_covariance(step=1, lam=0.0, gauge=0, coords=0, with_cameras=True)
    ctx.close()
    assert rc == 0
    print(f"bal against the ABI call: landmarks {rel(blocks, want):.2e}, cameras {rel(cam_blocks, want_cam):.2e}")
    assert rel(blocks, want) < 1e-9 and rel(cam_blocks, want_cam) < 1e-9
    # the landmark file alone, and from two shards
    os.remove(out)
    run(still + ["--landmark-covariance-path", out])
    assert rel(_read_blocks(out, n_lms, 9), want) < 1e-9
    os.remove(out)
    run(still + ["--landmark-covariance-path", out, "--gpus", "2"])
    assert rel(_read_blocks(out, n_lms, 9), want) < 1e-9
    os.remove(out)
    # after both steps: homogeneous blocks of rank 3
    run(["--max-num-iterations-step-1", "8", "--max-num-iterations-step-2", "4", "--landmark-covariance-path", out])
    ev = np.linalg.eigvalsh(_read_blocks(out, n_lms, 16))
    assert np.all(ev[:, -1] > 0) and np.all(np.abs(ev[:, 0]) <= 1e-9 * ev[:, -1]) and np.all(ev[:, 1] > 1e-9 * ev[:, -1])
