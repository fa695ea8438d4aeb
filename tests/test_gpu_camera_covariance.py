"""Per-camera marginal covariance (povar_camera_covariance_pose / _joint) against the long-double reference of
tests/covariance_reference.py, through the C ABI.

Tolerance, both modes, per block: |C^_cc - C_cc|_F <= n u cond_2(A) |A^-1|_2 with A the factored matrix (S(lambda), or
S0 + Q Q^T in the free gauge), n its dimension, u = 2^-53: the first-order bound of an inverse through a Cholesky factor
with the classical factor n; cond_2 and |A^-1|_2 from the reference matrix.  In camera coordinates the bound is carried
through the map: times max sigma_c^2.  Every case prints its worst ratio error / (u cond_2 |A^-1|_2) (DESIGN.md section 3
records them); the bound is not tightened to it.
"""
import os
import subprocess

import numpy as np
import pytest

import covariance_reference as R
from conftest import rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 1e-4
HUBER = {1: 30.0, 2: 0.5}  # as tests/test_gpu_sc_solvers.py


def _context(name, step, norm="NONE"):
    from povar_amd import capi
    p = R.problem(name)
    if step == 1:
        _, sigma, cams, lms, _ = _system(name, 1, 1.0, norm)
        ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=norm, huber=HUBER[1])
        ctx.set_cameras(cams)
        ctx.set_landmarks(lms)
        ctx.set_jl_col_scaling(False)
        assert ctx.linearize_pose(R.ALPHA)
    else:
        cams, lms_h, obs = R.state2(p)
        ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs, robust_norm=norm, huber=HUBER[2])
        ctx.set_cameras(cams)
        ctx.set_landmarks_homogeneous(lms_h)
        assert ctx.linearize_homogeneous()
    return ctx


_SYSTEMS = {}


def _system(name, step, lam, norm="NONE"):
    key = (name, step, lam, norm)
    if key not in _SYSTEMS:
        p = R.problem(name)
        _SYSTEMS[key] = R.system_pose(p, lam, norm, HUBER[1]) if step == 1 else R.system_joint(p, lam, norm, HUBER[2])
    return _SYSTEMS[key]


_REFS = {}


def _reference(name, step, lam, free_gauge, norm="NONE"):
    """(Reference, sigma, cams): computed once, shared, never modified."""
    key = (name, step, lam, free_gauge, norm)
    if key not in _REFS:
        sys_ = _system(name, step, lam, norm)
        S, sigma, cams = sys_[0], sys_[1], sys_[2]
        Q = None
        if free_gauge:
            Q = R.orthonormal(R.gauge_basis_pose(cams, sigma) if step == 1 else R.gauge_basis_joint(cams, sigma))
        _REFS[key] = (R.Reference(S, 12 if step == 1 else 11, Q), sigma, cams)
    return _REFS[key]


def _check(tag, got, rc, ref, sigma, cams, step, coords):
    """The bound and the properties of one returned set of blocks."""
    from povar_amd import capi
    assert rc == 0, tag
    dim = 12 if (step == 1 or coords == capi.COV_CAMERA_COORDS) else 11
    assert got.shape == (sigma.shape[0], dim, dim) and np.all(np.isfinite(got))
    want, bound, unit = ref.blocks, ref.bound, ref.unit
    if coords == capi.COV_CAMERA_COORDS:
        want = R.to_camera_coords(want, sigma, step, cams)
        scale = float(sigma.max() ** 2)
        bound, unit = bound * scale, unit * scale
    err = np.linalg.norm((got.astype(np.longdouble) - want).astype(np.float64), axis=(1, 2))
    print(f"{tag}: n {ref.n} cond {ref.cond:.3g} |A^-1| {ref.inv_norm:.3g} worst block error {err.max():.3e} "
          f"= {err.max() / unit:.3g} x u cond |A^-1| (bound: {ref.n} x)")
    assert np.all(err <= bound), (tag, err.max(), bound)
    # exactly symmetric, positive semidefinite within the bound
    assert np.array_equal(got, got.transpose(0, 2, 1)), tag
    assert np.linalg.eigvalsh(got).min() >= -bound, tag
    if step == 2 and coords == capi.COV_CAMERA_COORDS:
        # rank 11: the camera's own direction is no degree of freedom: block (h0 / sigma_c) = 0
        w, beta = R.householder(cams)
        h0 = R.reflectors(w, beta)[:, :, 0]
        resid = np.einsum("cij,cj->ci", got, h0 / sigma)
        assert np.all(np.linalg.norm(resid, axis=1) <= bound * np.linalg.norm(h0 / sigma, axis=1)), tag
        ev = np.linalg.eigvalsh(got)
        assert np.all(np.abs(ev[:, 0]) <= bound) and np.all(ev[:, 1] > bound), tag
    return float(err.max() / unit)


FREE_CASES = [(1, "small", "NONE"), (1, "p24", "NONE"), (2, "small", "NONE"), (2, "p24", "NONE"), (2, "p22", "NONE"),
              (1, "small", "HUBER"), (2, "small", "HUBER")]


@pytest.mark.parametrize("coords", [0, 1], ids=["camera", "solver"])
@pytest.mark.parametrize("step,name,norm", FREE_CASES)
def test_free_gauge(step, name, norm, coords):
    """small: N = 128, two panels, camera 5 straddles column 64; p24: N = 320, five panels, across the 256-row outer block;
    p22 in step 2: n = 242, N = 256, the matrix ends on the outer block's edge."""
    ref, sigma, cams = _reference(name, step, 0.0, True, norm)
    ctx = _context(name, step, norm)
    got, rc = ctx.camera_covariance(step=step, lam=0.0, gauge=0, coords=coords)
    _check(f"free gauge step {step} {name} {norm} coords {coords}", got, rc, ref, sigma, cams, step, coords)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_free_gauge_after_a_lane_per_landmark_linearisation(step, monkeypatch):
    """POVAR_E0_V1=0: the per-slot arrays the assembly reads come from the lane-per-landmark linearisation (ensure_legacy)."""
    monkeypatch.setenv("POVAR_E0_V1", "0")
    ref, sigma, cams = _reference("small", step, 0.0, True)
    ctx = _context("small", step)
    got, rc = ctx.camera_covariance(step=step, lam=0.0, gauge=0, coords=1)
    _check(f"free gauge step {step} small lane-per-landmark", got, rc, ref, sigma, cams, step, 1)
    ctx.close()


@pytest.mark.parametrize("lam", [1e-4, 1.0])
@pytest.mark.parametrize("name", ["small", "medium"])
@pytest.mark.parametrize("step", [1, 2])
def test_damped(step, name, lam):
    """medium: n = 588 / 539, N = 640 / 576: three outer blocks."""
    ref, sigma, cams = _reference(name, step, lam, False)
    ctx = _context(name, step)
    for coords in (1, 0):
        got, rc = ctx.camera_covariance(step=step, lam=lam, gauge=1, coords=coords)
        _check(f"damped step {step} {name} lambda {lam:g} coords {coords}", got, rc, ref, sigma, cams, step, coords)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_solver_and_camera_coordinates_agree(step):
    """Two calls on one linearisation, solver blocks mapped on the host vs the device's camera blocks: 1e-13 relative.
    The interface returns one coordinate system per call, and the assembly adds with atomics, so the two calls differ by
    the order of those adds; that is why this runs in the free gauge on small_problem, where cond_2(S0 + Q Q^T) is 272
    (step 1) and 128 (step 2): measured 1.1e-15 and 6.6e-15."""
    _, sigma, cams = _reference("small", step, 0.0, True)
    ctx = _context("small", step)
    ts, rc_s = ctx.camera_covariance(step=step, lam=0.0, gauge=0, coords=1)
    tc, rc_c = ctx.camera_covariance(step=step, lam=0.0, gauge=0, coords=0)
    assert rc_s == 0 and rc_c == 0
    mapped = R.to_camera_coords(ts, sigma, step, cams)
    print(f"step {step}: rel(camera blocks, mapped solver blocks) {rel(tc, mapped):.3e}")
    assert rel(tc, mapped) <= 1e-13
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_free_gauge_reports_degeneracy_beyond_the_gauge(step):
    """medium_problem: null dimension 21 / 30 instead of 12 / 15: POVAR_NUMERIC_FAILURE and all-NaN blocks."""
    from povar_amd import capi
    ctx = _context("medium", step)
    for coords in (0, 1):
        got, rc = ctx.camera_covariance(step=step, lam=0.0, gauge=0, coords=coords)
        assert rc == capi.NUMERIC_FAILURE and np.all(np.isnan(got))
    ctx.close()


def test_argument_errors():
    from povar_amd import capi
    p = R.problem("small")
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(R.ALPHA)
    out = np.zeros(144 * p.n_cams)

    def call(step, lam, gauge, coords):
        import ctypes as C
        fn = ctx.L.povar_camera_covariance_pose if step == 1 else ctx.L.povar_camera_covariance_joint
        return fn(ctx.h, C.c_double(lam), C.c_int32(gauge), C.c_int32(coords), C.c_void_p(out.ctypes.data))

    # no linearisation in force
    assert call(1, 0.0, 0, 0) < 0 and call(2, 0.0, 0, 0) < 0
    assert ctx.linearize_pose(R.ALPHA)
    assert call(2, 0.0, 0, 0) < 0  # step 1's linearisation does not serve step 2
    assert call(1, 1e-4, capi.COV_FREE_GAUGE, 0) < 0   # free gauge with lambda != 0
    assert call(1, 0.0, capi.COV_DAMPED, 0) < 0 and call(1, -1.0, capi.COV_DAMPED, 0) < 0  # damped with lambda <= 0
    assert call(1, 0.0, 2, 0) < 0 and call(1, 0.0, 0, 2) < 0 and call(1, 0.0, -1, 0) < 0  # unknown enum values
    with pytest.raises(capi.PovarError):
        ctx.camera_covariance(step=1, lam=1.0, gauge=capi.COV_FREE_GAUGE)
    assert call(1, 0.0, 0, 0) == 0
    ctx.close()


def test_solvers_unchanged_after_a_covariance_call():
    """The in-place inverse and the Q Q^T add leak nothing into the next assembly: CHOLESKY / RICHOLESKY on the same context
    still match the oracle's cholesky_solve (tolerance of test_cholesky_pose: 1e-8)."""
    from povar_amd import capi
    from oracle import povar_oracle as O
    p = R.problem("small")
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    for step in (1, 2):
        sys_ = _system("small", step, LAM)
        S, b = sys_[0], sys_[-1]
        ref, bad = orc.cholesky_solve(S, b)
        assert bad == 0
        ctx = _context("small", step)
        for gauge, lam in ((capi.COV_FREE_GAUGE, 0.0), (capi.COV_DAMPED, 1.0)):
            _, rc = ctx.camera_covariance(step=step, lam=lam, gauge=gauge)
            assert rc == 0
            if step == 1:
                inc, it, status, rc = ctx.solve_pose_sc(LAM, capi.SC_CHOLESKY)
            else:
                inc, it, status, rc = ctx.solve_joint_sc(LAM, method=capi.SC_CHOLESKY)
            assert rc == 0 and it == 0
            assert rel(inc, ref) < 1e-8, (step, gauge)
        ctx.close()


def test_bal_writes_the_camera_covariance(tmp_path):
    """`bal --camera-covariance-path`: n_cams, then one line of 144 numbers per camera: finite, symmetric, positive
    semidefinite blocks at the final state of the last step that ran: step 2, or step 1 when step 2 gets no iteration.
    The flag changes nothing the log records."""
    from povar_amd import synth
    p = synth.make_problem(10, 300, 1300, seed=21)
    f = str(tmp_path / "problem-10-300.txt")
    synth.write_data_custom(f, p)
    out = str(tmp_path / "cov.txt")
    base = [os.path.join(ROOT, "bin/bal"), "--input", f, "--quiet", "--max-num-iterations-step-1", "8",
            "--power-sc-iterations", "20"]
    written = {}
    for step2_iterations in ("4", "0"):
        log = str(tmp_path / f"log{step2_iterations}.json")
        cmd = base + ["--max-num-iterations-step-2", step2_iterations, "--log-log-path", log, "--camera-covariance-path", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = open(out).read().split("\n")
        assert int(lines[0]) == p.n_cams
        blocks = np.array([[float(x) for x in ln.split()] for ln in lines[1:1 + p.n_cams]])
        assert blocks.shape == (p.n_cams, 144) and np.all(np.isfinite(blocks))
        blocks = blocks.reshape(p.n_cams, 12, 12)
        assert np.array_equal(blocks, blocks.transpose(0, 2, 1))
        ev = np.linalg.eigvalsh(blocks)
        assert np.all(ev[:, 0] >= -1e-9 * ev[:, -1]) and np.all(ev[:, -1] > 0)
        # step 1's blocks have full rank (step 2's have rank 11: the camera's own direction is no degree of freedom)
        assert step2_iterations != "0" or np.all(ev[:, 0] > 0)
        written[step2_iterations] = blocks
        os.remove(out)  # the next run has to write its own
    assert not np.array_equal(written["4"], written["0"])
    # the covariance is taken after the summary is finished: the evaluation counts of the log do not see it
    r = subprocess.run(base + ["--max-num-iterations-step-2", "4", "--log-log-path", str(tmp_path / "plain.json")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    import json
    with_flag, plain = json.load(open(tmp_path / "log4.json")), json.load(open(tmp_path / "plain.json"))
    assert with_flag["_static"]["solver"]["num_jacobian_evaluations"] == plain["_static"]["solver"]["num_jacobian_evaluations"]
    cmd = base + ["--max-num-iterations-step-2", "4", "--camera-covariance-path", out]
    # --gpus > 1 does not serve the flag
    r = subprocess.run(cmd + ["--gpus", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--camera-covariance-path" in r.stderr
