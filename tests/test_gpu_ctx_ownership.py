"""A context owns its device memory (povar_amd/csrc/dev_buf.hpp, ~povar_ctx): a creation that is refused half-way frees what
it had allocated, and closing a context frees every buffer it allocated after povar_create -- the explicit-SC and dense
solvers, the covariance calls, the rows a host thread placed, the tile buffer of an export.  Measured as the device's free
bytes over repeated rounds, against a bound that is half of what a leak would take (pool noise cannot pass for a leak, nor
a leak for noise).  tests/test_host_dev_buf.py holds the buffer type itself, without a device."""
import numpy as np
import pytest

from test_gpu_state_tracking import _free_device_bytes

pytestmark = pytest.mark.gpu

ALPHA, LAM, M = 0.01, 1e-4, 6
_KNOBS = ("POVAR_DETERMINISTIC", "POVAR_DET_CK", "POVAR_FP32_TERMS", "POVAR_E0_CK", "POVAR_RES", "POVAR_E0_V1", "POVAR_NO_CK",
          "POVAR_LPL_PLACE", "POVAR_LPL_NOPLACE", "POVAR_CK_MAX_CAMS", "POVAR_CU_MASK")


@pytest.fixture(scope="module")
def problem():
    from povar_amd import synth
    return synth.make_problem(300, 60000, 300000, seed=4)   # (the size of the placement tests of test_gpu_state_tracking.py)


@pytest.fixture(autouse=True)
def _own_environment(monkeypatch):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)


def _create(p, **kw):
    from povar_amd import capi
    return capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, e0_mode=capi.E0_IMPLICIT_LDSACC, **kw)


def test_a_creation_refused_after_the_uploads_frees_everything(problem, monkeypatch):
    """POVAR_NO_CK=1 with POVAR_FLAG_FP32_TERMS: povar_create refuses once it finds no camera-chunk layout, AFTER every upload of
    the lane-per-landmark layout.  A context leaked there holds at least B = n_rows * 64 * 16 bytes (its image points alone);
    24 refused creations may cost the device less than 12 B."""
    from povar_amd import capi
    p = problem
    monkeypatch.setenv("POVAR_NO_CK", "1")
    twin = _create(p)
    B = twin.layout_info().n_rows * 64 * 16
    twin.close()
    assert B > (1 << 20)

    def refused(n):
        for _ in range(n):
            with pytest.raises(capi.PovarError, match="POVAR_FLAG_FP32_TERMS: the camera-chunk layout could not be built"):
                _create(p, flags=capi.FLAG_FP32_TERMS)
        return _free_device_bytes()

    free8 = refused(8)
    free32 = refused(24)
    print(f"refused late: B = {B} bytes, free after 8: {free8}, after 32: {free32}, drop {free8 - free32} (bound {12 * B})")
    assert free8 - free32 < 12 * B


def test_a_creation_refused_at_once_frees_everything(problem):
    """POVAR_FLAG_DETERMINISTIC with POVAR_FLAG_FP32_TERMS is refused before any layout exists (the stream does): 32 times, and
    a context created afterwards works."""
    from povar_amd import capi
    p = problem
    for _ in range(32):
        with pytest.raises(capi.PovarError, match="POVAR_FLAG_FP32_TERMS cannot be combined with POVAR_FLAG_DETERMINISTIC"):
            _create(p, flags=capi.FLAG_DETERMINISTIC | capi.FLAG_FP32_TERMS)
    ctx = _create(p)
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(ALPHA)
    assert ctx.linearize_pose(ALPHA)
    inc, it, _, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
    assert rc == 0 and it == M and np.all(np.isfinite(inc)) and np.linalg.norm(inc) > 0
    ctx.close()


def _round(p, small):
    """Every family of allocation that comes after povar_create, then close: (device_bytes of the large context, free bytes)."""
    from povar_amd import capi
    ctx = _create(p)
    assert ctx.layout_info().placement == 2
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(ALPHA)
    assert ctx.linearize_pose(ALPHA)
    assert ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)[3] == 0                       # a step-1 series
    assert ctx.layout_finalize(wait=True) and ctx.layout_info().placement == 3      # the placed rows swapped in
    assert ctx.linearize_pose(ALPHA)
    assert ctx.solve_pose_sc(LAM, capi.SC_CHOLESKY)[3] == 0                         # CHOLESKY
    assert ctx.get_buffer(capi.BUF_STORAGE).shape == (64 * p.n_obs,)                # the tiles of the export
    lms = ctx.get_landmarks()
    ctx.set_landmarks_homogeneous(np.concatenate([lms, np.ones((p.n_lms, 1))], axis=1))
    ctx.normalize_joint()
    assert ctx.linearize_homogeneous()
    assert ctx.solve_joint(LAM, M)[3] == 0                                          # a step-2 series
    assert ctx.solve_joint_sc(LAM, method=capi.SC_CHOLESKY)[3] == 0                 # RICHOLESKY
    held = ctx.device_bytes()
    ctx.close()
    # the covariance calls, on a problem of the dense tests' size
    cov = capi.Context(small.n_cams, small.lm_off, small.cam_idx, small.obs)
    cov.set_cameras(small.cams)
    cov.init_landmarks_pose(ALPHA)
    assert cov.linearize_pose(ALPHA)
    blocks, rc = cov.camera_covariance(step=1, lam=LAM, gauge=capi.COV_DAMPED)
    assert rc == 0 and np.all(np.isfinite(blocks))
    blocks, rc = cov.landmark_covariance(step=1, lam=LAM, gauge=capi.COV_DAMPED)
    assert rc == 0 and np.all(np.isfinite(blocks))
    rows, rc = cov.observation_covariance(step=1, lam=LAM, gauge=capi.COV_DAMPED)
    assert rc == 0 and np.all(np.isfinite(rows))
    cov.close()
    return held, _free_device_bytes()


def test_close_frees_what_every_late_allocation_took(problem, monkeypatch):
    """Six rounds of create, use everything, close: from the second round to the sixth the device loses less than what ONE
    such context holds (a buffer left behind by every close would take four times its size)."""
    from povar_amd import synth
    monkeypatch.setenv("POVAR_LPL_PLACE", "async")
    monkeypatch.setenv("POVAR_E0_V1", "0")
    small = synth.make_problem(29, 400, 2400, seed=11, popularity="uniform")
    free, held = [], 0
    for _ in range(6):
        held, f = _round(problem, small)
        free.append(f)
    print(f"teardown: one context holds {held} bytes; free bytes after rounds 1..6: {free}; drop 2 -> 6: {free[1] - free[5]}")
    assert free[1] - free[5] < held
