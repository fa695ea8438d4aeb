"""The two camera tails of a power-series term against each other: cam_cold_sum_binv[_h] (one kernel: gather, B^-1, AXPY, z) and
cam_cold_sum + cam_binv_axpy[_h] (POVAR_NO_FUSE=1: the gather leaves the dense y, the second kernel reads it back).  Both run
the same gather (cam_row_sum) and the same products in the same order behind it (povar_kernels_cam.hpp), and under
POVAR_DETERMINISTIC=1 the E0 kernels in front of them are bit-reproducible across contexts, so the two tails must leave the
SAME BITS: every term, the 20-term increment, and the iteration count and status of an early exit.

Measured before the per-camera kernels were given one body (cam_cold_sum_binv, cam_cold_sum_binv_h and cam_binv_axpy[_h]
as separate copies): the two tails agreed bit for bit in all 8 cases, so the assertion is np.array_equal, not a tolerance.

Problems: the edge graphs of tests/rounding_bounds.py (hubs of ~3000 observations, cameras with one observation, one camera
without any: its entries of every term are exactly 0), NONE and HUBER, default accumulator slots and POVAR_HOT_ACC=8 (most
cameras' sums then come through records of their own chunks)."""
import numpy as np
import pytest

import rounding_bounds as RB

pytestmark = pytest.mark.gpu
ALPHA, LAM, TERMS = 0.01, 1e-4, 20
_ENV = {"POVAR_E0_V1": "0", "POVAR_LPL_PLACE": "sync", "POVAR_DETERMINISTIC": "1"}
_LAYOUT_OVERRIDES = ("POVAR_CKH_ACC_CAP", "POVAR_CKH_STRIDE", "POVAR_HOT_ACC", "POVAR_CK_NB", "POVAR_CK_HMAX", "POVAR_LPL_K0", "POVAR_LPL_STRATEGY",
                     "POVAR_E0_WGS", "POVAR_E0_CK", "POVAR_NO_FUSE", "POVAR_RES")
_PROBLEMS = {}


def _problem(step):
    """(n_cams, lm_off, cam_idx, obs, cams, landmarks or None); the last camera has no observation"""
    if step not in _PROBLEMS:
        if step == 1:
            n_c, lm_off, cam_idx, obs, cams, _ = RB.edge_problem(0)
            _PROBLEMS[step] = (n_c + 1, lm_off, cam_idx, obs, np.concatenate([cams, cams[:1] + 0.5], 0), None)
        else:
            _PROBLEMS[step] = RB.edge_problem_joint(0)
    return _PROBLEMS[step]


def _tail(monkeypatch, step, robust, hot_acc, no_fuse):
    """x_0 and the 20 terms, the increment, and (iterations, status) of the series with q_tol = 0.05, through one tail"""
    from povar_amd import capi
    n_c, lm_off, cam_idx, obs, cams, lms_h = _problem(step)
    for k in _LAYOUT_OVERRIDES:
        monkeypatch.delenv(k, raising=False)
    for k, v in _ENV.items():
        monkeypatch.setenv(k, v)
    if hot_acc:
        monkeypatch.setenv("POVAR_HOT_ACC", hot_acc)
    if no_fuse:
        monkeypatch.setenv("POVAR_NO_FUSE", "1")
    ctx = capi.Context(n_c, lm_off, cam_idx, obs, robust_norm=robust, huber=RB.EDGE_HUBER if step == 1 else RB.EDGE_HUBER_H,
                       e0_mode=capi.E0_IMPLICIT_LDSACC)
    ctx.layout_finalize(True)
    ctx.set_cameras(cams)
    dim = 12 if step == 1 else 11
    if step == 1:
        ctx.init_landmarks_pose(ALPHA)
        assert ctx.linearize_pose(ALPHA)
        ctx.prepare_pose(LAM)
    else:
        ctx.set_landmarks_homogeneous(lms_h)
        assert ctx.linearize_homogeneous()
        ctx.prepare_joint(LAM)
    ctx.power_series_begin()
    terms = [ctx.get_term(dim)]
    for _ in range(TERMS):
        ctx.power_series_step()
        terms.append(ctx.get_term(dim))
    inc = ctx.get_increment(dim)
    li = ctx.layout_info()
    assert li.lane_per_landmark == 1
    assert (li.e0_kernel == 7) if step == 1 else (li.e0_kernel_h == 2), (li.e0_kernel, li.e0_kernel_h)
    if step == 1:
        _, it, status, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, TERMS, 0.05, -1.0)
    else:
        _, it, status, rc = ctx.solve_joint(LAM, TERMS, 0.05, -1.0)
    assert rc == 0
    ctx.close()
    return np.array(terms), inc, (it, status)


@pytest.mark.parametrize("hot_acc", [None, "8"], ids=["slots=default", "POVAR_HOT_ACC=8"])
@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
@pytest.mark.parametrize("step", [1, 2])
def test_fused_and_two_kernel_tail_leave_the_same_bits(monkeypatch, step, robust, hot_acc):
    n_c = _problem(step)[0]
    dim = 12 if step == 1 else 11
    t_f, inc_f, exit_f = _tail(monkeypatch, step, robust, hot_acc, False)
    t_n, inc_n, exit_n = _tail(monkeypatch, step, robust, hot_acc, True)
    rel = [float(np.linalg.norm(a - b) / np.linalg.norm(a)) for a, b in zip(t_f, t_n)]
    print(f"CAMSTEP step={step} {robust} hot_acc={hot_acc or 'default'}: worst term |fused - two-kernel| / |fused| = {max(rel):.3g}, "
          f"increment {float(np.linalg.norm(inc_f - inc_n) / np.linalg.norm(inc_f)):.3g}, early exit fused {exit_f} two-kernel {exit_n}")
    assert np.all(np.isfinite(t_f)) and np.all(np.isfinite(inc_f)) and np.linalg.norm(t_f[-1]) > 0
    for t in (t_f, t_n):
        assert np.all(t[:, dim * (n_c - 1):] == 0.0), "the camera without observations"
    assert np.array_equal(inc_f, inc_n)
    assert np.array_equal(t_f[-1], t_n[-1])
    assert np.array_equal(t_f, t_n)
    assert exit_f == exit_n
