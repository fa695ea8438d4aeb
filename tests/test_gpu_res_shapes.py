"""series_res and series_res_h through more of their instantiations (povar_kernels_res.hpp: one body res_series, 16 + 12
instantiations; the other modules reach the few that the library's own workgroup count gives).  POVAR_RES_WGS steers the
shape: on ladybug-49 (31 843 observations) the layout builder cuts

    POVAR_RES_WGS   step 1 <NW, H, RR, LS>   step 2 <NW, H, RR, LS>
    32              <16, 1, 1, 1>            <8, 1, 2, 1>
    30                                       <8, 2, 2, 1>
    16              <16, 2, 1, 1>            <8, 2, 2, 2>
    8               <8, 4, 2, 2>             <8, 4, 2, 2>  (step 1's instance, shared)

(below 8 workgroups no layout fits; step 1's other 512-thread shapes need cameras that overflow the 1024-thread shape's LDS:
the venice shards of test_gpu_res.py).  Every case asserts the shape it meant to reach -- a device with fewer CUs than the
value fails it, it does not test another kernel -- and then holds the resident series to the per-term kernels of the same
context as test_gpu_res.py and test_gpu_res_joint.py do: 20-term increment 1e-10 (relative 2-norm), the same iteration
count and status with q_tolerance = 0.05, no give-up.  State of the two steps as in those modules.
"""
import numpy as np
import pytest

from conftest import rel

pytestmark = pytest.mark.gpu
ALPHA, LAM, M = 0.01, 1e-4, 20
NAME = "ladybug-49"
_STATE = {}


def _state():
    """The problem, and step 2's state of test_gpu_res_joint.py (rng 11, normalised cameras, X_w = 1, obs / 500); built once."""
    from povar_amd import synth
    if not _STATE:
        p = synth.make_bal_problem(NAME)
        rng = np.random.default_rng(11)
        cams = rng.normal(size=(p.n_cams, 12))
        cams[:, 8:11] *= 0.1
        cams[:, 11] = 5 + rng.random(p.n_cams)
        cams /= np.linalg.norm(cams, axis=1, keepdims=True)
        lms_h = np.concatenate([rng.normal(size=(p.n_lms, 3)), np.ones((p.n_lms, 1))], 1)
        _STATE["p"], _STATE["joint"] = p, (cams, lms_h, p.obs / 500.0)
    return _STATE["p"], _STATE["joint"]


def _context(step, robust):
    """A linearised context of the step and a solve(**kw) -> (increment, iterations, status, rc) on it."""
    from povar_amd import capi
    p, (cams, lms_h, obs_h) = _state()
    if step == 1:
        ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=robust, e0_mode=capi.E0_IMPLICIT_LDSACC)
        ctx.layout_finalize(True)
        ctx.set_cameras(p.cams)
        ctx.init_landmarks_pose(ALPHA)
        assert ctx.linearize_pose(ALPHA)
        return ctx, lambda **kw: ctx.solve_pose(LAM, capi.POWER_VARPROJ, **kw)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs_h, robust_norm=robust, huber=1.0, e0_mode=capi.E0_IMPLICIT_LDSACC)
    ctx.layout_finalize(True)
    ctx.set_cameras(cams)
    ctx.set_landmarks_homogeneous(lms_h)
    assert ctx.linearize_homogeneous()
    return ctx, lambda **kw: ctx.solve_joint(LAM, **kw)


@pytest.mark.parametrize("step, wgs, shape", [(1, 32, (16, 1, 1)), (1, 16, (16, 2, 1)), (1, 8, (8, 4, 2)),
                                              (2, 32, (8, 1, 2)), (2, 30, (8, 2, 2)), (2, 16, (8, 2, 2)), (2, 8, (8, 4, 2))])
def test_resident_series_shape_against_the_per_term_kernels(monkeypatch, step, wgs, shape):
    """shape = (wavefronts per workgroup, rows per chunk, chunks per lane) of the instantiation the case is for."""
    for name in ("POVAR_RES", "POVAR_RES_MAX_OBS", "POVAR_RES_OBS_PER_WG", "POVAR_RES_SPIN", "POVAR_DETERMINISTIC"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("POVAR_RES_WGS", str(wgs))  # (read when the context is created)
    for robust in ("NONE", "HUBER"):
        ctx, solve = _context(step, robust)
        li = ctx.layout_info()
        if step == 1:
            ready, n_wg, got = li.res_ready, li.res_wgs, (li.res_waves, li.res_rows, li.res_rounds)
        else:
            ready, n_wg, got = li.res_ready_h, li.res_wgs_h, (li.res_waves_h, li.res_rows_h, li.res_rounds_h)
        print(f"RESSHAPE step={step} {robust} POVAR_RES_WGS={wgs}: ready={ready} wgs={n_wg} <NW, H, RR>={got} "
              f"lds={li.res_lds_bytes if step == 1 else li.res_lds_bytes_h} shared_h={li.res_shared_h}")
        assert ready == 1 and 1 <= n_wg <= wgs and got == shape, (ready, n_wg, got, shape)
        ctx.set_series_kernel(0)
        inc0, it0, st0, rc0 = solve(m=M)
        inc0q, it0q, st0q, rc0q = solve(m=M, q_tol=0.05, r_tol=-1.0)
        ctx.set_series_kernel(1)
        li = ctx.layout_info()
        assert (li.res_active if step == 1 else li.res_active_h) == 1
        inc, it, st, rc = solve(m=M)
        incq, itq, stq, rcq = solve(m=M, q_tol=0.05, r_tol=-1.0)
        print(f"RESSHAPE step={step} {robust} POVAR_RES_WGS={wgs}: rel={rel(inc, inc0):.3g} early exit: rel={rel(incq, inc0q):.3g} "
              f"iterations={itq} ({it0q}) status={stq} ({st0q})")
        assert rc == rc0 == 0 and (it, st) == (it0, st0) and rel(inc, inc0) < 1e-10
        assert rcq == rc0q == 0 and (itq, stq) == (it0q, st0q) and rel(incq, inc0q) < 1e-10
        assert ctx.layout_info().res_failed == 0
        ctx.close()
