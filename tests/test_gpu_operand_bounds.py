"""Every number an LM iteration hands to the power series held, entry by entry, to the long-double references and bounds of
tests/operand_bounds.py: the weights (through everything they enter), BUF_DIAG2, BUF_POSE_SCALING, the Jl column scale,
BUF_HLL_INV, the camera reflectors, b and B^-1 of both steps, for every kernel family that computes them.  The references
are built from what the caller set (graph, image points, cameras, landmarks, alpha, lambda, robust norm, eps, solver type),
not from the context's own buffers; only B^-1's right-residual check takes the device's sigma (checked before it) as exact.
The normwise tests of the other modules see these operands as relative 2-norms over all cameras or landmarks, which a
one-observation camera or a two-view landmark cannot move.

Families (each case forces its own with monkeypatch.setenv and asserts through layout_info() that it ran; under
POVAR_DETERMINISTIC=1 in the environment -- tools/forced_mode_suite.sh -- the cases of the other families skip):
  per_obs  lm_regular / lm_long<OpLinearize[H] / OpPrepare[H]>, cm_scatter, cam_sum_items[_h]          POVAR_E0_V1=1
  lpl      lpl_pass[_h]<0>, prepare_lpl[_h], cm_gram[_h] in gather mode, cam_cold_sum, cam_nt_project   POVAR_E0_V1=0
  det      the bit-reproducible mode: it pins the E0 mode to E0_IMPLICIT (povar_create.hip), so linearize / prepare take the
           per-observation kernels while the lane-per-landmark layout of its term kernels is in place   POVAR_DETERMINISTIC=1
all of them through cam_finish_linearize[_h] and cam_build_binv[_h].  Shapes: the edge graph of rounding_bounds.py with
one unobserved camera (151 cameras, 4 149 landmarks, 14 792 observations: hubs over several items and workgroups, 56
cameras with one or two observations, landmarks longer than a wavefront, near-parallel two-view landmarks) and
small_problem's size once per step (6 cameras: the tail workgroup of cam_build_binv).
"""
import os

import numpy as np
import pytest

import operand_bounds as OB
import rounding_bounds as RB

pytestmark = pytest.mark.gpu
ALPHA, LAM = 0.01, 1e-4
DET_ENV = os.environ.get("POVAR_DETERMINISTIC") == "1"
CK_VARIANTS = 6
_OVERRIDES = ("POVAR_E0_CK", "POVAR_PREPARE_V1", "POVAR_HOT_ACC", "POVAR_CK_NB", "POVAR_CK_HMAX", "POVAR_LPL_K0",
              "POVAR_LPL_STRATEGY", "POVAR_E0_WGS", "POVAR_RES")

# family: (environment, e0 mode, lane_per_landmark expected)
FAMILIES = {
    "per_obs": ({"POVAR_E0_V1": "1"}, "E0_IMPLICIT", 0),
    "lpl": ({"POVAR_E0_V1": "0", "POVAR_LPL_PLACE": "sync"}, "E0_IMPLICIT_LDSACC", 1),
    "det": ({"POVAR_DETERMINISTIC": "1", "POVAR_E0_V1": "0", "POVAR_LPL_PLACE": "sync"}, "E0_IMPLICIT_LDSACC", 1),
}


def _create(monkeypatch, fam, p, more_env=None):
    from povar_amd import capi
    env, mode, _ = FAMILIES[fam]
    env = {**env, **(more_env or {})}
    if DET_ENV and fam != "det":
        pytest.skip("POVAR_DETERMINISTIC=1 in the environment pins the kernels of this case")
    for k in _OVERRIDES:
        monkeypatch.delenv(k, raising=False)
    if fam != "det":
        monkeypatch.delenv("POVAR_DETERMINISTIC", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=p.robust, huber=p.huber, eps=p.eps, e0_mode=getattr(capi, mode))
    ctx.layout_finalize(True)
    return ctx


def _ran(ctx, fam, joint):
    li = ctx.layout_info()
    assert li.lane_per_landmark == FAMILIES[fam][2], (fam, li.lane_per_landmark)
    if fam == "det":
        if joint:  # (the step-2 term kernel is decided at the first term)
            ctx.power_series_begin()
            ctx.power_series_step()
            assert ctx.layout_info().e0_kernel_h == 2, ctx.layout_info().e0_kernel_h
        else:
            assert li.e0_kernel == CK_VARIANTS + 1, li.e0_kernel


def _assert_all(ctx, p, R, names, joint):
    """Every entry of every operand within its bound; on failure the operand, the worst entry's camera or landmark, its
    observation count and err / bound.  Returns {operand: worst err / bound}."""
    from povar_amd import capi
    out, bad = {}, []
    for name, per, cnt in names:
        dev = ctx.get_buffer(getattr(capi, "BUF_" + name))
        assert np.all(np.isfinite(dev)), name
        r, over, line = OB.report(name, per, dev, R.ref[name], R.bound[name], cnt)
        out[name] = r
        if over:
            bad.append(line)
    bname, n = ("B_INV_JOINT", 11) if joint else ("B_INV", 12)
    X = ctx.get_buffer(getattr(capi, "BUF_" + bname)).reshape(-1, n, n)
    assert np.all(np.isfinite(X))
    res, Rb, asym, ab = OB.binv_check(R, bname, p, X)
    for what, a, b in ((bname + " residual", res, Rb), (bname + " symmetry", asym, ab)):
        r, over, line = OB.report(what, n * n, a, np.zeros_like(a), b, p.n_c)
        out[what] = r
        if over:
            bad.append(line)
    # the cameras without observations: exact zeros, sigma = 1 / eps, B^-1 = I / lambda
    for c in np.flatnonzero(p.n_c == 0):
        d2 = ctx.get_buffer(capi.BUF_DIAG2).reshape(-1, 12)[c]
        b = ctx.get_buffer(capi.BUF_B_JOINT if joint else capi.BUF_B).reshape(p.n_cams, -1)[c]
        if not (np.all(d2 == 0.0) and np.all(b == 0.0)):
            bad.append(f"camera {c} without observations: diag2 {d2}, b {b}")
        off = X[c] - np.diag(np.diag(X[c]))
        if not (np.all(off == 0.0) and np.all(np.abs(np.diag(X[c]) * p.lam - 1) <= OB.g(3))):
            bad.append(f"camera {c} without observations: B^-1 is not I / lambda to gamma_3")
    if joint:
        v, vb = OB.nc_nullspace(R, p, ctx.get_buffer(capi.BUF_NC_HOUSEHOLDER))
        r, over, line = OB.report("N_c^T vec(P_c)", 11, v, np.zeros_like(v), vb, p.n_c)
        out["N_c^T vec(P_c)"] = r
        if over:
            bad.append(line)
    assert not bad, "\n".join(bad)
    return out


POSE_NAMES = lambda p: [("DIAG2", 12, p.n_c), ("POSE_SCALING", 12, p.n_c), ("JL_COL_SCALE", 3, p.n_l), ("HLL_INV", 9, p.n_l), ("B", 12, p.n_c)]
JOINT_NAMES = lambda p: [("DIAG2", 12, p.n_c), ("POSE_SCALING", 12, p.n_c), ("JL_COL_SCALE_H", 4, p.n_l), ("HLL_INV", 9, p.n_l),
                         ("NC_HOUSEHOLDER", 13, p.n_c), ("B_JOINT", 11, p.n_c)]


def _reference(p, ctx, joint, mutate):
    from povar_amd import capi
    R = (OB.joint_operands if joint else OB.pose_operands)(p, sigma_dev=ctx.get_buffer(capi.BUF_POSE_SCALING), mutate=mutate)
    R.ref["POSE_SCALING"], R.bound["POSE_SCALING"] = R.ref["SIGMA"], R.bound["SIGMA"]
    return R


def check_pose(ctx, p, fam, label, mutate=None):
    """linearize_pose + prepare_pose at the context's current point (= p's cameras and landmarks), then every operand.
    mutate: perturbs the reference side (operand_bounds.pose_operands); the hand-run mutation check passes it."""
    from povar_amd import capi
    ctx.set_jl_col_scaling(p.scale_jl)
    assert ctx.linearize_pose(p.alpha)
    ctx.prepare_pose(p.lam, getattr(capi, p.solver))
    _ran(ctx, fam, False)
    out = _assert_all(ctx, p, _reference(p, ctx, False, mutate), POSE_NAMES(p), False)
    if not p.scale_jl:
        assert np.all(ctx.get_buffer(capi.BUF_JL_COL_SCALE) == 1.0)
    print(f"OPBOUND {label} {fam} " + " ".join(f"{k.replace(' ', '_')}={v:.3g}" for k, v in out.items()))
    return out


def check_joint(ctx, p, fam, label, mutate=None):
    assert ctx.linearize_homogeneous()
    ctx.prepare_joint(p.lam)
    out = _assert_all(ctx, p, _reference(p, ctx, True, mutate), JOINT_NAMES(p), True)
    _ran(ctx, fam, True)
    print(f"OPBOUND {label} {fam} " + " ".join(f"{k.replace(' ', '_')}={v:.3g}" for k, v in out.items()))
    return out


# ---- the edge graph plus one camera without observations
def edge_pose(robust, **kw):
    n_c, lm_off, cam_idx, obs, cams, lms = RB.edge_problem(0)
    cams = np.concatenate([cams, cams[:1] + 0.5], 0)
    return OB.Pose(n_c + 1, lm_off, cam_idx, obs, cams, lms, ALPHA, LAM, robust, RB.EDGE_HUBER, **kw)


def edge_joint(robust):
    n_c, lm_off, cam_idx, obs, cams, X = RB.edge_problem_joint(0)
    return OB.Joint(n_c, lm_off, cam_idx, obs, cams, X, RB.EDGE_LAM_H, robust, RB.EDGE_HUBER_H)


def pose_context(monkeypatch, fam, p, env=None):
    ctx = _create(monkeypatch, fam, p, env)
    ctx.set_cameras(p.cams)
    ctx.set_landmarks(p.lms)
    return ctx


def joint_context(monkeypatch, fam, p, env=None):
    ctx = _create(monkeypatch, fam, p, env)
    ctx.set_cameras(p.cams)
    ctx.set_landmarks_homogeneous(p.lms)
    return ctx


# every family at its defaults, then the lpl family on the layouts that stress the row stream of lpl_pass[_h]<0> and
# prepare_lpl[_h] (povar_kernels_lpl.hpp): one workgroup of shortest tiles (at least 65 tiles over 16 wavefronts: later tiles
# from the counter, the prefetch cursor across tile boundaries and into "no tile left"), and 8 accumulators (mostly cold
# observations).  Set after _create's deletions.
LPL_STREAM_ENVS = ({"POVAR_E0_WGS": "1", "POVAR_LPL_K0": "2"}, {"POVAR_HOT_ACC": "8"})
EDGE_CASES = [(f, r, {}) for r in ("NONE", "HUBER") for f in FAMILIES] + [("lpl", r, e) for e in LPL_STREAM_ENVS for r in ("NONE", "HUBER")]
EDGE_IDS = ["-".join([f, r] + [f"{k}={v}" for k, v in e.items()]) for f, r, e in EDGE_CASES]


@pytest.mark.parametrize("fam,robust,env", EDGE_CASES, ids=EDGE_IDS)
def test_step1_operands_on_the_edge_graph(monkeypatch, fam, robust, env):
    p = edge_pose(robust)
    assert p.n_cams == 151 and p.n_lms == 4149 and len(p.cam_idx) == 14792 and (p.n_c == 0).sum() == 1
    ctx = pose_context(monkeypatch, fam, p, env)
    if "POVAR_E0_WGS" in env:
        assert ctx.layout_info().grid == 1
    check_pose(ctx, p, fam, f"edge/{robust}" + "".join(f"/{k}={v}" for k, v in env.items()))
    ctx.close()


@pytest.mark.parametrize("fam,robust,env", EDGE_CASES, ids=EDGE_IDS)
def test_step2_operands_on_the_edge_graph(monkeypatch, fam, robust, env):
    p = edge_joint(robust)
    assert p.n_cams == 151 and (p.n_c == 0).sum() == 1
    ctx = joint_context(monkeypatch, fam, p, env)
    if "POVAR_E0_WGS" in env:
        assert ctx.layout_info().grid == 1
    check_joint(ctx, p, fam, f"edge-joint/{robust}" + "".join(f"/{k}={v}" for k, v in env.items()))
    ctx.close()


@pytest.mark.parametrize("what", ["POWER_SCHUR_COMPLEMENT", "unscaled_jl"])
def test_step1_operands_solver_type_and_unscaled_jl(monkeypatch, what):
    """lambda on the landmark blocks; set_jl_col_scaling(False): every Jl scale exactly 1.0 and Hll^-1 of the unscaled rows."""
    p = edge_pose("NONE", solver="POWER_SCHUR_COMPLEMENT") if what == "POWER_SCHUR_COMPLEMENT" else edge_pose("HUBER", scale_jl=False)
    ctx = pose_context(monkeypatch, "lpl", p)
    check_pose(ctx, p, "lpl", f"edge/{what}")
    ctx.close()


def test_step1_operands_follow_the_second_linearisation_point(monkeypatch):
    """linearize + prepare, a solve, apply_pose, then linearize + prepare again: every operand is the one of the NEW point
    (a record left from the first point is what a relative 2-norm over all cameras cannot see)."""
    from povar_amd import capi
    p = edge_pose("HUBER")
    ctx = pose_context(monkeypatch, "lpl", p)
    check_pose(ctx, p, "lpl", "edge/first-point")
    inc, _, _, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, 5)
    assert rc == 0 and np.all(np.isfinite(inc))
    ctx.apply_pose(capi.POWER_VARPROJ, ALPHA, inc)
    cams, lms = ctx.get_cameras().reshape(-1, 12), ctx.get_landmarks().reshape(-1, 3)
    moved = np.abs(cams - p.cams).max(1) > 0
    assert moved[p.n_c > 0].all() and (np.abs(lms - p.lms).max(1) > 0).all()
    p2 = OB.Pose(p.n_cams, p.lm_off, p.cam_idx, p.obs, cams, lms, ALPHA, LAM, "HUBER", RB.EDGE_HUBER)
    check_pose(ctx, p2, "lpl", "edge/second-point")
    ctx.close()


# ---- six cameras: the tail workgroup of cam_build_binv[_h] (four cameras per workgroup)
def test_step1_operands_small(monkeypatch, small_problem):
    s = small_problem
    rng = np.random.default_rng(21)
    p = OB.Pose(s.n_cams, s.lm_off, s.cam_idx, s.obs, s.cams, s.lms + 0.0, ALPHA, LAM)
    ctx = _create(monkeypatch, "lpl", p)
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(ALPHA)
    p.lms = ctx.get_landmarks().reshape(-1, 3) + 1e-3 * rng.normal(size=(s.n_lms, 3))
    ctx.set_landmarks(p.lms)
    assert p.n_cams % 4 != 0
    check_pose(ctx, p, "lpl", "small")
    ctx.close()


def test_step2_operands_small(monkeypatch, small_problem):
    s = small_problem
    rng = np.random.default_rng(11)
    cams = rng.normal(size=(s.n_cams, 12))
    cams[:, 8:11] *= 0.1
    cams[:, 11] = 5 + rng.random(s.n_cams)
    cams /= np.linalg.norm(cams, axis=1, keepdims=True)
    lms_h = np.concatenate([rng.normal(size=(s.n_lms, 3)), np.ones((s.n_lms, 1))], 1)
    p = OB.Joint(s.n_cams, s.lm_off, s.cam_idx, s.obs / 500.0, cams, lms_h, LAM, "HUBER", 0.5)
    ctx = joint_context(monkeypatch, "lpl", p)
    assert p.n_cams % 4 != 0
    check_joint(ctx, p, "lpl", "small-joint")
    ctx.close()
