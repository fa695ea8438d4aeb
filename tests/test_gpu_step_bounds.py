"""The two ends of an LM iteration held, entry by entry, to the long-double references and bounds of tests/step_bounds.py:
the cost fields of error_pose / error_homogeneous, and after apply_pose (both solver types) / apply_joint / normalize_joint
every camera entry, every landmark coordinate and l_diff, for every kernel family that computes them.  The references are
built from what the caller set (graph, image points, cameras, landmarks, alpha, lambda, robust norm, eps, solver type, Jl
scaling, the increment), never from the context's buffers; the cost after an apply is referred to the state read back with
get_cameras / get_landmarks[_homogeneous], which holds the lane-ordered landmark mirror that backsub_lpl[_h] writes and the
landmark-order master to the same numbers.  The normwise tests of the other modules see the cost as one relative scalar and
the new landmarks as a relative 2-norm that the near-parallel two-view landmarks carry.

Families (tests/test_gpu_operand_bounds.py: each case forces its own and asserts through layout_info() that it ran; under
POVAR_DETERMINISTIC=1 in the environment the cases of the other families skip):
  per_obs  lm_regular / lm_long<OpError[H]> and <OpBackVarproj / OpBackPoba / OpBackJoint>
  lpl      lpl_pass[_h]<1>, backsub_lpl[_h]; POWER_SCHUR_COMPLEMENT back-substitutes through ensure_legacy's rebuild of the
           per-slot sqrt(w), weighted residual, Jl scale and linearisation-point landmarks after lpl_pass<0>
  det      linearises on the lane-per-landmark layout and back-substitutes through ensure_legacy
all of them through cam_apply_inc[_h].  Shapes: the edge graph (151 cameras, 4 149 landmarks, 14 792 observations) and
small_problem's once per step.  The increment is a seeded vector (step_bounds.seeded_increment), in one case per step the
device's own 20-term one.

Measured on an MI355X when these tests were written (largest err / bound per quantity; every figure is printed as
"STEPBOUND ..." before it is asserted; NONE | HUBER; "cost" is the larger of all_error / valid_error, "|r|" of the residual
sums, "new" the same two at the point the apply left behind):
  step 1, POWER_VARPROJ      cameras  landmarks      l_diff             cost               |r|      new cost           new |r|
    per_obs, det (alike)     0.97     0.12 | 0.084   0.031 | 0.0079     8.5e-5 | 4.2e-5    4.8e-6   1.3e-4 | 3.8e-5    3.0e-5 | 7.3e-5
    lpl                      0.97     0.12 | 0.084   0.015 | 4.4e-4     3.4e-5 | 6.0e-5    8.4e-5   4.0e-6 | 7.7e-5    2.7e-5 | 7.9e-5
    lpl, one workgroup       0.97     0.12 | 0.084   0.011 | 1.9e-4     1.5e-4 | 4.2e-5    9.4e-5   4.1e-6 | 1.5e-4    2.6e-5 | 3.0e-5
    lpl, 8 accumulators      0.97     0.12 | 0.084   0.015 | 1.1e-3     3.4e-5 | 6.0e-5    8.4e-5   4.1e-6 | 7.1e-6    5.9e-5 | 9.9e-6
    lpl, Jl scaling off      0.97     0.12 | 0.084   1.3e-4 | 4.7e-4    as lpl
    lpl, 20-term inc, HUBER  0.85     0.063          1.1e-5                                          5.3e-5             7.9e-5
    lpl, sequence, HUBER     0.99     0.13           3.6e-3 (half increment after restore_pose; the restored state bit for bit)
    small (lpl, HUBER)       0.92     0.043          1.4e-4             4.7e-3             1.5e-3   6.7e-3             2.3e-3
  step 1, POWER_SCHUR_COMPLEMENT (lpl: OpBackPoba after ensure_legacy's rebuild)
                             0.97     0.070 | 0.057  3.8e-5 | 2.4e-5    as lpl                      7.1e-5 | 7.2e-5    4.5e-5 | 5.7e-5
  step 2                     cameras         landmarks        l_diff             cost               |r|      new cost           new |r|
    per_obs, det (alike)     0.93 | 0.92     0.080 | 0.071    2.9e-5 | 5.6e-5    4.9e-6 | 3.7e-4    8.7e-4   1.0e-3 | 1.2e-4    1.0e-4 | 7.4e-5
    lpl                      0.93 | 0.92     0.080 | 0.071    7.0e-6 | 4.8e-5    4.9e-6 | 4.8e-4    8.7e-4   2.3e-3 | 2.7e-4    7.5e-5 | 3.6e-4
    lpl, one workgroup       0.93 | 0.92     0.080 | 0.071    7.0e-6 | 5.6e-5    8.7e-5 | 2.6e-4    8.7e-4   1.7e-3 | 1.5e-5    5.5e-4 | 1.9e-4
    lpl, 8 accumulators      0.93 | 0.92     0.080 | 0.071    7.0e-6 | 5.1e-5    4.9e-6 | 4.8e-4    6.9e-4   2.2e-3 | 1.9e-5    1.8e-4 | 5.5e-6
    lpl, 20-term inc, HUBER  0.78            0.049            4.5e-5                                          2.7e-4             3.4e-4
    lpl, sequence, HUBER     normalize_joint: cameras 0.26, landmarks 0.99 (one division against one rounding), X_w exactly 1;
                             the cost at the normalised point 1.6e-4, |r| 4.5e-4
    small (lpl, HUBER)       0.85            0.0017           1.8e-4             8.0e-3             9.2e-3   3.9e-3             3.9e-3
  CAUCHY, cost only          step 1: 4.1e-5 (per_obs and lpl), |r| 4.8e-6 | 8.4e-5     step 2: 3.8e-5, |r| 8.7e-4
  the camera without observations: 0.30 of its gamma_3 bound in step 1, 0.022 in step 2 (the reflector's dNc is in the bound)
Every family computes the same landmarks to the printed digits: the update is decided by the rows, not by the order of a
landmark's sum.  The cameras' ratio near 1 is two roundings against a two-rounding bound over 1 800 entries.  The cost's
ratios are small because gamma_{n_obs} of a sum in any tree carries its bound (tests/test_step_bounds.py says what the
cost's bound is good for); l_diff's are small where gamma_{4 n_obs} carries half of the bound.  No case exposed a defect:
the library is unchanged.
"""
import numpy as np
import pytest

import operand_bounds as OB
import step_bounds as SB
import test_gpu_operand_bounds as G

pytestmark = pytest.mark.gpu
ALPHA, LAM = G.ALPHA, G.LAM
_REF = {}


def _key(p, inc):
    return (type(p).__name__, p.robust, p.solver, p.scale_jl, p.huber, p.lam, p.alpha, hash(p.cams.tobytes()), hash(p.lms.tobytes()),
            hash(p.obs.tobytes()), hash(np.ascontiguousarray(inc, dtype=np.float64).tobytes()))


def _reference(p, inc):
    """The applied-step reference of (p, inc), computed once per problem and increment and left unchanged."""
    k = _key(p, inc)
    if k not in _REF:
        _REF[k] = SB.applied(p, inc)
    return _REF[k]


def _line(label, fam, what, figs):
    print(f"STEPBOUND {label} {fam} {what} " + " ".join(f"{k}={v:.3g}" for k, v in figs))


def check_cost(ctx, p, fam, label, what):
    """The cost fields at the context's current point (= p's cameras and landmarks); the counts exactly."""
    joint = isinstance(p, OB.Joint)
    ri = ctx.error_homogeneous() if joint else ctx.error_pose(p.alpha)
    assert ri.is_numerically_valid
    res = SB.cost_check(SB.cost(p), ri, 2 if joint else 1)
    _line(label, fam, "cost/" + what, [(k, r) for k, r, _ in res])
    bad = [f"{what}: {k} err/bound={r:.3g}" for k, r, over in res if over]
    assert not bad, "\n".join(bad)


def _state(ctx, joint):
    return ctx.get_cameras().reshape(-1, 12), (ctx.get_landmarks_homogeneous() if joint else ctx.get_landmarks())


def check_applied(ctx, p, fam, label, what, inc, l_diff):
    """Every camera entry, every landmark coordinate and l_diff after an apply of inc at p's state; the cameras without
    observations moved by sigma * inc with sigma = 1 / eps to gamma_3; then the cost at the state read back."""
    joint = isinstance(p, OB.Joint)
    R = _reference(p, inc)
    cams, lms = _state(ctx, joint)
    assert np.all(np.isfinite(cams)) and np.all(np.isfinite(lms)) and np.isfinite(l_diff)
    res = SB.apply_check(p, R, cams, lms, l_diff)
    _line(label, fam, "apply/" + what, [(n, r) for n, r, _, _ in res])
    bad = [line for _, _, over, line in res if over]
    err, bound, c0 = SB.unobserved_moved(p, R, cams, SB.ambient_increment(p, inc))
    if len(c0):
        _line(label, fam, "unobserved/" + what, [("cameras", float((err / bound).max()))])
        bad += [f"camera {c} without observations did not move by inc / eps" for c, e, b in zip(c0, err, bound) if not (e <= b).all()]
    assert not bad, "\n".join(bad)
    q = SB._with(p, cams=cams, lms=lms)
    check_cost(ctx, q, fam, label, what + "/new-point")
    return q


def _linearize(ctx, p, fam):
    from povar_amd import capi
    joint = isinstance(p, OB.Joint)
    if joint:
        assert ctx.linearize_homogeneous()
        ctx.prepare_joint(p.lam)
    else:
        ctx.set_jl_col_scaling(p.scale_jl)
        assert ctx.linearize_pose(p.alpha)
        ctx.prepare_pose(p.lam, getattr(capi, p.solver))
    G._ran(ctx, fam, joint)


def _apply(ctx, p, inc):
    from povar_amd import capi
    return ctx.apply_joint(inc) if isinstance(p, OB.Joint) else ctx.apply_pose(getattr(capi, p.solver), p.alpha, inc)


def run_case(monkeypatch, fam, p, env, label, device_inc=False):
    """cost at the start, linearize + prepare, apply, every number of the new state, the cost there."""
    from povar_amd import capi
    joint = isinstance(p, OB.Joint)
    ctx = (G.joint_context if joint else G.pose_context)(monkeypatch, fam, p, env)
    if "POVAR_E0_WGS" in env:
        assert ctx.layout_info().grid == 1
    check_cost(ctx, p, fam, label, "start")
    _linearize(ctx, p, fam)
    if device_inc:
        inc, it, _, rc = ctx.solve_joint(p.lam, 20) if joint else ctx.solve_pose(p.lam, getattr(capi, p.solver), 20)
        assert rc == 0 and it == 20 and np.all(np.isfinite(inc))
    else:
        inc = SB.seeded_increment(p)
    check_applied(ctx, p, fam, label, "seeded" if not device_inc else "20-term", inc, _apply(ctx, p, inc))
    ctx.close()


def _label(prefix, robust, env):
    return f"{prefix}/{robust}" + "".join(f"/{k}={v}" for k, v in env.items())


@pytest.mark.parametrize("fam,robust,env", G.EDGE_CASES, ids=G.EDGE_IDS)
def test_step1_cost_and_applied_step_on_the_edge_graph(monkeypatch, fam, robust, env):
    p = G.edge_pose(robust)
    assert p.n_cams == 151 and p.n_lms == 4149 and len(p.cam_idx) == 14792 and (p.n_c == 0).sum() == 1
    run_case(monkeypatch, fam, p, env, _label("edge", robust, env))


@pytest.mark.parametrize("fam,robust,env", G.EDGE_CASES, ids=G.EDGE_IDS)
def test_step2_cost_and_applied_step_on_the_edge_graph(monkeypatch, fam, robust, env):
    p = G.edge_joint(robust)
    assert p.n_cams == 151 and (p.n_c == 0).sum() == 1
    run_case(monkeypatch, fam, p, env, _label("edge-joint", robust, env))


@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
@pytest.mark.parametrize("what", ["POWER_SCHUR_COMPLEMENT", "unscaled_jl"])
def test_step1_solver_type_and_unscaled_jl(monkeypatch, what, robust):
    """POWER_SCHUR_COMPLEMENT in the lpl family: OpBackPoba on what ensure_legacy rebuilds after lpl_pass<0>;
    set_jl_col_scaling(False): every Jl scale exactly 1."""
    p = G.edge_pose(robust, solver="POWER_SCHUR_COMPLEMENT") if what == "POWER_SCHUR_COMPLEMENT" else G.edge_pose(robust, scale_jl=False)
    run_case(monkeypatch, "lpl", p, {}, f"edge/{what}/{robust}")


@pytest.mark.parametrize("fam", ["per_obs", "lpl"])
@pytest.mark.parametrize("step", [1, 2])
def test_cost_with_the_cauchy_norm(monkeypatch, step, fam):
    p = G.edge_pose("CAUCHY") if step == 1 else G.edge_joint("CAUCHY")
    ctx = (G.pose_context if step == 1 else G.joint_context)(monkeypatch, fam, p)
    assert ctx.layout_info().lane_per_landmark == G.FAMILIES[fam][2]
    check_cost(ctx, p, fam, f"edge{'-joint' if step == 2 else ''}/CAUCHY", "start")
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_applied_step_with_the_devices_own_increment(monkeypatch, step):
    """The increment of a 20-term solve instead of the seeded one (the reference takes its bits as an input)."""
    p = G.edge_pose("HUBER") if step == 1 else G.edge_joint("HUBER")
    run_case(monkeypatch, "lpl", p, {}, f"edge{'-joint' if step == 2 else ''}/HUBER", device_inc=True)


def test_step1_sequence_backup_apply_restore_apply_error(monkeypatch):
    """backup -> apply(inc) -> restore -> apply(0.5 inc) -> error in the lpl family: restore_pose invalidates the lane mirror
    that the first backsub_lpl wrote; every stage within its bound, the restored state bit for bit."""
    p = G.edge_pose("HUBER")
    ctx = G.pose_context(monkeypatch, "lpl", p)
    _linearize(ctx, p, "lpl")
    inc = SB.seeded_increment(p)
    ctx.backup_pose()
    check_applied(ctx, p, "lpl", "edge/sequence", "apply", inc, _apply(ctx, p, inc))
    ctx.restore_pose()
    cams, lms = _state(ctx, False)
    assert np.array_equal(cams, p.cams) and np.array_equal(lms, p.lms)
    check_cost(ctx, p, "lpl", "edge/sequence", "restored")
    check_applied(ctx, p, "lpl", "edge/sequence", "apply-half", 0.5 * inc, _apply(ctx, p, 0.5 * inc))
    ctx.close()


def test_step2_sequence_apply_normalize_error(monkeypatch):
    """apply -> normalize_joint -> error_homogeneous in the lpl family: normalize_joint divides the lane mirror along with
    the landmark-order master; X_w exactly 1 afterwards."""
    p = G.edge_joint("HUBER")
    ctx = G.joint_context(monkeypatch, "lpl", p)
    _linearize(ctx, p, "lpl")
    inc = SB.seeded_increment(p)
    q = check_applied(ctx, p, "lpl", "edge-joint/sequence", "apply", inc, _apply(ctx, p, inc))
    ctx.normalize_joint()
    cams, lms = _state(ctx, True)
    RN = SB.normalize_joint(q.cams, q.lms)
    bad, figs = [], []
    for nm, dev, per, cnt in (("CAMERAS", cams, 12, p.n_c), ("LANDMARKS", lms, 4, p.n_l)):
        r, over, line = SB.report("normalize " + nm, per, dev.reshape(-1), RN.ref[nm], RN.bound[nm], cnt)
        figs.append((nm, r))
        if over:
            bad.append(line)
    _line("edge-joint/sequence", "lpl", "normalize", figs)
    assert not bad, "\n".join(bad)
    assert np.all(lms[:, 3] == 1.0)
    check_cost(ctx, SB._with(p, cams=cams, lms=lms), "lpl", "edge-joint/sequence", "normalized")
    ctx.close()


# ---- small_problem once per step (six cameras, no camera without observations)
def test_step1_small(monkeypatch, small_problem):
    s = small_problem
    rng = np.random.default_rng(21)
    p = OB.Pose(s.n_cams, s.lm_off, s.cam_idx, s.obs, s.cams, s.lms + 0.0, ALPHA, LAM, "HUBER", 1.0)
    ctx = G._create(monkeypatch, "lpl", p)
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(ALPHA)
    p.lms = ctx.get_landmarks().reshape(-1, 3) + 1e-3 * rng.normal(size=(s.n_lms, 3))
    ctx.set_landmarks(p.lms)
    check_cost(ctx, p, "lpl", "small", "start")
    _linearize(ctx, p, "lpl")
    inc = SB.seeded_increment(p)
    check_applied(ctx, p, "lpl", "small", "seeded", inc, _apply(ctx, p, inc))
    ctx.close()


def test_step2_small(monkeypatch, small_problem):
    s = small_problem
    rng = np.random.default_rng(11)
    cams = rng.normal(size=(s.n_cams, 12))
    cams[:, 8:11] *= 0.1
    cams[:, 11] = 5 + rng.random(s.n_cams)
    cams /= np.linalg.norm(cams, axis=1, keepdims=True)
    lms_h = np.concatenate([rng.normal(size=(s.n_lms, 3)), np.ones((s.n_lms, 1))], 1)
    p = OB.Joint(s.n_cams, s.lm_off, s.cam_idx, s.obs / 500.0, cams, lms_h, LAM, "HUBER", 0.5)
    run_case(monkeypatch, "lpl", p, {}, "small-joint")
