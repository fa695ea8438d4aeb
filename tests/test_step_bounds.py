"""The cost and applied-step bounds of tests/step_bounds.py checked on the CPU: the long-double references against exact rational
arithmetic (step-1 cost with the trivial norm, the POWER_VARPROJ re-solve) and against the CPU oracle (everything else, every
l_diff), fp64 NumPy emulations of the two summation orders within every bound, and the defects a relative 2-norm over all
landmarks or one relative scalar lets through, reported on exactly the entries they touch.

Measured when these tests were written (largest err / bound over every entry of the quantity; every figure is printed as
"STEPBOUND ..." before it is asserted):
  * the long-double reference against exact rationals on the tiny problem, in the long-double model's own bound: new cameras
    0.91 (two roundings against a two-rounding bound), re-solved landmarks 0.0081, the cost inside its bound;
  * the cost, edge graphs (NONE | HUBER | CAUCHY; the oracle sums in row order like the per-observation emulation):
      step 1   row order 1.5e-4 | 1.4e-3 | 1.3e-4   lane-per-landmark order 3.4e-5 | 6.0e-5 | 4.6e-5   |r| sum 1.7e-4, 4.8e-6
      step 2   row order 1.9e-3 | 3.4e-3 | 5.8e-4   lane-per-landmark order 4.9e-6 | 1.8e-4 | 3.9e-5   |r| sum 1.1e-3, 4.0e-4
    The bound is 1.7e-12 of the cost: gamma_{n_obs} of the sum in ANY tree is 1.6e-12 at 14 792 observations and carries it,
    while every summation order in use rounds like a short tree.  So the cost's bound is no tighter than the 1e-12 of the
    normwise tests; what it adds is a reference built from the inputs alone (the counts and the valid set exactly), the
    check of the cost at the point an apply left behind, and the per-observation errors E(e_i), which are 1e-15 of e_i;
  * the applied step, edge graphs plus one unobserved camera (NONE | HUBER), oracle and both emulated orders alike but l_diff:
      POWER_VARPROJ            cameras 0.97   landmarks 0.10 | 0.084    l_diff 0.031 | 0.017 (oracle), 0.012 (emulations)
      POWER_SCHUR_COMPLEMENT   cameras 0.97   landmarks 0.093 | 0.092   l_diff 1.0e-4 | 1.5e-4
      Jl scaling off           cameras 0.97   landmarks 0.10 | 0.084    l_diff 6.1e-5 | 5.8e-3
      step 2                   cameras 0.93 | 0.92   landmarks 0.080 | 0.071   l_diff 2.7e-4 | 3.4e-5
      normalize_joint          cameras 0.29   landmarks 0.99
    The camera update is two roundings and X / X_w one: the bound is those roundings (plus |inc| E(sigma)), and over 1 800
    entries one of them comes within a few per cent of it -- a ratio near 1 that is as tight as a bound gets, not a
    miscount.  The landmarks compound absolute-value maps the way Hll^-1 and b of operand_bounds do.  l_diff: half of the
    bound of POWER_SCHUR_COMPLEMENT and step 2 is gamma_{4 n_obs} (gamma_{2 n_obs}) of sum |term|, the rest the terms' own
    errors; its relative size is 2.6e-11 | 5.6e-11 (POWER_SCHUR_COMPLEMENT), 7.4e-12 | 1.5e-10 (step 2) and 1.6e-9 | 1.4e-9
    for POWER_VARPROJ, where ONE near-parallel two-view landmark (E(delta) / |delta| = 6e-4) carries 83 % of it: its stored
    rows of the linearisation point see the re-solved update's weak direction -- conditioning of the data;
  * the conditions, for the reference alone: inv3's E(det) / |det| at most 2.4e-7 at P_new (POWER_VARPROJ), 2.2e-8
    (POWER_SCHUR_COMPLEMENT), 5.0e-5 (step 2) against 2^-10 = 9.8e-4; the smallest ||z| - 1e-5| is 1.2e13 times err(z); every
    entry has a finite bound and is compared: the share of skipped entries is 0.  The same holds at half the increment and
    at a 20-term solve's increment (cameras move by up to 15);
  * mutations (the unmutated emulation as the device): each is reported on exactly the landmark (or the one coordinate) it
    touches, on no camera, and l_diff / the cost exactly when it is touched.  At full size none of them hides from the
    normwise tolerances either on this graph (landmarks < 1e-9 | 1e-10, l_diff and cost 1e-9 | 1e-12): an observation left
    out of g, the linearisation-point camera in the re-solve, a missing column scale and a stale Huber weight move the
    landmark 2-norm by more than its tolerance; a landmark left out of l_diff is 2e-5 to 2e-3 of it; an observation left out
    of the cost or a stale landmark in it 2e-5 of it.  Only "landmarks unchanged" (l_diff dropped) and "l_diff unchanged"
    (column scale) pass normwise, rightly;
  * what the normwise tests cannot see is the SIZE: the detectable relative change (the smallest power of ten above ten
    times the bound) of one coordinate of x_new of the best-conditioned landmark of three to five observations, and of l_diff:
      POWER_VARPROJ x_new 1e-12, l_diff 1e-7   POWER_SCHUR_COMPLEMENT x_new 1e-12, l_diff 1e-9   step 2 x_new 1e-11, l_diff 1e-10
    A defect of that size on that coordinate is reported on exactly it and moves the landmark 2-norm by less than a
    thousandth of its tolerance (asserted).
"""
from decimal import Decimal, getcontext
from fractions import Fraction as F

import numpy as np
import pytest

import operand_bounds as OB
import rounding_bounds as RB
import step_bounds as SB
from exact_rational import ExactStep1, scale_decimal
from test_operand_bounds import _dec, _tiny, edge_joint, edge_pose

ALPHA, LAM = 0.01, 1e-4
rel = lambda a, b: float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))
# the normwise tolerances in place (tests/test_gpu_step1.py, test_gpu_step2.py, test_gpu_lpl_stream.py)
TOL_LM = {1: 1e-9, 2: 1e-10}
TOL_LDIFF, TOL_COST = 1e-9, 1e-12

_MEMO = {}


def _note(*a):
    print("STEPBOUND", *a)


def _problem(kind, robust):
    """kind: varproj | poba | unscaled | joint."""
    if kind == "joint":
        return edge_joint(robust)
    return edge_pose(robust, **{"varproj": {}, "poba": {"solver": "POWER_SCHUR_COMPLEMENT"}, "unscaled": {"scale_jl": False}}[kind])


def _case(kind, robust):
    """(problem, increment, unmutated operand reference, unmutated applied-step reference) -- computed once, left unchanged."""
    key = (kind, robust)
    if key not in _MEMO:
        p = _problem(kind, robust)
        inc = SB.seeded_increment(p)
        R0 = (OB.joint_operands if kind == "joint" else OB.pose_operands)(p)
        _MEMO[key] = (p, inc, R0, SB.applied(p, inc, R0=R0))
    return _MEMO[key]


def _emu(kind, robust, order):
    key = (kind, robust, order)
    if key not in _MEMO:
        p, inc, _, _ = _case(kind, robust)
        _MEMO[key] = SB.emulate_apply(p, inc, order)
    return _MEMO[key]


def _within(p, R, state, tag):
    res = SB.apply_check(p, R, *state)
    _note(tag, " ".join(f"{n}={r:.3g}" for n, r, _, _ in res))
    bad = [line for _, _, over, line in res if over]
    assert not bad, "\n".join(bad)
    return {n: r for n, r, _, _ in res}


# ---- the long-double references against exact rationals
def test_step1_cost_and_varproj_resolve_against_exact_rational_arithmetic():
    """The long-double cost (trivial norm), new cameras and re-solved landmarks within the long-double model's own bound (or
    1e-17 relative) of the exact values on the tiny problem: sigma to 60 digits, everything else in rationals."""
    p = _tiny()
    getcontext().prec = 60
    D = lambda fr: Decimal(fr.numerator) / Decimal(fr.denominator)
    ex = ExactStep1(p.alpha, p.n_cams, p.lm_off, p.cam_idx, p.obs, p.cams, p.lms)
    Rc = SB.cost_pose(p, u=RB.ULD)
    v = D(ex.cost_none())
    assert abs(_dec(Rc.ref["all_error"][0]) - v) <= max(Decimal(float(Rc.bound["all_error"][0])), Decimal("1e-17") * abs(v))
    inc = SB.seeded_increment(p, scale=1e-2)
    sig = scale_decimal(ex.diag2(), p.eps)
    fr = lambda dec: F(*dec.as_integer_ratio())
    cams_new = [[F(float(p.cams[c, j])) + fr(sig[12 * c + j]) * F(float(inc[12 * c + j])) for j in range(12)] for c in range(p.n_cams)]
    R = SB.apply_pose(p, inc, u=RB.ULD)
    worst = {}
    for name, vals in (("CAMERAS", [D(t) for r in cams_new for t in r]),
                       ("LANDMARKS", [D(t) for r in ExactStep1(p.alpha, p.n_cams, p.lm_off, p.cam_idx, p.obs, cams_new, p.lms).varproj_resolve() for t in r])):
        ref, bound = R.ref[name], R.bound[name]
        assert len(vals) == len(ref)
        for i, v in enumerate(vals):
            err = abs(_dec(ref[i]) - v)
            assert err <= max(Decimal(float(bound[i])), Decimal("1e-17") * abs(v)), (name, i, float(err), float(bound[i]))
            worst[name] = max(worst.get(name, 0.0), float(err) / float(bound[i]))
    _note("exact-rational", worst)


# ---- the references and the oracle: an fp64 implementation of the same formulas lies inside the fp64 bounds
def _oracle(p, robust):
    from oracle import povar_oracle as O
    return O.Oracle(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=robust, huber=p.huber, eps=p.eps)


@pytest.mark.parametrize("robust", ["NONE", "HUBER", "CAUCHY"])
@pytest.mark.parametrize("step", [1, 2])
def test_cost_reference_against_the_oracle_and_both_summation_orders(step, robust):
    p = _problem("varproj" if step == 1 else "joint", robust)
    R = SB.cost(p)
    orc = _oracle(p, robust)
    ro = orc.error_pose(ALPHA, p.cams, p.lms) if step == 1 else orc.error_homogeneous(p.cams, p.lms)
    for tag, ri in (("oracle", ro), ("obs", SB.emulate_cost(p, "obs")), ("lpl", SB.emulate_cost(p, "lpl"))):
        res = SB.cost_check(R, ri, step)
        _note(f"cost step{step}/{robust}/{tag}", " ".join(f"{k}={r:.3g}" for k, r, _ in res))
        assert not any(over for _, _, over in res), res
    if step == 2:
        assert R.aux["z_gap"] > 1 and R.aux["valid_num_obs"] == R.aux["all_num_obs"] == len(p.cam_idx)
    assert all(np.isfinite(R.bound[k]).all() for k in R.bound)  # nothing excluded


@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
@pytest.mark.parametrize("kind", ["varproj", "poba", "joint"])
def test_applied_step_reference_against_the_oracle(kind, robust):
    """back_substitute_pose / _poba / _joint, apply_cam_inc_joint and normalize_joint within the fp64 bounds: checks the
    restatement of l_diff's mixture of scaled and unscaled quantities as well."""
    p, inc, _, R = _case(kind, robust)
    orc = _oracle(p, robust)
    if kind == "joint":
        st, _ = orc.linearize_homogeneous(p.cams, p.lms)
        jls = orc.scale_jl_cols_homogeneous(st)
        sigma = 1.0 / (p.eps + np.sqrt(orc.jp_diag2_homogeneous(st)))
        orc.scale_jp_cols_joint(st, sigma)
        ld, lms = orc.back_substitute_joint(st, jls, p.lam, p.cams, p.lms, inc)
        cams = orc.apply_cam_inc_joint(p.cams, inc, sigma)
        cn, ln = orc.normalize_joint(cams, lms)
        RN = SB.normalize_joint(cams, lms)
        for nm, dev, per, cnt in (("CAMERAS", cn, 12, p.n_c), ("LANDMARKS", ln, 4, p.n_l)):
            r, over, line = SB.report("normalize " + nm, per, dev.reshape(-1), RN.ref[nm], RN.bound[nm], cnt)
            _note(f"normalize/{robust}/oracle {nm}={r:.3g}")
            assert not over, line
        assert np.all(ln[:, 3] == 1.0)
    else:
        st, _, jls, sigma, _ = orc.stage1_pose(ALPHA, p.cams, p.lms)
        orc.scale_jp_cols_pose(st, sigma)
        inc_s = inc * sigma
        cams = p.cams + inc_s.reshape(-1, 12)
        if kind == "varproj":
            ld, lms = orc.back_substitute_pose(ALPHA, st, cams, p.lms, inc_s * (1.0 / sigma))
        else:
            ld, lms = orc.back_substitute_poba(st, jls, LAM, p.lms, inc)
    _within(p, R, (cams, lms, ld), f"apply {kind}/{robust}/oracle")


@pytest.mark.parametrize("order", ["obs", "lpl"])
@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
@pytest.mark.parametrize("kind", ["varproj", "poba", "unscaled", "joint"])
def test_fp64_emulations_within_every_bound(kind, robust, order):
    p, inc, _, R = _case(kind, robust)
    cams, lms, ld = _emu(kind, robust, order)
    _within(p, R, (cams, lms, ld), f"apply {kind}/{robust}/{order}")
    # the cameras without observations: sigma = 1 / eps to gamma_3
    err, bound, c0 = SB.unobserved_moved(p, R, cams, SB.ambient_increment(p, inc))
    assert len(c0) == 1 and (err <= bound).all(), (err / bound).max()
    # the cost at the new point from the state alone; step 2 through normalize_joint as well
    q = SB._with(p, cams=cams, lms=lms)
    res = SB.cost_check(SB.cost(q), SB.emulate_cost(q, order), 2 if kind == "joint" else 1)
    assert not any(over for _, _, over in res), res
    if kind == "joint":
        RN = SB.normalize_joint(cams, lms)
        cn, ln = SB.emulate_normalize(cams, lms)
        for nm, dev in (("CAMERAS", cn), ("LANDMARKS", ln)):
            r, _, over = RB.check(dev.reshape(-1), RN.ref[nm], RN.bound[nm])
            assert not over, (nm, r)


@pytest.mark.parametrize("kind", ["varproj", "poba", "joint"])
def test_conditions_hold_for_the_reference_alone(kind):
    """inv3's first-order condition where H is formed (P_new for POWER_VARPROJ), the |z| gap, nothing excluded."""
    for robust in ("NONE", "HUBER"):
        p, _, _, R = _case(kind, robust)
        assert R.aux["det_ratio"].shape == (p.n_lms,) and R.aux["det_ratio"].max() < OB.DET_RATIO
        assert all(np.isfinite(R.bound[k]).all() and len(R.bound[k]) == len(R.ref[k]) for k in R.bound)
        assert len(R.bound["LANDMARKS"]) == p.lms.size and len(R.bound["CAMERAS"]) == 12 * p.n_cams
        if kind == "joint":
            assert R.aux["z_gap"] > 1
        _note(f"conditions {kind}/{robust} det_ratio={R.aux['det_ratio'].max():.3g}" + (f" z_gap={R.aux['z_gap']:.3g}" if kind == "joint" else ""))


# ---- mutations: a defect on the reference side, the unmutated emulation as the "device"
def _first(p, cam):
    return int(np.flatnonzero(p.cam_idx == cam)[0])


def _lm_flags(p, R, state):
    per = p.lms.shape[1]
    return (SB.flagged(state[0], R.ref["CAMERAS"], R.bound["CAMERAS"], 12), SB.flagged(state[1], R.ref["LANDMARKS"], R.bound["LANDMARKS"], per),
            bool(SB.flagged([state[2]], R.ref["L_DIFF"], R.bound["L_DIFF"], 1)))


def _through(p, Rm, R, step):
    """Does the normwise tolerance in place let the mutated reference through (landmarks, l_diff)?"""
    return (rel(Rm.ref["LANDMARKS"].astype(float), R.ref["LANDMARKS"].astype(float)) < TOL_LM[step],
            abs(float(Rm.ref["L_DIFF"][0] - R.ref["L_DIFF"][0])) <= TOL_LDIFF * abs(float(R.ref["L_DIFF"][0])))


def test_mutation_observation_left_out_of_g():
    """One observation of a tail landmark (seen by a one-observation camera) left out of g in the POWER_VARPROJ re-solve."""
    p, inc, R0, R = _case("varproj", "NONE")
    c1 = int(np.flatnonzero(p.n_c == 1)[0])
    i = _first(p, c1)
    l = int(p.lm[i])
    assert p.n_l[l] >= 2
    Rm = SB.apply_pose(p, inc, {"drop_g": [i]}, R0=R0)
    fc, fl, _ = _lm_flags(p, Rm, _emu("varproj", "NONE", "lpl"))
    assert fc == set() and fl == {l}
    _note("mutation drop_g normwise lets through (landmarks, l_diff):", _through(p, Rm, R, 1))


def test_mutation_linearisation_point_camera_in_the_resolve():
    """The camera of the linearisation point instead of P_new for one one-observation camera: exactly its landmark."""
    p, inc, R0, R = _case("varproj", "HUBER")
    c1 = int(np.flatnonzero(p.n_c == 1)[1])
    l = int(p.lm[_first(p, c1)])
    Rm = SB.apply_pose(p, inc, {"lin_cam": [c1]}, R0=R0)
    fc, fl, _ = _lm_flags(p, Rm, _emu("varproj", "HUBER", "obs"))
    assert fc == set() and fl == {l}
    _note("mutation lin_cam normwise lets through:", _through(p, Rm, R, 1))


@pytest.mark.parametrize("kind", ["poba", "joint"])
def test_mutation_column_scale_not_applied_to_one_coordinate(kind):
    p, inc, R0, R = _case(kind, "NONE")
    l = _best_mid_landmark(p, R)
    Rm = SB.applied(p, inc, {"no_scale": (l, 1)}, R0=R0)
    state = _emu(kind, "NONE", "lpl")
    per = p.lms.shape[1]
    err = np.abs(np.asarray(state[1], dtype=SB.LD).reshape(-1) - Rm.ref["LANDMARKS"]).astype(float)
    assert set(np.flatnonzero(err > Rm.bound["LANDMARKS"]).tolist()) == {per * l + 1}
    assert _lm_flags(p, Rm, state)[0] == set()
    _note(f"mutation no_scale {kind} normwise lets through:", _through(p, Rm, R, 2 if kind == "joint" else 1))


@pytest.mark.parametrize("kind", ["poba", "joint"])
def test_mutation_stale_weight_on_one_huber_outlier(kind):
    """A weight of 1 instead of w on one outlier in the stored rows: the landmark it belongs to, no other."""
    p, inc, R0, R = _case(kind, "HUBER")
    i = int(np.flatnonzero((R0.aux["w"] < 0.7) & (p.n_l[p.lm] >= 3) & (p.n_l[p.lm] <= 5))[0])
    Rm = SB.applied(p, inc, {"w_one": [i]}, R0=R0)
    fc, fl, _ = _lm_flags(p, Rm, _emu(kind, "HUBER", "obs"))
    assert fc == set() and fl == {int(p.lm[i])}
    _note(f"mutation w_one {kind} normwise lets through:", _through(p, Rm, R, 2 if kind == "joint" else 1))


@pytest.mark.parametrize("kind", ["varproj", "poba", "joint"])
def test_mutation_landmark_contribution_dropped_from_l_diff(kind):
    p, inc, R0, R = _case(kind, "HUBER")
    l = _best_mid_landmark(p, R)
    Rm = SB.applied(p, inc, {"drop_ldiff": [l]}, R0=R0)
    fc, fl, fd = _lm_flags(p, Rm, _emu(kind, "HUBER", "lpl"))
    assert fc == set() and fl == set() and fd
    _note(f"mutation drop_ldiff {kind} normwise lets through:", _through(p, Rm, R, 2 if kind == "joint" else 1),
          "share", float(abs(Rm.ref["L_DIFF"][0] - R.ref["L_DIFF"][0]) / abs(R.ref["L_DIFF"][0])))


@pytest.mark.parametrize("step", [1, 2])
def test_mutations_of_the_cost(step):
    """One observation of a one-observation camera dropped from the cost; the old landmark (a stale lane mirror) used for one
    landmark in the cost after an apply."""
    kind = "varproj" if step == 1 else "joint"
    p, inc, _, R = _case(kind, "HUBER")
    cams, lms, _ = _emu(kind, "HUBER", "lpl")
    q = SB._with(p, cams=cams, lms=lms)
    dev = SB.emulate_cost(q, "lpl")
    clean = SB.cost(q)
    assert not any(over for _, _, over in SB.cost_check(clean, dev, step))
    i = _first(p, int(np.flatnonzero(p.n_c == 1)[0]))
    Rm = SB.cost(q, {"drop_cost": [i]})
    with pytest.raises(AssertionError):
        SB.cost_check(Rm, dev, step)  # the count
    for k in SB.COST_FIELDS[step]:
        assert abs(float(dev.__dict__[k] - Rm.ref[k][0])) > Rm.bound[k][0], k
    l = _best_mid_landmark(p, R)
    Rm = SB.cost(q, {"old_lm": ([l], p.lms[[l]])})
    res = SB.cost_check(Rm, dev, step)
    assert all(over for _, _, over in res), res
    share = abs(float(Rm.ref["all_error"][0] - clean.ref["all_error"][0])) / float(clean.ref["all_error"][0])
    _note(f"mutation old_lm step{step}: share of the cost {share:.3g}; the tolerance in place lets it through: {share < TOL_COST}")


# ---- the detectable scale
def _best_mid_landmark(p, R):
    """The best-conditioned landmark of three to five observations (the entrywise bound of its update relative to the
    update is the smallest)."""
    d, Ed = np.abs(R.aux["delta"].astype(float)), R.aux["Edelta"]
    mid = np.flatnonzero((p.n_l >= 3) & (p.n_l <= 5))
    return int(mid[np.argmin((Ed[mid] / np.maximum(d[mid], 1e-300)).max(1))])


DETECTABLE = {"varproj": (1e-12, 1e-7), "poba": (1e-12, 1e-9), "joint": (1e-11, 1e-10)}  # (x_new, l_diff)


@pytest.mark.parametrize("kind", ["varproj", "poba", "joint"])
def test_detectable_scale(kind):
    """The smallest relative change (a power of ten above ten times the bound) of one coordinate of the best-conditioned
    mid-size landmark's x_new and of l_diff that the bounds detect (the recorded scales, module docstring)."""
    p, _, _, R = _case(kind, "NONE")
    l = _best_mid_landmark(p, R)
    per = p.lms.shape[1]
    i = per * l + 1
    sx, sl = SB.detectable(R, "LANDMARKS", i), SB.detectable(R, "L_DIFF", 0)
    _note(f"detectable {kind}: x_new {sx:.0e} l_diff {sl:.0e}")
    assert sx <= DETECTABLE[kind][0] and sl <= DETECTABLE[kind][1]
    # a defect of that size on that one coordinate: the bound reports exactly it; a relative 2-norm over all landmarks moves
    # by less than a thousandth of its tolerance
    cams, lms, ld = _emu(kind, "NONE", "obs")
    ref = R.ref["LANDMARKS"].copy()
    ref[i] *= 1 + SB.LD(sx)
    err = np.abs(np.asarray(lms, dtype=SB.LD).reshape(-1) - ref).astype(float)
    assert set(np.flatnonzero(err > R.bound["LANDMARKS"]).tolist()) == {i}
    assert rel(ref.astype(float), R.ref["LANDMARKS"].astype(float)) < 1e-3 * TOL_LM[2 if kind == "joint" else 1]
    assert abs(float(SB.LD(ld) - R.ref["L_DIFF"][0] * (1 + SB.LD(sl)))) > R.bound["L_DIFF"][0]
