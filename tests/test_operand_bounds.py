"""The operand bounds of tests/operand_bounds.py checked on the CPU: the long-double references against exact rational
arithmetic (step 1) and the CPU oracle (step 2), fp64 NumPy emulations of the kernels' operation order within every
bound, and the defects the normwise tests let through reported by the operand they touch, on every camera or landmark
they touch.

Measured when these tests were written (largest err / bound over every entry of the operand):
  * the long-double step-1 reference against exact rationals, in the long-double model's own bound: diag2 0.15, sigma 0.23,
    Jl scale 0.12, Hll^-1 0.0033, b 0.0014; B_ref within the same model's E(B);
  * fp64 emulations on the edge graph plus one unobserved camera (NONE | HUBER; the per-observation and the lane-per-landmark
    order differ only in b: 0.014 | 0.011 against 0.018 | 0.018):
      step 1   diag2 0.18 | 0.17   sigma 0.26   Jl scale 0.22 | 0.21   Hll^-1 0.027 | 0.023   b 0.018
               B^-1 residual 0.046   B^-1 symmetry 3.9e-4 | 1.3e-4
      step 2   diag2 0.21   sigma 0.25   Jl scale 0.25 | 0.23   Hll^-1 0.013 | 0.014   reflectors 0.24   b 0.012 | 0.0084
               B^-1 residual 0.019 | 0.021   B^-1 symmetry 1.1e-3 | 6.9e-4   N_c^T vec(P_c) 0.050
    and the CPU oracle within the same fp64 step-2 bounds: diag2 0.25, sigma 0.26, Jl scale 0.26, Hll^-1 0.013 | 0.015,
    b 0.012 | 0.0084, B^-1 residual 0.030 | 0.021, symmetry 7.5e-4 | 4.8e-4.
    diag2, sigma, the scales and the reflectors are a handful of roundings on one- and two-observation blocks: a quarter of
    the bound is one rounding out of four, as tight as a first-order bound gets.  Hll^-1, b and the residual compound
    absolute-value maps the way the E0 bounds do (0.01 to 0.05 there as well).  The symmetry ratios are the smallest:
    the bound carries the worst-case residual through |B^-1| once more, while the columns of chol_inverse_16 share one L
    and differ from the transpose by a few ulps of the entries -- pessimistic by |B^-1| |B|, not vacuous: the bound
    is 2e-10 to 4e-9 of the off-diagonal entries of a hub's block, 5e-12 to 3e-10 on a 118-observation camera, and up to
    1e-6 of an entry only on the one-observation cameras, whose B is lambda I plus a rank-two block.
  * the first-order condition of inv3_bound, E(det) / |det|: at most 5.5e-7 on the step-1 edge graph (the 60 near-parallel
    two-view landmarks, cond(Hll) above 1e6 on at least two of them), 5.0e-5 on the step-2 one (2^-10 = 9.8e-4 is asserted);
  * detectable relative scale of one entry (the smallest power of ten above ten times its bound): entry (0, 1) of the
    best-conditioned landmark's Hll^-1, entry 2 of b and the diagonal entry (2, 2) of B^-1 of the mid camera (20 to 400
    observations) whose worst landmark is best conditioned (cond(Hll) below 10 on all of them):
      step 1   Hll^-1 1e-11   b 1e-8   B^-1 1e-12            step 2   Hll^-1 1e-10   b 1e-11   B^-1 1e-12
    On a camera that shares near-parallel two-view landmarks with its twin (camera 4) b's bound is 3e-8 to 1.6e-6 of the
    entry in step 1: E(Hll^-1) of those landmarks enters b as an operand perturbation, and b is the gradient close to the
    minimum, where the residual part and the eliminated part cancel -- conditioning of the data, not a loose count (the
    emulation uses a hundredth of the bound there as elsewhere).
"""
from decimal import Decimal, getcontext
from fractions import Fraction as F

import numpy as np
import pytest

import operand_bounds as OB
import rounding_bounds as RB
from exact_rational import ExactStep1, scale_decimal

ALPHA, LAM = 0.01, 1e-4
POSE_OPS = [("DIAG2", 12, "c"), ("SIGMA", 12, "c"), ("JL_COL_SCALE", 3, "l"), ("HLL_INV", 9, "l"), ("B", 12, "c")]
JOINT_OPS = [("DIAG2", 12, "c"), ("SIGMA", 12, "c"), ("JL_COL_SCALE_H", 4, "l"), ("HLL_INV", 9, "l"), ("NC_HOUSEHOLDER", 13, "c"),
             ("B_JOINT", 11, "c")]


def _counts(p, kind):
    return p.n_c if kind == "c" else p.n_l


# ---- step 1: the long-double reference against exact rationals
def _dec(x):
    """A long double as an exact Decimal (its 64-bit significand splits into two doubles)."""
    hi = float(x)
    return Decimal(hi) + Decimal(float(x - np.longdouble(hi)))


def _tiny():
    """Four cameras (one of them with a single observation), seven landmarks of two or three views."""
    rng = np.random.default_rng(3)
    lists = [[0, 1], [0, 2], [1, 2], [0, 1, 2], [0, 1, 3], [1, 2], [0, 2]]
    lm_off = np.concatenate([[0], np.cumsum([len(t) for t in lists])])
    cam_idx = np.concatenate(lists)
    cams = np.zeros((4, 12))
    cams[:, :8] = 2.0 * rng.normal(size=(4, 8))
    cams[:, 8:11] = 0.05 * rng.normal(size=(4, 3))
    cams[:, 11] = 1.0
    X = rng.normal(size=(7, 3))
    lm = np.repeat(np.arange(7), np.diff(lm_off))
    pc = np.einsum("nij,nj->ni", cams[cam_idx].reshape(-1, 3, 4), np.concatenate([X[lm], np.ones((len(lm), 1))], 1))
    obs = np.rint((pc[:, :2] / pc[:, 2:3] + rng.normal(scale=0.05, size=(len(lm), 2))) * 1e6) / 1e6
    return OB.Pose(4, lm_off, cam_idx, obs, cams, X, ALPHA, LAM)


def test_step1_longdouble_reference_against_exact_rational_arithmetic():
    """Every step-1 operand's reference within the long-double model's own bound (or 1e-17 relative) of the exact value:
    diag2, b and Hpp from the reference's explicit rows in rationals, the square roots to 60 digits."""
    p = _tiny()
    ex = ExactStep1(p.alpha, p.n_cams, p.lm_off, p.cam_idx, p.obs, p.cams, p.lms)
    getcontext().prec = 60
    D = lambda fr: Decimal(fr.numerator) / Decimal(fr.denominator)
    d2 = ex.diag2()
    sig = scale_decimal(d2, p.eps)
    s = [scale_decimal(t, p.eps) for t in ex.jl_col_sq()]
    hi = [D(H[a][b]) / (s[l][a] * s[l][b]) for l, H in enumerate(ex.hll_inv()) for a in range(3) for b in range(3)]
    b = [sg * D(t) for sg, t in zip(sig, ex.b())]
    exact = {"DIAG2": [D(t) for t in d2], "SIGMA": sig, "JL_COL_SCALE": [t for r in s for t in r], "HLL_INV": hi, "B": b}
    sd = np.array([float(t) for t in sig])
    R = OB.pose_operands(p, sigma_dev=sd, u=RB.ULD)
    for name, vals in exact.items():
        ref, bound = R.ref[name], R.bound[name]
        assert len(vals) == len(ref)
        for i, v in enumerate(vals):
            err = abs(_dec(ref[i]) - v)
            assert err <= max(Decimal(float(bound[i])), Decimal("1e-17") * abs(v)), (name, i, float(err), float(bound[i]))
    Hpp = ex.hpp()
    B, EB = R.aux["B_INV"]["B"], R.aux["B_INV"]["EB"]
    for c in range(p.n_cams):
        for i in range(12):
            for j in range(12):
                v = Decimal(float(sd[12 * c + i])) * Decimal(float(sd[12 * c + j])) * D(Hpp[c][i][j]) + (Decimal(p.lam) if i == j else 0)
                err = abs(_dec(B[c, i, j]) - v)
                assert err <= max(Decimal(float(EB[c, i, j])), Decimal("1e-17") * abs(v)), (c, i, j, float(err))


# ---- the edge problems
def edge_pose(robust, **kw):
    n_c, lm_off, cam_idx, obs, cams, lms = RB.edge_problem(0)
    cams = np.concatenate([cams, cams[:1] + 0.5], 0)  # one appended camera without observations
    return OB.Pose(n_c + 1, lm_off, cam_idx, obs, cams, lms, ALPHA, LAM, robust, RB.EDGE_HUBER, **kw)


def edge_joint(robust):
    n_c, lm_off, cam_idx, obs, cams, X = RB.edge_problem_joint(0)
    return OB.Joint(n_c, lm_off, cam_idx, obs, cams, X, RB.EDGE_LAM_H, robust, RB.EDGE_HUBER_H)


_MEMO = {}


def _case(step, robust):
    """(problem, emulations by form, unmutated reference) -- computed once and left unchanged."""
    key = (step, robust)
    if key not in _MEMO:
        if step == 1:
            p = edge_pose(robust)
            em = {f: OB.emulate_pose(p, f) for f in ("obs", "lpl")}
            R = OB.pose_operands(p, sigma_dev=em["obs"]["SIGMA"])
        else:
            p = edge_joint(robust)
            em = {"obs": OB.emulate_joint(p)}
            R = OB.joint_operands(p, sigma_dev=em["obs"]["SIGMA"])
        _MEMO[key] = (p, em, R)
    return _MEMO[key]


def _ratios(p, R, dev, ops, bname, n):
    out = {}
    for name, per, kind in ops:
        r, over, line = OB.report(name, per, dev[name], R.ref[name], R.bound[name], _counts(p, kind))
        assert over == 0, line
        out[name] = r
    res, Rb, asym, ab = OB.binv_check(R, bname, p, dev[bname])
    for what, a, b in (("residual", res, Rb), ("symmetry", asym, ab)):
        r, over, line = OB.report(f"{bname} {what}", n * n, a, np.zeros_like(a), b, p.n_c)
        assert over == 0, line
        out[what] = r
    return out


@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
def test_step1_emulations_within_every_bound(robust):
    p, em, R = _case(1, robust)
    assert R.aux["det_ratio"].max() < 1e-6  # (the condition inv3_bound asserts, with room: the largest is 5.5e-7)
    cond = np.linalg.cond(R.aux["H"].astype(np.float64))
    assert (cond > 1e6).sum() >= 2 and (p.n_c == 0).sum() == 1
    for form in ("obs", "lpl"):
        Rf = R if form == "obs" else OB.pose_operands(p, sigma_dev=em[form]["SIGMA"])
        out = _ratios(p, Rf, em[form], POSE_OPS, "B_INV", 12)
        print(f"OPBOUND-CPU step1 {robust} {form} " + " ".join(f"{k}={v:.3g}" for k, v in out.items()))
        for k, v in out.items():  # neither a missing count nor a vacuous bound
            assert 1e-5 < v < 0.5, (k, v)
    c0 = int(np.flatnonzero(p.n_c == 0)[0])
    for form in ("obs", "lpl"):
        e = em[form]
        assert np.all(e["DIAG2"].reshape(-1, 12)[c0] == 0) and np.all(e["B"].reshape(-1, 12)[c0] == 0)
        assert np.all(np.abs(e["SIGMA"].reshape(-1, 12)[c0] * p.eps - 1) <= OB.g(3))
        X = e["B_INV"].reshape(-1, 12, 12)[c0]
        assert np.all(X - np.diag(np.diag(X)) == 0) and np.all(np.abs(np.diag(X) * p.lam - 1) <= OB.g(3))


@pytest.mark.parametrize("what", ["POWER_SCHUR_COMPLEMENT", "unscaled_jl"])
def test_step1_emulation_solver_type_and_unscaled_jl(what):
    p = edge_pose("NONE", solver="POWER_SCHUR_COMPLEMENT") if what == "POWER_SCHUR_COMPLEMENT" else edge_pose("HUBER", scale_jl=False)
    em = OB.emulate_pose(p, "lpl")
    R = OB.pose_operands(p, sigma_dev=em["SIGMA"])
    _ratios(p, R, em, POSE_OPS, "B_INV", 12)
    if what == "unscaled_jl":
        assert np.all(R.ref["JL_COL_SCALE"] == 1) and np.all(R.bound["JL_COL_SCALE"] == 0)


@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
def test_step2_emulation_within_every_bound(robust):
    p, em, R = _case(2, robust)
    assert R.aux["det_ratio"].max() < 1e-4
    out = _ratios(p, R, em["obs"], JOINT_OPS, "B_INV_JOINT", 11)
    v, vb = OB.nc_nullspace(R, p, em["obs"]["NC_HOUSEHOLDER"])
    r, over, line = OB.report("N_c^T vec(P_c)", 11, v, np.zeros_like(v), vb, p.n_c)
    assert over == 0, line
    out["nullspace"] = r
    print(f"OPBOUND-CPU step2 {robust} " + " ".join(f"{k}={v:.3g}" for k, v in out.items()))
    for k, val in out.items():
        assert 1e-5 < val < 0.5, (k, val)
    c0 = int(np.flatnonzero(p.n_c == 0)[0])
    e = em["obs"]
    assert np.all(e["DIAG2"].reshape(-1, 12)[c0] == 0) and np.all(e["B_JOINT"].reshape(-1, 11)[c0] == 0)
    X = e["B_INV_JOINT"].reshape(-1, 11, 11)[c0]
    assert np.all(X - np.diag(np.diag(X)) == 0) and np.all(np.abs(np.diag(X) * p.lam - 1) <= OB.g(3))


@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
def test_step2_reference_against_the_oracle(robust):
    """The CPU oracle (fp64, the reference's explicit tiles and the same Householder bases) within the fp64 bounds of the
    long-double step-2 reference."""
    from oracle import povar_oracle as O
    p = edge_joint(robust)
    orc = O.Oracle(p.n_cams, p.lm_off.astype(np.int32), p.cam_idx.astype(np.int32), p.obs, robust_norm=robust, huber=p.huber)
    st_h, ok = orc.linearize_homogeneous(p.cams, p.lms)
    assert ok
    diag2 = orc.jp_diag2_homogeneous(st_h)
    jls = orc.scale_jl_cols_homogeneous(st_h)
    sigma = 1.0 / (p.eps + np.sqrt(diag2))
    orc.scale_jp_cols_joint(st_h, sigma)
    st_n = orc.linearize_nullspace(p.cams, p.lms, st_h)
    hll, b, binv = orc.prepare_hb_joint(st_h, st_n, p.lam)
    dev = {"DIAG2": diag2, "SIGMA": sigma, "JL_COL_SCALE_H": jls, "HLL_INV": hll, "B_JOINT": b, "B_INV_JOINT": binv}
    R = OB.joint_operands(p, sigma_dev=sigma)
    ops = [o for o in JOINT_OPS if o[0] != "NC_HOUSEHOLDER"]
    out = _ratios(p, R, dev, ops, "B_INV_JOINT", 11)
    print(f"OPBOUND-CPU oracle {robust} " + " ".join(f"{k}={v:.3g}" for k, v in out.items()))


# ---- mutations: each defect is reported by the operand it touches, on every camera or landmark it touches
def _reported(p, R, dev, name, per, joint):
    if name.startswith("B_INV"):
        res, Rb, _, _ = OB.binv_check(R, name, p, dev[name])
        return OB.flagged(res, np.zeros_like(res), Rb, per)
    return OB.flagged(dev[name], R.ref[name], R.bound[name], per)


@pytest.mark.parametrize("step", [1, 2])
def test_structural_mutations_are_reported(step):
    p, em, R = _case(step, "HUBER")
    dev = em["obs"]
    fn = OB.pose_operands if step == 1 else OB.joint_operands
    muts = OB.structural_mutations(p, R, step == 2)
    assert len(muts) == (9 if step == 1 else 10)
    for name, mutate, expect in muts:
        Rm = fn(p, sigma_dev=dev["SIGMA"], mutate=mutate)
        for op, per, blocks in expect:
            got = _reported(p, Rm, dev, op, per, step == 2)
            want = set(range(len(Rm.ref[op]) // per)) if blocks is None else blocks
            assert want <= got, (name, op, sorted(want - got)[:5])
            clean = _reported(p, R, dev, op, per, step == 2)
            assert not clean, (name, op)


@pytest.mark.parametrize("step", [1, 2])
def test_detectable_relative_scale_of_hll_inv_b_and_b_inv(step):
    """The smallest power of ten above ten times the entry's bound, applied to one entry of the best-conditioned landmark's
    Hll^-1, and of b and B^-1 of the mid camera (20 to 400 observations) whose worst landmark is best conditioned, is
    reported; none of the three scales is above 1e-6."""
    p, em, R = _case(step, "NONE")
    dev = em["obs"]
    fn = OB.pose_operands if step == 1 else OB.joint_operands
    bn, binv, n = ("B", "B_INV", 12) if step == 1 else ("B_JOINT", "B_INV_JOINT", 11)
    cond = np.linalg.cond(R.aux["H"].astype(np.float64))
    l = int(np.argmin(cond))
    worst = np.zeros(p.n_cams)
    np.maximum.at(worst, p.cam_idx, cond[p.lm])  # (a camera is as well-conditioned as the worst landmark it sees)
    mids = np.flatnonzero((p.n_c > 20) & (p.n_c < 400))
    c = int(mids[np.argmin(worst[mids])])
    print(f"OPBOUND-CPU step{step} camera {c}: {p.n_c[c]} observations, largest cond(Hll) of its landmarks {worst[c]:.3g}")
    scales = {}
    for op, i, per, blk in (("HLL_INV", 9 * l + 1, 9, l), (bn, n * c + 2, n, c)):
        s = OB.entry_scale(R, op, i)
        scales[op] = s
        Rm = fn(p, sigma_dev=dev["SIGMA"], mutate={"entry": {op: (i, 1 + s)}})
        assert blk in OB.flagged(dev[op], Rm.ref[op], Rm.bound[op], per), (op, s)
    # B^-1: the diagonal entry (2, 2) of the device's block scaled; its share of the residual is B_22 X_22 s
    res, Rb, _, _ = OB.binv_check(R, binv, p, dev[binv])
    X = dev[binv].reshape(-1, n, n).copy()
    B = R.aux[binv]["B"].astype(np.float64)
    s = 10.0 ** np.ceil(np.log10(10 * Rb[c, 2, 2] / (B[c, 2, 2] * abs(X[c, 2, 2]))))
    scales[binv] = s
    X[c, 2, 2] *= 1 + s
    res, Rb, _, _ = OB.binv_check(R, binv, p, X)
    assert c in OB.flagged(res, np.zeros_like(res), Rb, n * n)
    print(f"OPBOUND-CPU step{step} detectable scales " + " ".join(f"{k}={v:.0e}" for k, v in scales.items()))
    for k, v in scales.items():
        assert v <= 1e-6, (k, v)
