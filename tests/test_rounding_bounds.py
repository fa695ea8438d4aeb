"""The componentwise bounds of tests/rounding_bounds.py (step 1 and step 2) checked on the CPU: the long-double references
against exact rational arithmetic, NumPy emulations of the fp64 and fp32 kernels within their bounds, and deliberate defects
reported as violations (the bounds are sharp, not vacuous).

Slack measured when these tests were written (largest err / bound over every output entry):
  * the long-double reference against the exact E0 x of the golden problem: below 0.05;
  * on the edge graph (rounding_bounds.edge_problem: hubs, one- and two-observation cameras, long landmarks, cond(Hll) above
    1e6, |u| above 16.78, packed and unpacked points), x ~ N(0, 1) and per-camera scales 10^U(-4, 4):
      fp64 emulation / fp64 bound  0.019 (NONE), 0.041 (HUBER);   fp32 emulation / fp32 bound  0.017 (NONE), 0.023 (HUBER);
    and the fp32 emulation exceeds the fp64 bound by 1e7 (the two bounds are far apart, as they should be).
    The MI355X kernels reach 0.001 to 0.048 of their bounds (tests/test_gpu_e0_bounds.py): the same slack as the emulations.

Step 2 (rounding_bounds.evaluate_joint: the next power-series term of the joint system, 11 entries per camera):
  * the long-double reference against the exact term of the golden step-2 problem (explicit tangent tiles in rationals, the
    reflectors given): below 0.05 as well;
  * the ambient image of the reference's first five terms on medium_problem against the CPU oracle's: within 1e-11;
  * on the step-2 edge graph (rounding_bounds.edge_problem_joint: the same graph plus an unobserved camera, X.x of either sign
    and exactly 0, X_w != 1, depths down to 1e-2 of the typical one), the real term sequence, largest err / bound:
      e0_ck_h emulation / ckh bound   1.0e-3 (NONE, CAUCHY), 5.9e-4 (HUBER);
      Jl3 emulation / jl3 bound       7.5e-4 (NONE, CAUCHY), 4.3e-4 (HUBER);
    the MI355X kernels (tests/test_gpu_e0h_bounds.py, largest over the five terms of every case):
      edge graph   lm_h 7.1e-4, e0_lm_cached_h 1.1e-3, e0_lpl_h 7.6e-4, e0_ck_h 8.0e-4, e0_ck_h_det 6.3e-4;
      257 cameras  e0_lpl_h 2.8e-4, e0_ck_h 3.3e-4, e0_ck_h_det 2.3e-4;   700 cameras, either stride: e0_ck_h 5.6e-4;
    no term of any case below 6e-5 -- the same slack as the emulations, so nothing points at a missing count.  The ratios are
    ten to forty times smaller than step 1's because the worst case compounds through four more absolute-value maps (|N_l|
    twice, |N_c|^T, the 11x11 |B^-1|) and about three times as many roundings per entry, none of which a real run aligns:
    pessimistic by the usual sqrt-of-the-count statistics, not by a wrong count.  What the bound cannot see: at
    lambda = 1e-4 a one-observation camera's |B^-1| |y11| is 1e6 to 1e7 times |B^-1 y11| (entries near 1 / lambda), so the
    bound there is 2e-8 to 2e-5 of the entry: a relative 1e-9 defect of such a block is below what fp64 itself may do
    (test_step2_mutation_scaled_tail_camera_block runs at lambda = 1 for that reason).
"""
import os
from decimal import Decimal, getcontext
from fractions import Fraction as F

import numpy as np
import pytest

import rounding_bounds as RB
from exact_rational import ExactStep1

HERE = os.path.dirname(os.path.abspath(__file__))


def _ld(fr):
    getcontext().prec = 40
    return np.longdouble(str(Decimal(fr.numerator) / Decimal(fr.denominator)))


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "step1_small_none.npz"))
    n_c = int(g["n_cams"])
    ex = ExactStep1(float(g["alpha"]), n_c, g["lm_off"], g["cam_idx"], g["obs"], g["cams"], g["lms"])
    G = np.array([[[_ld(Hi[a][b]) for b in range(3)] for a in range(3)] for _, Hi in ex.lm], dtype=np.longdouble)
    prob = RB.Step1(n_c, g["lm_off"], g["cam_idx"], g["obs"], g["cams"], g["lms"], float(g["alpha"]), g["sigma"], G)
    sg = [F(float(t)) for t in g["sigma"]]
    x = np.random.default_rng(5).normal(size=12 * n_c)
    y_exact = [s * t for s, t in zip(sg, ex.e0([F(float(a)) * s for a, s in zip(x, sg)]))]
    return prob, x, np.array([_ld(t) for t in y_exact], dtype=np.longdouble)


def test_longdouble_reference_against_exact_rational_arithmetic(golden):
    """The C-form restatement, the scalings taken as exact and sigma: the long-double reference is within its own bound of
    the exact E0 x (exact_rational builds the reference's explicit rows, not the C-form)."""
    prob, x, y_exact = golden
    y_ref, bound = RB.evaluate(prob, x, RB.MODELS["longdouble"])
    worst, i, n_over = RB.check(y_ref, y_exact, bound)
    assert n_over == 0, (worst, i)
    assert worst < 0.5


@pytest.mark.parametrize("dtype,model", [(np.float64, "fp64"), (np.float32, "fp32")])
def test_emulation_against_exact_rational_arithmetic(golden, dtype, model):
    prob, x, y_exact = golden
    _, bound = RB.evaluate(prob, x, RB.MODELS[model])
    worst, i, n_over = RB.check(RB.emulate(prob, x, dtype), y_exact, bound)
    assert n_over == 0, (worst, i)


def _edge(robust):
    n_c, lm_off, cam_idx, obs, cams, lms = RB.edge_problem(0)
    prob, s, Hi = RB.system(n_c, lm_off, cam_idx, obs, cams, lms, 0.01, robust, RB.EDGE_HUBER)
    assert (np.linalg.cond(Hi) >= 1e6).any()
    assert ((prob.n_c >= 1) & (prob.n_c <= 2)).mean() >= 0.3 and prob.n_l.max() > 64 and prob.n_c.max() > 1000
    assert (np.abs(obs) > 16.78).any()
    return prob


@pytest.fixture(scope="module", params=["NONE", "HUBER"])
def edge(request):
    return _edge(request.param)


def _inputs(n_c):
    rng = np.random.default_rng(7)
    x = rng.normal(size=12 * n_c)
    return [x, x * np.repeat(10.0 ** rng.uniform(-4, 4, n_c), 12)]


@pytest.mark.parametrize("dtype,model", [(np.float64, "fp64"), (np.float32, "fp32")])
def test_emulation_on_the_edge_graph(edge, dtype, model):
    for x in _inputs(edge.n_cams):
        y_ref, bound = RB.evaluate(edge, x, RB.MODELS[model])
        worst, i, n_over = RB.check(RB.emulate(edge, x, dtype), y_ref, bound)
        assert n_over == 0, (worst, i)
        assert worst > 1e-4  # (not vacuous: the emulation uses a visible share of its bound)


def test_fp32_emulation_breaks_the_fp64_bound(edge):
    x = _inputs(edge.n_cams)[0]
    y_ref, bound = RB.evaluate(edge, x, RB.MODELS["fp64"])
    assert RB.check(RB.emulate(edge, x, np.float32), y_ref, bound)[2] > 0


# ---- mutations: a wrong "device" result must be reported
def _violates(prob, x, y_bad, model="fp64"):
    y_ref, bound = RB.evaluate(prob, x, RB.MODELS[model])
    return RB.check(y_bad, y_ref, bound)[2] > 0


def test_mutation_dropped_observation_of_a_tail_camera(edge):
    x = _inputs(edge.n_cams)[1]
    cam = int(np.flatnonzero((edge.n_c >= 1) & (edge.n_c <= 2))[0])
    i = int(np.flatnonzero(edge.cam_idx == cam)[0])

    def drop(w, o0, o1):
        w = w.copy()
        if o0 <= i < o1:
            w[i - o0] = 0
        return w
    y_bad, _ = RB.evaluate(edge, x, RB.MODELS["fp64"], mutate={"w": drop})
    assert _violates(edge, x, y_bad)


def test_mutation_perturbed_landmark_block(edge):
    x = _inputs(edge.n_cams)[0]
    lm = int(np.argmax(edge.n_l))

    def pert(G, l0, l1):
        G = G.copy()
        if l0 <= lm < l1:
            G[lm - l0] *= 1 + np.longdouble(2.0 ** -20)
        return G
    y_bad, _ = RB.evaluate(edge, x, RB.MODELS["fp64"], mutate={"G": pert})
    assert _violates(edge, x, y_bad)


def _round_bits(a, bits):
    m, e = np.frexp(np.asarray(a, dtype=np.float64))
    return np.ldexp(np.rint(m * 2.0 ** bits) / 2.0 ** bits, e)


def test_mutation_half_precision_operands(edge):
    """h~ and G rounded to 11 significant bits: caught by the fp32 bound."""
    import copy
    x = _inputs(edge.n_cams)[0]
    bad = copy.copy(edge)
    bad.lms = _round_bits(edge.lms, 11)
    bad.G = _round_bits(edge.G.astype(np.float64), 11).astype(np.longdouble)
    y_bad, _ = RB.evaluate(bad, x, RB.MODELS["fp32"])
    assert _violates(edge, x, y_bad, "fp32")


def test_mutation_huber_weight_one():
    edge = _edge("HUBER")
    w, _ = RB.weights(edge, edge.cams[edge.cam_idx].astype(np.longdouble), [np.repeat(edge.lms[:, k], edge.n_l).astype(np.longdouble)
                      for k in range(3)], edge.obs.astype(np.longdouble), 1 - np.longdouble(0.01), np.longdouble(0.01), RB.MODELS["fp32"])
    assert (w < 1).mean() > 0.2 and (w == 1).mean() > 0.2  # (the threshold splits the residuals)
    x = _inputs(edge.n_cams)[0]
    y_bad, _ = RB.evaluate(edge, x, RB.MODELS["fp64"], mutate={"w": lambda w, o0, o1: np.ones_like(w)})
    assert _violates(edge, x, y_bad, "fp32")


def test_mutation_scaled_tail_camera_block(edge):
    x = _inputs(edge.n_cams)[1]
    y_ref, _ = RB.evaluate(edge, x, RB.MODELS["fp64"])
    cam = int(np.flatnonzero((edge.n_c >= 1) & (edge.n_c <= 2))[-1])
    y_bad = y_ref.copy()
    y_bad[12 * cam:12 * cam + 12] *= 1 + np.longdouble(1e-9)
    assert _violates(edge, x, y_bad)


# ======== step 2 (rounding_bounds.evaluate_joint: the joint system's next term and its bound)
def _state(p, seed=11):  # (the step-2 state of tests/test_gpu_step2.py)
    rng = np.random.default_rng(seed)
    cams = rng.normal(size=(p.n_cams, 12))
    cams[:, 8:11] *= 0.1
    cams[:, 11] = 5 + rng.random(p.n_cams)
    cams /= np.linalg.norm(cams, axis=1, keepdims=True)
    lms_h = np.concatenate([rng.normal(size=(p.n_lms, 3)), np.ones((p.n_lms, 1))], 1)
    return cams, lms_h, p.obs / 500.0


def _exact_joint_term(prob, x):
    """B^-1 Jp11^T Jl3 Hll^-1 Jl3^T Jp11 x in exact rationals from the explicit tiles Jp11 = Jp12 N_c, Jl3 = Jl4 N_l of
    povar_kernels_joint.hpp's header comment (unit weights), every operand of `prob` -- the reflectors (w, beta) included --
    taken as the rational it is."""
    Q = lambda a: [F(float(v)) for v in a]
    n_c, n_l = prob.n_cams, len(prob.n_l)

    def basis(w, beta):  # N = (I - beta w w^T)[:, 1:]
        return [[(1 if i == j else 0) - beta * w[i] * w[j] for j in range(1, len(w))] for i in range(len(w))]
    Nc = [basis(Q(prob.ncw[c, :12]), F(float(prob.ncw[c, 12]))) for c in range(n_c)]
    Nl = [basis(Q(prob.lw[l, :4]), F(float(prob.lw[l, 4]))) for l in range(n_l)]
    xs = [Q(x[11 * c:11 * c + 11]) for c in range(n_c)]
    y11 = [[F(0)] * 11 for _ in range(n_c)]
    for l in range(n_l):
        X, s = Q(prob.lms[l]), Q(prob.s[l])
        rows = []
        for i in range(int(prob.lm_off[l]), int(prob.lm_off[l + 1])):
            c = int(prob.cam_idx[i])
            P, sg = Q(prob.cams[c]), Q(prob.sigma[c])
            pc = [sum(P[4 * r + j] * X[j] for j in range(4)) for r in range(3)]
            D = [[1 / pc[2], 0, -pc[0] / pc[2] ** 2], [0, 1 / pc[2], -pc[1] / pc[2] ** 2]]
            jp12 = [[D[r][a] * X[j] * sg[4 * a + j] for a in range(3) for j in range(4)] for r in range(2)]
            jp11 = [[sum(jp12[r][k] * Nc[c][k][m] for k in range(12)) for m in range(11)] for r in range(2)]
            jl4 = [[sum(D[r][a] * P[4 * a + j] for a in range(3)) * s[j] for j in range(4)] for r in range(2)]
            jl3 = [[sum(jl4[r][k] * Nl[l][k][m] for k in range(4)) for m in range(3)] for r in range(2)]
            rows.append((c, jp11, jl3))
        u3 = [sum(jl3[r][m] * sum(jp11[r][k] * xs[c][k] for k in range(11)) for c, jp11, jl3 in rows for r in range(2)) for m in range(3)]
        hi = [[F(float(prob.hi[l, min(a, b), max(a, b)])) for b in range(3)] for a in range(3)]
        g = [sum(hi[a][b] * u3[b] for b in range(3)) for a in range(3)]
        for c, jp11, jl3 in rows:
            v = [sum(jl3[r][m] * g[m] for m in range(3)) for r in range(2)]
            y11[c] = [y11[c][k] + jp11[0][k] * v[0] + jp11[1][k] * v[1] for k in range(11)]
    return [sum(F(float(prob.binv[c, i, j])) * y11[c][j] for j in range(11)) for c in range(n_c) for i in range(11)]


def test_step2_longdouble_reference_against_exact_rational_arithmetic():
    """The ambient restatement (U4 / G4, N_l once per landmark) against the explicit tangent tiles in exact rationals on the
    golden step-2 problem: within the reference's own bound and below half of it."""
    g = np.load(os.path.join(HERE, "golden", "step2_small.npz"))
    prob = RB.system_joint(int(g["n_cams"]), g["lm_off"], g["cam_idx"], g["obs"], g["cams"], g["lms_h"], float(g["lam"]), eps=float(g["eps"]))
    lw, lb = RB.house4(prob.lms)
    prob.lw = np.concatenate([lw, lb[:, None]], 1)
    x = np.random.default_rng(5).normal(size=11 * prob.n_cams)
    t_exact = np.array([_ld(v) for v in _exact_joint_term(prob, x)], dtype=np.longdouble)
    t_ref, bound = RB.evaluate_joint(prob, x, RB.MODELS_H["longdouble"])
    worst, i, n_over = RB.check(t_ref, t_exact, bound)
    assert n_over == 0, (worst, i)
    assert 0 < worst < 0.5
    for form, model in (("ambient", "ckh"), ("jl3", "jl3")):  # (and the fp64 emulations against the exact term)
        _, b64 = RB.evaluate_joint(prob, x, RB.MODELS_H[model])
        assert RB.check(RB.emulate_joint(prob, x, form), t_exact, b64)[2] == 0


def test_step2_reference_terms_against_the_oracle(medium_problem):
    """Basis-independent: the ambient image N_c t_i of the reference's terms against the CPU oracle's, 1e-11 relative (the
    tolerance of the golden test's ambient terms)."""
    from oracle import povar_oracle as O
    p = medium_problem
    cams, lms_h, obs = _state(p)
    lam, m = 1e-4, 5
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, obs)
    st_h, ok = orc.linearize_homogeneous(cams, lms_h)
    sigma = 1.0 / (1e-5 + np.sqrt(orc.jp_diag2_homogeneous(st_h)))
    jls = orc.scale_jl_cols_homogeneous(st_h)
    orc.scale_jp_cols_joint(st_h, sigma)
    st_n = orc.linearize_nullspace(cams, lms_h, st_h)
    hll, b, binv = orc.prepare_hb_joint(st_h, st_n, lam)
    _, _, _, terms = orc.solve_joint(st_n, hll, binv, b, m, want_terms=True)
    ncw = RB.system_joint(p.n_cams, p.lm_off, p.cam_idx, obs, cams, lms_h, lam).ncw  # (house of vec(P_c): the oracle's basis)
    prob = RB.Step2(p.n_cams, p.lm_off, p.cam_idx, obs, cams, lms_h, sigma, jls, hll, ncw, binv)
    t = terms[0]
    for i in range(1, m + 1):
        t, _ = RB.evaluate_joint(prob, t.astype(np.float64))
        a, b_ = RB.ambient(prob, t).astype(np.float64), RB.ambient(prob, terms[i]).astype(np.float64)
        assert np.linalg.norm(a - b_) <= 1e-11 * np.linalg.norm(b_), i


_EDGE_H = {}


def _edge_h(robust):
    if robust not in _EDGE_H:
        n_c, lm_off, cam_idx, obs, cams, X = RB.edge_problem_joint(0)
        prob = RB.system_joint(n_c, lm_off, cam_idx, obs, cams, X, RB.EDGE_LAM_H, robust, RB.EDGE_HUBER_H)
        assert n_c == 151 and prob.n_c[-1] == 0 and prob.n_c.max() > 1000 and prob.n_l.max() > 64
        assert ((prob.n_c >= 1) & (prob.n_c <= 2)).mean() >= 0.3
        assert min((X[:, 0] < 0).mean(), (X[:, 0] > 0).mean(), (X[:, 0] == 0).mean()) >= 0.1 and (X[:, 3] != 1).mean() >= 0.2
        assert (cams[:, 0] < 0).sum() >= 20 and (cams[:, 0] > 0).sum() >= 20
        _, _, parts = RB.evaluate_joint(prob, prob.t0, want_parts=True)
        az = np.abs(parts["pz"].astype(np.float64))
        assert az.min() >= 1e-5 and 24 <= (az <= 0.02 * np.median(az)).sum() <= 200  # (small depths, every observation valid)
        if robust == "HUBER":  # (the threshold splits the residuals)
            assert (parts["sw"] < 1).mean() > 0.2 and (parts["sw"] == 1).mean() > 0.2
        _EDGE_H[robust] = prob
    return _EDGE_H[robust]


def _terms_h(prob, n=5):
    """The real term sequence in fp64 (the e0_ck_h emulation's)."""
    ts = [prob.t0]
    for _ in range(n):
        ts.append(RB.emulate_joint(prob, ts[-1], "ambient"))
    return ts


@pytest.mark.parametrize("robust", ["NONE", "HUBER", "CAUCHY"])
@pytest.mark.parametrize("form,model", [("ambient", "ckh"), ("jl3", "jl3")])
def test_step2_emulation_on_the_edge_graph(robust, form, model):
    prob = _edge_h(robust)
    top = 0.0
    for x in _terms_h(prob)[:-1]:
        t_ref, bound = RB.evaluate_joint(prob, x, RB.MODELS_H[model])
        t = RB.emulate_joint(prob, x, form)
        worst, i, n_over = RB.check(t, t_ref, bound)
        assert n_over == 0, (worst, i)
        assert np.all(t[-11:] == 0) and np.all(bound[-11:] == 0)  # (the camera without observations)
        top = max(top, worst)
    print(f"E0HBOUND emulation {form} {robust} err/bound={top:.3g}")
    assert top > 1e-4  # (not vacuous)


def _violates_h(prob, x, t_bad, model="ckh"):
    t_ref, bound = RB.evaluate_joint(prob, x, RB.MODELS_H[model])
    return RB.check(t_bad, t_ref, bound)[2] > 0


def _tail(prob, which=0):
    return int(np.flatnonzero(prob.n_c == 1)[which])


def test_step2_mutation_dropped_observation_of_a_one_observation_camera():
    prob = _edge_h("NONE")
    x = _terms_h(prob, 1)[1]
    i = int(np.flatnonzero(prob.cam_idx == _tail(prob))[0])

    def drop(sw):
        sw = sw.copy()
        sw[i] = 0
        return sw
    assert _violates_h(prob, x, RB.evaluate_joint(prob, x, mutate={"sw": drop})[0])


def test_step2_mutation_perturbed_landmark_block():
    prob = _edge_h("NONE")
    x = _terms_h(prob, 1)[1]
    lm = int(np.argmax(prob.n_l))

    def pert(hi):
        hi = hi.copy()
        hi[lm] *= 1 + 2.0 ** -20
        return hi
    assert _violates_h(prob, x, RB.evaluate_joint(prob, x, mutate={"hi": pert})[0])


def test_step2_mutation_house4_sign_taken_the_wrong_way():
    prob = _edge_h("NONE")
    x = _terms_h(prob, 1)[1]
    lm = int(np.flatnonzero(prob.lms[:, 0] < 0)[0])

    def flip(sign):
        sign = sign.copy()
        sign[lm] = -sign[lm]
        return sign
    assert _violates_h(prob, x, RB.evaluate_joint(prob, x, mutate={"sign": flip})[0])


def test_step2_mutation_sqrt_weight_applied_once():
    prob = _edge_h("HUBER")
    x = _terms_h(prob, 1)[1]
    assert _violates_h(prob, x, RB.evaluate_joint(prob, x, mutate={"sw2": np.ones_like})[0])


def test_step2_mutation_scaled_tail_camera_block():
    """At the damping 1 (the upper end of what the outer loop reaches).  At lambda = 1e-4 a one- or two-observation camera's
    B^-1 has entries near 1 / lambda and |B^-1| |y11| is 1e6 to 1e7 times |B^-1 y11|: fp64 may move such a block by more than
    1e-9 of itself (its bound is 2e-8 of the entry at best on this graph), so a factor 1 + 1e-9 is no defect there; at
    lambda = 1 every tail camera's bound is below 2e-10 of its entries and the factor is reported."""
    n_c, lm_off, cam_idx, obs, cams, X = RB.edge_problem_joint(0)
    prob = RB.system_joint(n_c, lm_off, cam_idx, obs, cams, X, 1.0)
    x = _terms_h(prob, 1)[1]
    t_bad = RB.evaluate_joint(prob, x)[0].copy()
    cam = _tail(prob, -1)
    t_bad[11 * cam:11 * cam + 11] *= 1 + np.longdouble(1e-9)
    assert _violates_h(prob, x, t_bad)


def test_step2_mutation_stale_z_of_a_tail_camera():
    """A tail camera's z = sigma N_c x left over from the previous term."""
    prob = _edge_h("NONE")
    ts = _terms_h(prob, 2)
    cam = _tail(prob, 1)
    z_prev = RB.evaluate_joint(prob, ts[1], want_parts=True)[2]["z"]

    def stale(z):
        z = z.copy()
        z[cam] = z_prev[cam]
        return z
    assert _violates_h(prob, ts[2], RB.evaluate_joint(prob, ts[2], mutate={"z": stale})[0])
