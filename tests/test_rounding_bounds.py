"""The componentwise bound of tests/rounding_bounds.py checked on the CPU: its long-double reference against exact rational
arithmetic, NumPy emulations of the fp64 and fp32 kernels within their bounds, and deliberate defects reported as violations
(the bound is sharp, not vacuous).

Slack measured when these tests were written (largest err / bound over every output entry):
  * the long-double reference against the exact E0 x of the golden problem: below 0.05;
  * on the edge graph (rounding_bounds.edge_problem: hubs, one- and two-observation cameras, long landmarks, cond(Hll) above
    1e6, |u| above 16.78, packed and unpacked points), x ~ N(0, 1) and per-camera scales 10^U(-4, 4):
      fp64 emulation / fp64 bound  0.019 (NONE), 0.041 (HUBER);   fp32 emulation / fp32 bound  0.017 (NONE), 0.023 (HUBER);
    and the fp32 emulation exceeds the fp64 bound by 1e7 (the two bounds are far apart, as they should be).
    The MI355X kernels reach 0.001 to 0.048 of their bounds (tests/test_gpu_e0_bounds.py): the same slack as the emulations.
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
