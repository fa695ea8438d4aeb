"""POVAR_FLAG_FP32_TERMS -- step 1's power-series terms in single precision (e0_ck_f32, povar_kernels_ck_f32.hpp; the numerical
contract is stated at the flag in include/povar_hip.h) -- against the oracle and the fp64 path at the same linearisation point.

Tolerances (relative 2-norms), derived before any run, not fitted to one:
  * fp32 unit roundoff u = 2^-24 = 6.0e-8, one ulp = 2^-23 = 1.2e-7.  One application of E0 to a camera vector is, per
    observation, a chain of about 40 dependent fp32 operations (Z h~ and its weighting: ~12, P3^T: ~6, G u: ~6 on a landmark sum of
    tens of fp32 adds, P3 g and the weighting: ~12) on fp32-rounded operands (Z, P3, h~, G, the image point: five more roundings);
    the landmark sums and the within-chunk sums (<= 16 observations) add a few more.  Everything summed across chunks of a camera
    is fp64.  So the relative error of one application is a few tens of u in the worst case and grows like sqrt(n) on average:
    the bound of about 80 ulp of fp32 is 80 * 1.2e-7 = 9.5e-6, i.e. 1e-5, for E0 x and for one term (B^-1 is fp64).
  * The 20-term increment: every term carries the error of its own E0 application; the series is a contraction (spectral
    radius < 1), so the errors of the terms do not compound beyond the same 1e-5 in the running sum.
  * The graph path against the kernel-by-kernel path: the same kernels; they differ only in the arrival order of the LDS adds
    (fp32 adds on the landmark slots: a few u on a sum; ~1e-7), hence 1e-6.
  * Two shards against one context: the same kernels on different landmark sets; the shard sums are exchanged in fp64.  The
    difference is two rounding paths of the fp32 chain, each within the 1e-5 of the first bullet: 1e-5.

Measured on one MI355X (profiles/fp32_terms_*): the 20-term increments meet the bound everywhere but HUBER under
POWER_VARPROJ on the 257-camera problem (4.6e-5), and E0 x of a RANDOM vector misses it from trafalgar-257 on (3.1e-5 to
5.6e-5; ladybug-49 meets it).  Those cases (and one term of the term-by-term test, 1.14e-5) are strict xfails with the measured number: the bound stays what was derived above
(the derivation leaves out how the 3x3 landmark blocks' conditioning amplifies the fp32 error of u = Jl^T Jp x through
g = G u), and a run that meets it turns the xfail into a failure to be looked at.

The pass/fail criterion for those cases is tests/test_gpu_e0_bounds.py: every output entry of e0_ck_f32 within a
componentwise rounding-error bound (tests/rounding_bounds.py) that scales with |G| |u| and with the HUBER weight's
cancellation.  Measured on one MI355X: largest err / bound 0.005 (trafalgar-257, every norm), 0.009 (local-900), 0.0069
(venice-1778), 0.036 on the edge graph, and 0.0012 to 0.0027 for the terms of the p257 problem (HUBER under POWER_VARPROJ
included).  Against a long-double reference built from the context's OWN Hll^-1 the normwise error of E0 x is 5.8e-6
(trafalgar-257) and 3.5e-5 (venice-1778): the misses above come from the conditioning, not from a defect of the kernel.
"""
import os
import threading

import numpy as np
import pytest

from conftest import rel

pytestmark = pytest.mark.gpu
ALPHA, LAM, M = 0.01, 1e-4, 20
NT = min(os.cpu_count() or 1, 16)
TOL = 1e-5


def _problem(name):
    from povar_amd import synth
    if name == "local-900":
        return synth.make_problem(900, 40000, 200000, seed=9, popularity="local")
    if name == "p257":
        return synth.make_problem(257, 12000, 60000, seed=4)
    return synth.make_bal_problem(name)


def _ctx(p, fp32, robust="NONE", flags=0, obs=None):
    from povar_amd import capi
    return capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs if obs is None else obs, robust_norm=robust, huber=1.0,
                        e0_mode=capi.E0_IMPLICIT_LDSACC, flags=flags | (capi.FLAG_FP32_TERMS if fp32 else 0))


def _linearized(p, fp32, robust="NONE", flags=0, lms=None):
    ctx = _ctx(p, fp32, robust, flags)
    ctx.set_cameras(p.cams)
    if lms is None:
        ctx.init_landmarks_pose(ALPHA)
    else:
        ctx.set_landmarks(lms)
    assert ctx.linearize_pose(ALPHA)
    return ctx


def _e0_miss(name, measured):
    return pytest.param(name, marks=pytest.mark.xfail(strict=True, reason=f"E0 x of a random vector: {measured} measured against "
                                                       f"the derived 1e-5 (module docstring)"))


@pytest.mark.parametrize("name", ["ladybug-49", "trafalgar-257", "local-900", "venice-1778"])
def test_fp32_terms_against_oracle_at_size(name):
    """The layout flag, the 20-term increment against the oracle and against the fp64 path."""
    from povar_amd import capi
    from oracle import povar_oracle as O
    p = _problem(name)
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    lms = orc.init_landmarks_pose(ALPHA, p.cams)
    st, diag2, jls, sigma, ok = orc.stage1_pose(ALPHA, p.cams, lms)
    assert ok
    orc.scale_jp_cols_pose(st, sigma)
    hll, b, binv = orc.prepare_hb_pose(st, LAM)
    ref, it, status, _ = orc.solve_pose(st, hll, binv, b, M, n_threads=NT)
    del st

    ctx = _linearized(p, True, lms=lms)
    li = ctx.layout_info()
    assert li.ck_ready == 1 and li.lane_per_landmark == 1 and li.placement == 1
    inc, it2, st2, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
    assert ctx.layout_info().fp32_terms == 1
    assert rc == 0 and it2 == M
    assert rel(inc, ref) <= TOL, rel(inc, ref)
    ctx.close()

    c64 = _linearized(p, False, lms=lms)
    inc64, _, _, _ = c64.solve_pose(LAM, capi.POWER_VARPROJ, M)
    assert c64.layout_info().fp32_terms == 0
    c64.close()
    assert rel(inc, inc64) <= TOL


@pytest.mark.parametrize("name", ["ladybug-49", _e0_miss("trafalgar-257", "3.7e-5"), _e0_miss("local-900", "3.1e-5"),
                                  _e0_miss("venice-1778", "5.6e-5")])
def test_fp32_e0_against_oracle_at_size(name):
    """right_mul_e0_pose of a random vector on an fp32 context against the oracle (the E0 application of the terms)."""
    from povar_amd import capi
    from oracle import povar_oracle as O
    p = _problem(name)
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    lms = orc.init_landmarks_pose(ALPHA, p.cams)
    st, diag2, jls, sigma, ok = orc.stage1_pose(ALPHA, p.cams, lms)
    assert ok
    orc.scale_jp_cols_pose(st, sigma)
    hll, b, binv = orc.prepare_hb_pose(st, LAM)
    x = np.random.default_rng(5).normal(size=12 * p.n_cams)
    e0_ref = orc.right_mul_e0_pose(st, hll, x, n_threads=NT)
    del st
    ctx = _linearized(p, True, lms=lms)
    ctx.prepare_pose(LAM)
    y = ctx.right_mul_e0_pose(x)
    ctx.close()
    assert rel(y, e0_ref) <= TOL, rel(y, e0_ref)


@pytest.mark.xfail(strict=True, reason="a term 1.14e-5 from the fp64 path's within the first five on trafalgar-257, against the "
                                      "derived 1e-5 (module docstring)")
def test_single_terms_against_fp64():
    """povar_power_series_begin / _step / get_term: the first terms of the fp32 loop against the fp64 path's, term by term
    (each loop continues from its own previous term: a contraction, so the error stays that of one application)."""
    from povar_amd import capi
    p = _problem("trafalgar-257")
    c32, c64 = _linearized(p, True), _linearized(p, False)
    for c in (c32, c64):
        c.prepare_pose(LAM)
        c.power_series_begin()
    # B^-1 (-b): fp64 on both; the two contexts' rows are in different orders and b's sums land in arrival order
    assert rel(c32.get_term(), c64.get_term()) <= 1e-13
    for _ in range(5):
        c32.power_series_step()
        c64.power_series_step()
        t32, t64 = c32.get_term(), c64.get_term()
        assert rel(t32, t64) <= TOL
    assert c32.layout_info().fp32_terms == 1
    c32.close()
    c64.close()


@pytest.mark.parametrize("robust,solver", [(r, s) for r in ("NONE", "HUBER", "CAUCHY") for s in ("POWER_VARPROJ", "POWER_SCHUR_COMPLEMENT")
                                           if (r, s) != ("HUBER", "POWER_VARPROJ")] +
                         [pytest.param("HUBER", "POWER_VARPROJ", marks=pytest.mark.xfail(
                             strict=True, reason="4.6e-5 measured against the derived 1e-5 (module docstring)"))])
def test_increment_every_norm(robust, solver):
    from povar_amd import capi
    st = capi.POWER_VARPROJ if solver == "POWER_VARPROJ" else capi.POWER_SCHUR_COMPLEMENT
    p = _problem("p257")
    out = []
    for fp32 in (True, False):
        c = _linearized(p, fp32, robust)
        inc, it, status, rc = c.solve_pose(LAM, st, M)
        assert rc == 0 and it == M
        assert c.layout_info().fp32_terms == (1 if fp32 else 0)
        out.append(inc)
        c.close()
    assert rel(out[0], out[1]) <= TOL, rel(out[0], out[1])


def test_early_exit_term_count():
    """r_tolerance ends the series on the device (series_check).  The term norms of the two paths differ by about 1e-5
    relative (above), so a threshold crossing can move by one term where a norm lies that close to r_tol -- not more:
    consecutive term norms of the series differ by far more than 1e-5 (the contraction factor is not within 1e-5 of 1)."""
    from povar_amd import capi
    p = _problem("p257")
    its = []
    for fp32 in (True, False):
        c = _linearized(p, fp32)
        inc, it, status, rc = c.solve_pose(LAM, capi.POWER_VARPROJ, 200, 0.0, 1e-3)
        assert rc == 0 and status == 1 and it < 200  # (POVAR_LINEAR_SOLVER_SUCCESS)
        its.append(it)
        c.close()
    assert abs(its[0] - its[1]) <= 1, its


def test_graph_and_no_graph_agree():
    """The captured hipGraph and the kernel-by-kernel launches run the same kernels; the fp32 LDS adds land in arrival order
    (not bit-reproducible, as the default mode), so the two agree to rounding: 1e-6."""
    from povar_amd import capi
    p = _problem("p257")
    out = []
    for flags in (0, capi.FLAG_NO_GRAPH):
        c = _linearized(p, True, flags=flags)
        inc, it, status, rc = c.solve_pose(LAM, capi.POWER_VARPROJ, M, 0.0, 1e-9)
        assert rc == 0 and c.layout_info().fp32_terms == 1
        out.append((inc, it))
        c.close()
    assert out[0][1] == out[1][1]
    assert rel(out[0][0], out[1][0]) <= 1e-6


class HostAllReduce:
    def __init__(self, world):
        self.world, self.bar = world, threading.Barrier(world)
        self.bufs = [None] * world

    def fn(self, rank):
        def f(buf):
            self.bufs[rank] = buf.copy()
            self.bar.wait()
            tot = sum(self.bufs[r] for r in range(self.world))
            self.bar.wait()
            buf[:] = tot
        return f


def test_two_shards_against_one_context():
    """Two in-process landmark shards on one device (the exchange in fp64 through the host all-reduce hook) against one fp32
    context of the whole problem."""
    from povar_amd import capi
    p = _problem("p257")
    c = _linearized(p, True)
    ref, _, _, rc = c.solve_pose(LAM, capi.POWER_VARPROJ, M)
    assert rc == 0
    c.close()
    world = 2
    ar = HostAllReduce(world)
    out = [None] * world

    def worker(rank):
        lb, le = capi.shard_range(p.lm_off, world, rank)
        ob, oe = int(p.lm_off[lb]), int(p.lm_off[le])
        ctx = capi.Context(p.n_cams, p.lm_off[lb:le + 1] - p.lm_off[lb], p.cam_idx[ob:oe], p.obs[ob:oe],
                           e0_mode=capi.E0_IMPLICIT_LDSACC, flags=capi.FLAG_FP32_TERMS)
        ctx.comm_init_host(world, rank, ar.fn(rank))
        ctx.set_cameras(p.cams)
        ctx.init_landmarks_pose(ALPHA)
        ok = ctx.linearize_pose(ALPHA)
        inc, it, st, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
        out[rank] = dict(ok=ok, inc=inc, rc=rc, fp32=ctx.layout_info().fp32_terms)
        ctx.close()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=300) for t in th]
    assert all(o is not None for o in out)
    for o in out:
        assert o["ok"] and o["rc"] == 0 and o["fp32"] == 1
        assert np.array_equal(o["inc"], out[0]["inc"])
        assert rel(o["inc"], ref) <= TOL, rel(o["inc"], ref)


def test_step2_unchanged_by_the_flag():
    """Step 2 (RIPOBA) is out of the mode: with the flag it runs the kernels it runs without (forced to the same one: the timing
    that picks it otherwise could decide differently in two contexts), and its increment is the flag-off one to the rounding
    of those kernels.  Not bit for bit: e0_ck_h adds in LDS in arrival order, so two flag-OFF contexts already differ (1.1e-13
    measured on this problem); 1e-11 is the reduction-order tolerance of the sharded tests (test_gpu_sharded.py)."""
    from povar_amd import capi
    p = _problem("trafalgar-257")  # (the flag-off context builds the chunk layout from 65 536 observations on)
    rng = np.random.default_rng(11)
    cams = np.concatenate([rng.normal(size=(p.n_cams, 8)), rng.normal(size=(p.n_cams, 4))], 1)
    cams[:, 11] = 5 + rng.random(p.n_cams)
    cams /= np.linalg.norm(cams, axis=1, keepdims=True)
    lms_h = np.concatenate([rng.normal(size=(p.n_lms, 3)), np.ones((p.n_lms, 1))], 1)
    obs = p.obs / 500.0
    out = []
    kernels = []
    for fp32 in (True, False):
        c = _ctx(p, fp32, obs=obs)
        c.set_e0_kernel(1)
        c.set_cameras(cams)
        c.set_landmarks_homogeneous(lms_h)
        assert c.linearize_homogeneous()
        inc, it, st, rc = c.solve_joint(LAM, M)
        assert rc == 0
        out.append(inc)
        kernels.append(c.layout_info().e0_kernel_h)
        c.close()
    assert kernels[0] == kernels[1] == 1
    assert rel(out[0], out[1]) <= 1e-11, rel(out[0], out[1])


@pytest.mark.parametrize("extra,what", [("det", "DETERMINISTIC"), ("res", "SERIES_KERNEL"), ("lpl", "E0_KERNEL"),
                                        ("mode", "E0 mode")])
def test_refused_combinations(extra, what):
    from povar_amd import capi
    p = _problem("ladybug-49")
    flags = {"det": capi.FLAG_DETERMINISTIC, "res": capi.flag_series_kernel(1), "lpl": capi.flag_e0_kernel(0), "mode": 0}[extra]
    e0_mode = capi.E0_IMPLICIT if extra == "mode" else capi.E0_IMPLICIT_LDSACC
    with pytest.raises(Exception) as ei:
        capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, e0_mode=e0_mode, flags=capi.FLAG_FP32_TERMS | flags)
    assert "FP32_TERMS" in str(ei.value) and what in str(ei.value)


def test_setters_that_would_leave_the_mode_are_refused():
    from povar_amd import capi
    p = _problem("ladybug-49")
    c = _linearized(p, True)
    for call in (lambda: c.set_e0_kernel(0), lambda: c.set_e0_mode(capi.E0_IMPLICIT)):
        with pytest.raises(Exception):
            call()
    c.set_e0_kernel(-1)  # (step 2's choice back to the library; step 1 stays on the fp32 kernel)
    inc, it, st, rc = c.solve_pose(LAM, capi.POWER_VARPROJ, M)
    assert rc == 0 and c.layout_info().fp32_terms == 1
    c.close()


# ---- known answer: bin/bal --fp32-terms on the POWER_VARPROJ / RIPOBA configurations of test_known_answer.py
def _ka_params():
    from test_known_answer import KNOWN_ANSWER
    return [pa for pa in KNOWN_ANSWER if "POWER_VARPROJ" in pa.values[2] and "RIPOBA" in pa.values[2]]


@pytest.mark.parametrize("shape,seed,flags", _ka_params())
def test_bal_fp32_terms_reaches_noise_floor(tmp_path, shape, seed, flags):
    from test_known_answer import COMMON, check_floor, run_bal, write_problem
    p, f = write_problem(tmp_path, shape, seed)
    res = run_bal("bin/bal", f, str(tmp_path / "log.json"), flags + COMMON + ["--fp32-terms", "--quiet"])
    check_floor(p, res)
