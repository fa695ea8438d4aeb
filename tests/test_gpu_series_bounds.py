"""Whole power-series launches held to the componentwise identity of tests/series_bounds.py: from the final state of ONE
launch of k terms (x_0 from power_series_begin, the last term x_k and the sum S_k),

    R = (S_k - x_0) - T_ref(S_k) + T_ref(x_k),      |R_i| <= bound_i for EVERY entry

with the long-double reference and the bound built from the context's own operands.  The relative 2-norms of
test_gpu_res.py, test_gpu_res_shapes.py and test_gpu_res_joint.py hold the 20-term increment to 1e-10; the first-term test of
test_gpu_res_joint.py holds term 1 componentwise, the one term before any in-launch hand-over.  Here every term's error enters
R undamped, so what is specific to a resident launch (series_res / series_res_h, povar_kernels_res.hpp) -- z of term i
replacing z of term i - 1, records of term i + 1 replacing those of term i, the parity halves of the norm granules reused from
term 3 on, the landmark sums re-zeroed, the region changing roles -- is checked entry by entry for a one-observation camera
as hard as for a hub, and so is the replayed hipGraph of per-term kernels behind solve_pose(m) / solve_joint(m).

Cases: the edge graphs of both steps plus an unobserved camera (NONE, HUBER, CAUCHY; eight workgroups and the library's own
count; k = 1, 2, 3, 5, 8: each overwrite rule and each parity half used at least twice -- tests/test_series_bounds.py finds
every injected defect at k = 8, so 8 stays the largest); the seven instantiations of test_gpu_res_shapes.py; the norm sweep
on without convergence; an early exit by q_tolerance and by r_tolerance placed between two consecutive values of the
reference's test quantity; the per-term graph of e0_lpl, e0_ck, e0_lpl_h and e0_ck_h; a second launch on the same context.
Every resident case forces the kernel itself (set_series_kernel(1)) and asserts that the launch did not give up.

POVAR_DETERMINISTIC=1 in the environment pins the per-term kernels: the resident cases skip (and the graph cases of the other
families, as in test_gpu_e0_bounds.py); POVAR_RES_WGS from tools/forced_mode_suite.sh may leave no layout for the cases that
do not set it themselves: they skip as test_gpu_res.py does.
"""
import os

import numpy as np
import pytest

import rounding_bounds as RB
import series_bounds as SB
import test_gpu_e0_bounds as E0
import test_gpu_e0h_bounds as E0H
import test_gpu_res_shapes as SHAPES

pytestmark = pytest.mark.gpu
ALPHA, LAM = 0.01, 1e-4
KS = (1, 2, 3, 5, 8)
DET_ENV = os.environ.get("POVAR_DETERMINISTIC") == "1"
_EDGE = {}


def _edge(step):
    """(n_cams, lm_off, cam_idx, obs, cams, landmarks or None) of the step's edge graph; the last camera has no observation."""
    if step not in _EDGE:
        if step == 1:
            n_c, lm_off, cam_idx, obs, cams, _ = RB.edge_problem(0)
            _EDGE[step] = (n_c + 1, lm_off, cam_idx, obs, np.concatenate([cams, cams[:1] + 0.5], 0), None)
        else:
            _EDGE[step] = RB.edge_problem_joint(0)
    return _EDGE[step]


def _resident_context(monkeypatch, step, robust, wgs="keep"):
    """A prepared context of the step's edge graph in the LDS-accumulating E0 mode; wgs: POVAR_RES_WGS ("keep": the environment's)."""
    from povar_amd import capi
    if DET_ENV:
        pytest.skip("POVAR_DETERMINISTIC=1 pins the per-term kernels: no resident series")
    if wgs is None:
        monkeypatch.delenv("POVAR_RES_WGS", raising=False)
    elif wgs != "keep":
        monkeypatch.setenv("POVAR_RES_WGS", wgs)
    n_c, lm_off, cam_idx, obs, cams, lms_h = _edge(step)
    huber = RB.EDGE_HUBER if step == 1 else RB.EDGE_HUBER_H
    ctx = capi.Context(n_c, lm_off, cam_idx, obs, robust_norm=robust, huber=huber, e0_mode=capi.E0_IMPLICIT_LDSACC)
    ctx.layout_finalize(True)
    ctx.set_cameras(cams)
    if step == 1:
        ctx.init_landmarks_pose(ALPHA)
        assert ctx.linearize_pose(ALPHA)
        ctx.prepare_pose(LAM)
    else:
        ctx.set_landmarks_homogeneous(lms_h)
        assert ctx.linearize_homogeneous()
        ctx.prepare_joint(RB.EDGE_LAM_H)
    li = ctx.layout_info()
    ready, n_wg = (li.res_ready, li.res_wgs) if step == 1 else (li.res_ready_h, li.res_wgs_h)
    if ready != 1 and wgs == "keep" and os.environ.get("POVAR_RES_WGS") is not None:
        pytest.skip("POVAR_RES_WGS leaves no layout at this size")
    assert ready == 1 and n_wg >= 1 and (wgs in (None, "keep") or n_wg <= int(wgs)), "the resident layout must exist for the edge graph"
    return ctx, _operands(ctx, step, obs, robust, huber), n_wg


def _operands(ctx, step, obs, robust, huber):
    """(Step1 | Step2 of the context, step 1's B^-1 or None)."""
    from povar_amd import capi
    if step == 1:
        return RB.Step1.from_context(ctx, obs, ALPHA, robust, huber), ctx.get_buffer(capi.BUF_B_INV).reshape(-1, 12, 12)
    return RB.Step2.from_context(ctx, obs, robust, huber), None


class _Series:
    """The launches of one prepared context against the identity; the reference series is built once per x_0."""

    def __init__(self, ctx, step, operands, model, label, unobserved=None):
        self.ctx, self.step, (self.prob, self.binv), self.model, self.label = ctx, step, operands, model, label
        self.unobserved, self.refs, self.worst = unobserved, {}, 0.0

    def reference(self, x0, m=max(KS)):
        key = x0.tobytes()
        if key not in self.refs:
            self.refs[key] = SB.reference_series(self.prob, self.binv, x0, m, self.model)
        return self.refs[key]

    def begin(self):
        self.ctx.power_series_begin()
        return self.ctx.get_term(SB.dim(self.prob))

    def launch(self, k, kernel, q_tol=0.0, r_tol=-1.0, expect=None, what=""):
        """power_series_begin, one launch of k terms with series kernel `kernel` (1: resident, 0: the per-term graph), the
        identity over the terms it ran; expect: (iterations, status) where the tolerances are on.  Returns |R| / bound."""
        ctx, D = self.ctx, SB.dim(self.prob)
        x0 = self.begin()
        ctx.set_series_kernel(kernel)
        li = ctx.layout_info()
        assert (li.res_active if self.step == 1 else li.res_active_h) == kernel
        it, st = ctx.power_series_pose(k, q_tol, r_tol)
        xk, Sk = ctx.get_term(D), ctx.get_increment(D)
        assert ctx.layout_info().res_failed == 0, "the resident launch gave up: the per-term kernels computed this series"
        if expect is not None:
            assert (it, st) == expect, (self.label, what, it, st, expect)
        else:
            assert it == k
        ref = self.reference(x0)
        R, bound = SB.launch_identity(self.prob, self.binv, x0, xk, Sk, it, self.model, ref=ref)
        r, j, n_over = SB.check(R, bound)
        print(f"SERIESBOUND {self.label} {'series_res' if kernel else 'per-term graph'}{what} k={k} ran={it} |R|/bound={r:.3g} over={n_over}")
        assert np.all(np.isfinite(xk)) and np.all(np.isfinite(Sk))
        assert n_over == 0, (self.label, what, k, r, j // D, j % D, float(R[j]), float(bound[j]))
        if self.unobserved is not None:  # (no observation: every term after x_0 is exactly 0, the sum is x_0's bits)
            c = self.unobserved
            assert np.all(xk[D * c:D * c + D] == 0.0) and np.array_equal(Sk[D * c:D * c + D], x0[D * c:D * c + D])
        self.worst = max(self.worst, r)
        return r


# ---- the edge graphs through the resident series
@pytest.mark.parametrize("wgs", ["8", None])
@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
@pytest.mark.parametrize("step", [1, 2])
def test_resident_launches_on_the_edge_graph(monkeypatch, step, robust, wgs):
    """k = 1, 2, 3, 5, 8 on one prepared context: over eight workgroups (most cameras have records from several of them)
    and over the library's own count (most workgroups own few cameras)."""
    ctx, operands, n_wg = _resident_context(monkeypatch, step, robust, wgs)
    s = _Series(ctx, step, operands, SB.resident_model(operands[0]), f"edge/step{step}/{robust}/res_wgs={wgs or 'default'}({n_wg})",
                unobserved=ctx.n_cams - 1)
    for k in KS:
        s.launch(k, 1)
    assert s.worst > 1e-6  # (not vacuous)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_resident_launch_cauchy(monkeypatch, step):
    ctx, operands, n_wg = _resident_context(monkeypatch, step, "CAUCHY", None)
    _Series(ctx, step, operands, SB.resident_model(operands[0]), f"edge/step{step}/CAUCHY/res_wgs=default({n_wg})", ctx.n_cams - 1).launch(5, 1)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_resident_second_launch_on_the_same_context(monkeypatch, step):
    """The second launch replays the captured one; the launch counter has advanced the granule tags."""
    ctx, operands, n_wg = _resident_context(monkeypatch, step, "HUBER")
    s = _Series(ctx, step, operands, SB.resident_model(operands[0]), f"edge/step{step}/HUBER/res_wgs=env({n_wg})", ctx.n_cams - 1)
    for rep in (1, 2, 3):
        s.launch(5, 1, what=f" launch {rep}")
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_resident_launch_with_the_norm_sweep_on(monkeypatch, step):
    """Tolerances of 1e-30: every term publishes and sweeps the norm granules (both parity halves, reused from term 3 on) and
    none converges."""
    from povar_amd import capi
    ctx, operands, n_wg = _resident_context(monkeypatch, step, "NONE")
    s = _Series(ctx, step, operands, SB.resident_model(operands[0]), f"edge/step{step}/NONE/res_wgs=env({n_wg})", ctx.n_cams - 1)
    for k in (5, 8):
        s.launch(k, 1, q_tol=1e-30, r_tol=1e-30, expect=(k, capi.NO_CONVERGENCE), what=" norms on")
    ctx.close()


def _between(values, m):
    """(tolerance, iterations): the geometric mean of low = min(values[1 .. j]) and values[j + 1] < low, so that the loop's
    first value under the tolerance is values[j + 1] -- for the LAST j + 1 < m whose gap low / values[j + 1] is at least 1.05
    (the device's norms agree with the reference's to some 1e-13: the decision has a margin of 2.5 % either way)."""
    best = None
    for j in range(1, m - 1):
        low = float(np.min(values[1:j + 1]))
        if low / values[j + 1] >= 1.05:
            best = (float(np.sqrt(low * values[j + 1])), j + 1)
    assert best is not None, "no two consecutive values to put a tolerance between"
    return best


@pytest.mark.parametrize("step", [1, 2])
def test_resident_launch_early_exit(monkeypatch, step):
    """q_tolerance, then r_tolerance, each the geometric mean of two consecutive values of the reference's test quantity
    (i |x_i| / |S_i|, |x_i| / |x_0|: oracle/povar_oracle.c, LPV:206-229): iterations and status are the reference's, and the
    identity holds over the terms that ran."""
    from povar_amd import capi
    ctx, operands, n_wg = _resident_context(monkeypatch, step, "NONE")
    s = _Series(ctx, step, operands, SB.resident_model(operands[0]), f"edge/step{step}/NONE/res_wgs=env({n_wg})", ctx.n_cams - 1)
    m = max(KS)
    ref = s.reference(s.begin())
    q_tol, it_q = _between(ref["zeta"], m)
    r_tol, it_r = _between(ref["rel"], m)
    assert SB.expected_exit(ref, m, q_tol, -1.0) == (it_q, True) and SB.expected_exit(ref, m, 0.0, r_tol) == (it_r, True)
    s.launch(m, 1, q_tol=q_tol, r_tol=-1.0, expect=(it_q, capi.SUCCESS), what=f" q_tol={q_tol:.3g}")
    s.launch(m, 1, q_tol=0.0, r_tol=r_tol, expect=(it_r, capi.SUCCESS), what=f" r_tol={r_tol:.3g}")
    ctx.close()


# ---- the instantiations of test_gpu_res_shapes.py on ladybug-49
@pytest.mark.parametrize("step, wgs, shape", [(1, 32, (16, 1, 1)), (1, 16, (16, 2, 1)), (1, 8, (8, 4, 2)),
                                              (2, 32, (8, 1, 2)), (2, 30, (8, 2, 2)), (2, 16, (8, 2, 2)), (2, 8, (8, 4, 2))])
def test_resident_launch_shapes(monkeypatch, step, wgs, shape):
    """shape = (wavefronts per workgroup, rows per chunk, chunks per lane) as in test_gpu_res_shapes.py: the case asserts the
    instantiation it meant to reach."""
    if DET_ENV:
        pytest.skip("POVAR_DETERMINISTIC=1 pins the per-term kernels: no resident series")
    for name in ("POVAR_RES", "POVAR_RES_MAX_OBS", "POVAR_RES_OBS_PER_WG", "POVAR_RES_SPIN"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("POVAR_RES_WGS", str(wgs))
    ctx, _ = SHAPES._context(step, "NONE")
    li = ctx.layout_info()
    if step == 1:
        ready, n_wg, got = li.res_ready, li.res_wgs, (li.res_waves, li.res_rows, li.res_rounds)
        ctx.prepare_pose(LAM)
        obs = SHAPES._state()[0].obs
    else:
        ready, n_wg, got = li.res_ready_h, li.res_wgs_h, (li.res_waves_h, li.res_rows_h, li.res_rounds_h)
        ctx.prepare_joint(LAM)
        obs = SHAPES._state()[1][2]
    assert ready == 1 and 1 <= n_wg <= wgs and got == shape, (ready, n_wg, got, shape)
    operands = _operands(ctx, step, obs, "NONE", 1.0)
    _Series(ctx, step, operands, SB.resident_model(operands[0]), f"ladybug-49/step{step}/NONE/<NW,H,RR>={shape}({n_wg})").launch(5, 1)
    ctx.close()


# ---- the replayed graph of per-term kernels
@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
@pytest.mark.parametrize("fam", ["e0_lpl", "e0_ck"])
def test_per_term_graph_step1(monkeypatch, fam, robust):
    """solve_pose's graph of eight terms (E0 kernel, per-camera step) with the family forced as in test_gpu_e0_bounds.py."""
    n_c, lm_off, cam_idx, obs, cams, _ = _edge(1)
    ctx = E0._context(monkeypatch, fam, n_c, lm_off, cam_idx, obs, cams, robust=robust, huber=RB.EDGE_HUBER)
    operands = _operands(ctx, 1, obs, robust, RB.EDGE_HUBER)
    s = _Series(ctx, 1, operands, RB.MODELS[E0.FAMILIES[fam][3]], f"edge/step1/{robust}/{fam}", n_c - 1)
    for rep in (1, 2):
        s.launch(8, 0, what=f" launch {rep}")
    li = ctx.layout_info()
    assert li.lane_per_landmark == 1 and li.e0_kernel == (0 if fam == "e0_lpl" else 1), (li.lane_per_landmark, li.e0_kernel)
    ctx.close()


@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
@pytest.mark.parametrize("fam", ["e0_lpl_h", "e0_ck_h"])
def test_per_term_graph_step2(monkeypatch, fam, robust):
    """solve_joint's graph of eight terms with the family forced as in test_gpu_e0h_bounds.py."""
    n_c, lm_off, cam_idx, obs, cams, lms_h = _edge(2)
    ctx = E0H._context(monkeypatch, fam, n_c, lm_off, cam_idx, obs, cams, lms_h, robust, RB.EDGE_HUBER_H)
    assert E0H.LAM == RB.EDGE_LAM_H
    operands = _operands(ctx, 2, obs, robust, RB.EDGE_HUBER_H)
    s = _Series(ctx, 2, operands, RB.MODELS_H[E0H.FAMILIES[fam][5]], f"edge/step2/{robust}/{fam}", n_c - 1)
    for rep in (1, 2):
        s.launch(8, 0, what=f" launch {rep}")
    E0H._ran(ctx, fam)
    ctx.close()
