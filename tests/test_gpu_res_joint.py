"""series_res_h -- the RESIDENT power series of step 2: the whole loop of solve_joint (sc/linearization_power_varproj.hpp:
240-287: x_0 = B^-1 (-b), x_i = B^-1 N_c^T sigma E0 sigma N_c x_{i-1}, early exit) as ONE launch (povar_kernels_res.hpp:
res_series with ResJoint; layout: res_layout.hpp, res_shape_step2()) -- against the CPU oracle at size, against the per-term kernels (e0_lpl_h /
e0_ck_h + cam_cold_sum_binv_h) with robust norms, early exit, m = 0 and m = 1, its first term componentwise against the
"ckh" rounding-error model, across linearisations, the library's own choice between the two forms, the give-up path, and a
term-by-term continuation.

State as test_step2_at_size (tests/test_gpu_baseline_sizes.py): rng 11, normalised cameras, X_w = 1, obs / 500.  Tolerances
as for the per-term kernels and series_res: 20-term increment 1e-10, last term 1e-9, relative 2-norms.
"""
import os

import numpy as np
import pytest

import rounding_bounds as RB
from conftest import rel

pytestmark = pytest.mark.gpu
if os.environ.get("POVAR_DETERMINISTIC") == "1":
    pytest.skip("POVAR_DETERMINISTIC=1 pins the per-term kernels: no resident series", allow_module_level=True)

LAM, M = 1e-4, 20
_STATE = {}


def _state(name):
    """(problem, cameras, homogeneous landmarks, observations) of test_step2_at_size; built once per problem."""
    from povar_amd import synth
    if name not in _STATE:
        _STATE.clear()
        p = synth.make_bal_problem(name)
        rng = np.random.default_rng(11)
        cams = rng.normal(size=(p.n_cams, 12))
        cams[:, 8:11] *= 0.1
        cams[:, 11] = 5 + rng.random(p.n_cams)
        cams /= np.linalg.norm(cams, axis=1, keepdims=True)
        lms_h = np.concatenate([rng.normal(size=(p.n_lms, 3)), np.ones((p.n_lms, 1))], 1)
        _STATE[name] = (p, cams, lms_h, p.obs / 500.0)
    return _STATE[name]


def _need_layout(li):
    """The step-2 instance exists at the sizes of this module -- unless the environment has cut the workgroups it may use
    (tools/forced_mode_suite.sh: POVAR_RES_WGS=7)."""
    if li.res_ready_h != 1 and os.environ.get("POVAR_RES_WGS") is not None:
        pytest.skip("POVAR_RES_WGS leaves no layout at this size")
    assert li.res_ready_h == 1 and li.res_wgs_h >= 1 and li.res_waves_h == 8, "the step-2 resident layout must exist at this size"
    assert 0 < li.res_lds_bytes_h <= 160 * 1024


def _ctx(name, robust="NONE", huber=1.0, linearize=True):
    from povar_amd import capi
    p, cams, lms_h, obs = _state(name)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs, robust_norm=robust, huber=huber, e0_mode=capi.E0_IMPLICIT_LDSACC)
    ctx.layout_finalize(True)
    ctx.set_cameras(cams)
    ctx.set_landmarks_homogeneous(lms_h)
    if linearize:
        assert ctx.linearize_homogeneous()
    return ctx


@pytest.mark.parametrize("name", ["ladybug-49", "trafalgar-257"])
def test_resident_joint_series_oracle_parity_at_size(name):
    """The 20-term increment and the twelfth term (get_term(11): the last term, eleven entries per camera) of the resident
    series against the oracle and against the per-term kernels of the same context; the second solve replays the graph.
    On the parent commit: no res_active_h (and with the field alone, 0)."""
    from oracle import povar_oracle as O
    p, cams, lms_h, obs = _state(name)
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, obs)
    ctx = _ctx(name)
    _need_layout(ctx.layout_info())
    st_h, ok = orc.linearize_homogeneous(cams, lms_h)
    diag2 = orc.jp_diag2_homogeneous(st_h)
    orc.scale_jl_cols_homogeneous(st_h)
    sigma = 1.0 / (1e-5 + np.sqrt(diag2))
    orc.scale_jp_cols_joint(st_h, sigma)
    st_n = orc.linearize_nullspace(cams, lms_h, st_h)
    hll, b, binv = orc.prepare_hb_joint(st_h, st_n, LAM)
    ref, it, status, _ = orc.solve_joint(st_n, hll, binv, b, M, want_terms=True)
    ctx.set_series_kernel(0)
    inc0, it0, st0, rc0 = ctx.solve_joint(LAM, M)
    term0 = ctx.get_term(11)
    assert rc0 == 0 and rel(inc0, ref) < 1e-10
    ctx.set_series_kernel(1)
    assert ctx.layout_info().res_active_h == 1
    for _ in range(2):
        inc, it2, st2, rc = ctx.solve_joint(LAM, M)
        assert rc == 0 and (it2, st2) == (it, status)
        assert rel(inc, ref) < 1e-10
        assert rel(inc, inc0) < 1e-10 and rel(ctx.get_term(11), term0) < 1e-9
    assert ctx.layout_info().res_failed == 0
    ctx.close()


@pytest.mark.parametrize("robust", ["NONE", "HUBER", "CAUCHY"])
def test_resident_joint_series_against_the_per_term_kernels(robust):
    """Every robust norm; fixed m, early exit by r_tolerance and by q_tolerance, m = 0 and m = 1: the same increment,
    iteration count and status as the per-term kernels."""
    ctx = _ctx("ladybug-49", robust)
    _need_layout(ctx.layout_info())
    cases = [dict(m=M), dict(m=M, q_tol=0.0, r_tol=1e-3), dict(m=M, q_tol=0.05, r_tol=-1.0), dict(m=40, q_tol=1e-3, r_tol=1e-6),
             dict(m=0), dict(m=1), dict(m=3, q_tol=0.5, r_tol=0.5)]
    ctx.set_series_kernel(0)
    want = [ctx.solve_joint(LAM, **kw) for kw in cases]
    ctx.set_series_kernel(1)
    assert ctx.layout_info().res_active_h == 1
    for kw, (inc0, it0, st0, rc0) in zip(cases, want):
        inc, it, st, rc = ctx.solve_joint(LAM, **kw)
        assert rc == rc0 == 0 and (it, st) == (it0, st0), (kw, it, st, it0, st0)
        assert rel(inc, inc0) < 1e-10, kw
    assert ctx.layout_info().res_failed == 0
    ctx.close()


_EDGE = []


@pytest.mark.parametrize("wgs", ["8", None])
@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
def test_resident_joint_first_term_componentwise(monkeypatch, robust, wgs):
    """The edge graph (151 cameras, one-observation cameras, one unobserved camera, both house4 branches, X_w != 1, small
    depths), far below the size where most workgroups have work -- once over eight workgroups, once over the library's own
    count.  The prologue's x_0 has the bits of povar_power_series_begin (inc == x_0 + t_1 exactly), every entry of the first
    term is within the "ckh" bound of the long-double operator applied to x_0, and the unobserved camera's block is 0."""
    from povar_amd import capi
    if wgs is None:
        monkeypatch.delenv("POVAR_RES_WGS", raising=False)
    else:
        monkeypatch.setenv("POVAR_RES_WGS", wgs)
    if not _EDGE:
        _EDGE.append(RB.edge_problem_joint(0))
    n_c, lm_off, cam_idx, obs, cams, lms_h = _EDGE[0]
    ctx = capi.Context(n_c, lm_off, cam_idx, obs, robust_norm=robust, huber=RB.EDGE_HUBER_H, e0_mode=capi.E0_IMPLICIT_LDSACC)
    ctx.layout_finalize(True)
    ctx.set_cameras(cams)
    ctx.set_landmarks_homogeneous(lms_h)
    assert ctx.linearize_homogeneous()
    ctx.prepare_joint(RB.EDGE_LAM_H)
    li = ctx.layout_info()
    assert li.res_ready_h == 1 and (wgs is None or li.res_wgs_h <= int(wgs))
    prob = RB.Step2.from_context(ctx, obs, robust, RB.EDGE_HUBER_H)
    ctx.power_series_begin()
    x0 = ctx.get_term(11)
    ctx.set_series_kernel(1)
    assert ctx.layout_info().res_active_h == 1
    it, st = ctx.power_series_pose(1)
    t1, inc = ctx.get_term(11), ctx.get_increment(11)
    assert ctx.layout_info().res_failed == 0, "the resident launch gave up: the per-term kernels computed this term"
    assert np.array_equal(inc, x0 + t1)
    t_ref, bound = RB.evaluate_joint(prob, x0, RB.MODELS_H["ckh"])
    r, j, n_over = RB.check(t1, t_ref, bound)
    print(f"E0HBOUND edge/{robust}/res_wgs={wgs or 'default'}({li.res_wgs_h}) series_res_h term=1 err/bound={r:.3g} "
          f"rel={rel(t1, t_ref.astype(np.float64)):.3g} over={n_over}")
    assert np.all(np.isfinite(t1))
    assert n_over == 0, (r, j // 11, j % 11, float(t1[j]), float(t_ref[j]), float(bound[j]))
    assert np.all(t1[11 * (n_c - 1):11 * n_c] == 0.0)
    ctx.close()


def test_resident_joint_series_follows_a_new_linearisation_and_damping():
    """The captured launch is replayed across LM iterations: new cameras, landmarks and lambda are picked up."""
    ctx = _ctx("trafalgar-257", linearize=False)
    _need_layout(ctx.layout_info())
    for lam in (1e-4, 1e-2):
        assert ctx.linearize_homogeneous()
        ctx.set_series_kernel(0)
        inc0 = ctx.solve_joint(lam, M)[0]
        ctx.set_series_kernel(1)
        assert ctx.layout_info().res_active_h == 1
        inc = ctx.solve_joint(lam, M)[0]
        assert rel(inc, inc0) < 1e-10
        ctx.apply_joint(inc0)
        ctx.normalize_joint()
    assert ctx.layout_info().res_failed == 0
    ctx.close()


def test_joint_series_kernel_is_chosen_by_timing_both():
    """Nothing forced: the first solve_joint times the per-term kernels and series_res_h on the prepared joint system and
    keeps the faster form; forcing either and handing the choice back work; step 1's state is untouched."""
    if os.environ.get("POVAR_RES") is not None:
        pytest.skip("the environment forces the series kernel: this test is about the automatic choice")
    ctx = _ctx("trafalgar-257")
    li = ctx.layout_info()
    _need_layout(li)
    assert li.res_auto_h == 1 and li.res_active_h == 0 and li.tune_terms_h_us == 0 and li.tune_res_h_us == 0
    step1 = (li.res_auto, li.res_active, li.tune_terms_us, li.tune_res_us)
    inc_auto = ctx.solve_joint(LAM, M)[0]
    li = ctx.layout_info()
    assert li.res_auto_h == 2 and li.tune_terms_h_us > 0 and li.tune_res_h_us > 0
    assert (li.res_active_h == 1) == (li.tune_res_h_us < 0.98 * li.tune_terms_h_us)
    assert (li.res_auto, li.res_active, li.tune_terms_us, li.tune_res_us) == step1
    print(f"RESH tune trafalgar-257 terms={li.tune_terms_h_us:.2f} us res={li.tune_res_h_us:.2f} us active={li.res_active_h} "
          f"wgs={li.res_wgs_h} rows={li.res_rows_h} shared={li.res_shared_h}")
    for forced in (0, 1):
        ctx.set_series_kernel(forced)
        li = ctx.layout_info()
        assert li.res_auto_h == 0 and li.res_active_h == forced
        assert rel(ctx.solve_joint(LAM, M)[0], inc_auto) < 1e-10
    ctx.set_series_kernel(-1)
    assert ctx.layout_info().res_auto_h == 1
    assert rel(ctx.solve_joint(LAM, M)[0], inc_auto) < 1e-10
    assert ctx.layout_info().res_auto_h == 2
    ctx.close()


def test_resident_joint_series_gives_up_and_the_per_term_kernels_take_over(monkeypatch):
    """A spin budget of one poll: the first hand-over that is not instantly there gives up; the library repeats the series
    with the per-term kernels and keeps the context on them."""
    monkeypatch.setenv("POVAR_RES_SPIN", "1")
    ctx = _ctx("trafalgar-257")
    _need_layout(ctx.layout_info())
    ctx.set_series_kernel(0)
    inc0 = ctx.solve_joint(LAM, M)[0]
    ctx.set_series_kernel(1)
    inc = ctx.solve_joint(LAM, M)[0]
    assert rel(inc, inc0) < 1e-10
    li = ctx.layout_info()
    if li.res_failed:
        assert li.res_active_h == 0
    ctx.close()


def test_resident_joint_series_continues_term_by_term():
    """After a resident solve_joint(m = 5), one power_series_step gives the sixth term of five per-term steps plus one."""
    ctx = _ctx("ladybug-49")
    _need_layout(ctx.layout_info())
    ctx.set_series_kernel(1)
    assert ctx.layout_info().res_active_h == 1
    inc5 = ctx.solve_joint(LAM, 5)[0]
    ctx.power_series_step()
    t6 = ctx.get_term(11)
    assert ctx.layout_info().res_failed == 0
    ref = _ctx("ladybug-49")
    ref.set_series_kernel(0)
    ref.prepare_joint(LAM)
    ref.power_series_begin()
    for _ in range(5):
        ref.power_series_step()
    assert rel(inc5, ref.get_increment(11)) < 1e-10
    ref.power_series_step()
    assert rel(t6, ref.get_term(11)) < 1e-9
    assert rel(ctx.get_increment(11), ref.get_increment(11)) < 1e-10
    ctx.close()
    ref.close()
