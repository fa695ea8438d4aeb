"""Constant cameras (povar_set_fixed_cameras) on the device, through the C ABI: B^-1 and the Schur-Jacobi inverse with zero
blocks on the fixed set F, every term and increment of every solver exactly zero on F and, on the free cameras, the
solve of S_ff x_f = -b_f; the covariance calls in the gauge F fixes (POVAR_COV_FIXED_GAUGE) and damped.

References: tests/fixed_cameras_reference.py -- the oracle's own series and PCG with zeroed blocks (held on the CPU, by
tests/test_fixed_cameras_reference.py, to the explicitly restricted system), the decoupled matrix CHOLESKY factors, and
[S_ff]^-1 zero-padded, fed to the formulas of the existing covariance reference modules.  Tolerances are the ones the
existing test of the same path states (named at each use); the bounds of the covariance cases are evaluated with the
matrices that are actually inverted (S_ff, and H without the fixed cameras).

Shapes: `small` (6 cameras, F = {1, 4}: camera 4 sits in the tail workgroup of cam_build_binv; dense n = 72 / 66 padded to
128), p22 (F = {2, 3, 5}: in step 1 camera 5 owns rows 60..71 and straddles a 64-row block; five blocks) and the edge graph
of tests/rounding_bounds.py with one unobserved camera (151 cameras; F = a hub, a one-observation camera, the unobserved
camera, the last camera) for the forced kernel families.  On the edge graph the tests check what only that graph shows --
exact zeros for those four kinds of camera in every family, bitwise-unchanged free blocks -- and leave the comparison
with the oracle to the shapes whose tolerances the existing step tests state.
"""
import copy
import os
import subprocess
import threading

import numpy as np
import pytest

import covariance_reference as R
import fixed_cameras_reference as FR
import landmark_covariance_reference as L
import sc_bounds as SB
import test_gpu_operand_bounds as G
from conftest import rel
from test_gpu_sharded import HostAllReduce

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA, LAM, M = 0.01, 1e-4, 20
DET_ENV = os.environ.get("POVAR_DETERMINISTIC") == "1"
LPL = {"POVAR_E0_V1": "0", "POVAR_LPL_PLACE": "sync"}


def _exact_zero(x, k):
    """+0.0 or -0.0 in every entry k."""
    return bool(np.all(np.asarray(x).reshape(-1)[k] == 0.0))


def _set_env(monkeypatch, env, det=False):
    if DET_ENV and not det:
        pytest.skip("POVAR_DETERMINISTIC=1 in the environment pins the kernels of this case")
    for k in G._OVERRIDES + ("POVAR_E0_V1", "POVAR_LPL_PLACE"):
        monkeypatch.delenv(k, raising=False)
    if not det:
        monkeypatch.delenv("POVAR_DETERMINISTIC", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# family of the power series: (environment, e0 mode, flags, what to set on the context, what layout_info must say afterwards)
def _families():
    from povar_amd import capi
    return {
        "auto": ({}, capi.E0_IMPLICIT, 0, lambda c: None, lambda li, joint: li.lane_per_landmark == 0),
        "e0_lpl": (LPL, capi.E0_IMPLICIT_LDSACC, 0, lambda c: (c.set_e0_kernel(0), c.set_series_kernel(0)),
                   lambda li, joint: li.lane_per_landmark == 1 and (li.e0_kernel_h if joint else li.e0_kernel) == 0),
        "e0_ck": ({**LPL, "POVAR_E0_CK": "1"}, capi.E0_IMPLICIT_LDSACC, 0, lambda c: c.set_series_kernel(0),
                  lambda li, joint: li.lane_per_landmark == 1 and (li.e0_kernel_h if joint else li.e0_kernel) >= 1),
        "det": ({**LPL, "POVAR_DETERMINISTIC": "1"}, capi.E0_IMPLICIT_LDSACC, 0, lambda c: None,
                lambda li, joint: (li.e0_kernel_h == 2) if joint else (li.e0_kernel == G.CK_VARIANTS + 1)),
        "resident": (LPL, capi.E0_IMPLICIT_LDSACC, 0, lambda c: c.set_series_kernel(1),
                     lambda li, joint: joint or li.res_active == 1),
        "fp32": (LPL, capi.E0_IMPLICIT_LDSACC, capi.FLAG_FP32_TERMS, lambda c: None, lambda li, joint: li.fp32_terms == 1),
        "no_graph": (LPL, capi.E0_IMPLICIT_LDSACC, capi.FLAG_NO_GRAPH, lambda c: c.set_series_kernel(0),
                     lambda li, joint: li.lane_per_landmark == 1),
    }


def _series_context(monkeypatch, fam, n_cams, lm_off, cam_idx, obs, cams, lms, step):
    from povar_amd import capi
    env, mode, flags, setup, _ = _families()[fam]
    _set_env(monkeypatch, env, det=fam == "det")
    ctx = capi.Context(n_cams, lm_off, cam_idx, obs, e0_mode=mode, flags=flags)
    ctx.layout_finalize(True)
    setup(ctx)
    ctx.set_cameras(cams)
    if step == 1:
        ctx.set_landmarks(lms)
        assert ctx.linearize_pose(ALPHA)
    else:
        ctx.set_landmarks_homogeneous(lms)
        assert ctx.linearize_homogeneous()
    return ctx


def _prepare(ctx, step, lam=LAM):
    if step == 1:
        ctx.prepare_pose(lam)
    else:
        ctx.prepare_joint(lam)


def _binv(ctx, step):
    from povar_amd import capi
    d = 12 if step == 1 else 11
    return ctx.get_buffer(capi.BUF_B_INV if step == 1 else capi.BUF_B_INV_JOINT).reshape(-1, d * d)


def _edge(step):
    """(n_cams, lm_off, cam_idx, obs, cams, lms, F) of the edge graph with its unobserved camera."""
    p = G.edge_pose("NONE") if step == 1 else G.edge_joint("NONE")
    assert p.n_cams == 151 and (p.n_c == 0).sum() == 1
    F = sorted({int(np.argmax(p.n_c)), int(np.flatnonzero(p.n_c == 1)[0]), int(np.flatnonzero(p.n_c == 0)[0]), p.n_cams - 1})
    assert p.n_c[F[0]] > 1000 or max(p.n_c[F]) > 1000
    return p, F


def _small_state(name, step):
    """(p, cams, lms, obs) of `small` / p22 at the state of the step's existing tests."""
    p = R.problem(name)
    if step == 1:
        from oracle import povar_oracle as O
        cams = np.asarray(p.cams, dtype=np.float64).reshape(-1, 12)
        return p, cams, O.Oracle(p.n_cams, p.lm_off, p.cam_idx, p.obs).init_landmarks_pose(ALPHA, cams), p.obs
    cams, lms_h, obs = R.state2(p)
    return p, cams, lms_h, obs


# ------------------------------------------------------------------------------------------ 4. B^-1
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("shape,fam", [("small", "auto"), ("edge", "auto"), ("edge", "e0_lpl"), ("edge", "det")])
def test_binv_blocks(monkeypatch, shape, fam, step):
    """Blocks on F exactly zero, every other block bitwise what the same context built before the set was installed, and the
    whole buffer bitwise back after the set is cleared.  The set takes effect at the next preparation, not before."""
    if shape == "small":
        p, cams, lms, obs = _small_state("small", step)
        n_cams, lm_off, cam_idx, F = p.n_cams, p.lm_off, p.cam_idx, list(FR.SETS["small"])
        assert n_cams % 4 != 0 and max(F) >= n_cams - n_cams % 4  # the tail workgroup of cam_build_binv[_h]
    else:
        p, F = _edge(step)
        n_cams, lm_off, cam_idx, obs, cams, lms = p.n_cams, p.lm_off, p.cam_idx, p.obs, p.cams, p.lms
    ctx = _series_context(monkeypatch, fam, n_cams, lm_off, cam_idx, obs, cams, lms, step)
    _prepare(ctx, step)
    B0 = _binv(ctx, step)
    assert np.all(np.isfinite(B0)) and ctx.fixed_cameras().size == 0
    ctx.set_fixed_cameras(F + F[:1])  # (a duplicate)
    assert list(ctx.fixed_cameras()) == sorted(F)
    assert np.array_equal(_binv(ctx, step), B0)  # a system prepared earlier is what it was
    _prepare(ctx, step)
    B1 = _binv(ctx, step)
    free = np.setdiff1d(np.arange(n_cams), F)
    assert np.all(B1[F] == 0.0)
    assert np.array_equal(B1[free], B0[free])
    assert ctx.layout_info().lane_per_landmark == (0 if fam == "auto" else 1)
    ctx.set_fixed_cameras([])
    assert ctx.fixed_cameras().size == 0
    _prepare(ctx, step)
    assert np.array_equal(_binv(ctx, step), B0)
    ctx.close()


# ------------------------------------------------------------------------------------------ 5. terms and sums
_SERIES = {}


def _masked_series(name, step):
    """The masked-oracle series of (`small` | p22, step): computed once, shared, never modified."""
    if (name, step) not in _SERIES:
        _SERIES[(name, step)] = FR.masked_series(R.problem(name), step, LAM, FR.SETS[name], M)
    return _SERIES[(name, step)]


SERIES_CASES = ([("small", f, s) for s in (1, 2) for f in ("auto", "e0_lpl", "e0_ck", "det", "resident", "no_graph")] +
                [("small", "fp32", 1), ("p22", "auto", 1), ("p22", "auto", 2), ("p22", "e0_ck", 1), ("p22", "e0_ck", 2)])


@pytest.mark.parametrize("name,fam,step", SERIES_CASES)
def test_series_terms_and_sum(monkeypatch, name, fam, step):
    """Every term and the final increment exactly zero on F; free entries against the masked-oracle series at the per-term
    tolerances of tests/test_gpu_step1.py (1e-12 / 1e-11 / 1e-10) and test_gpu_step2.py (1e-11 / 1e-10 / 1e-10), which run
    the same families on the same shapes; fp32 terms at test_gpu_fp32_terms.py's 1e-5 (the series start is fp64)."""
    from povar_amd import capi
    ref, terms, s = _masked_series(name, step)
    F = FR.SETS[name]
    p, cams, lms, obs = _small_state(name, step)
    dim = 12 if step == 1 else 11
    k = FR.fixed_coords(p.n_cams, dim, F)
    t0, tk, ts = ((1e-12, 1e-11, 1e-10) if step == 1 else (1e-11, 1e-10, 1e-10)) if fam != "fp32" else (1e-12, 1e-5, 1e-5)
    ctx = _series_context(monkeypatch, fam, p.n_cams, p.lm_off, p.cam_idx, obs, cams, lms, step)
    ctx.set_fixed_cameras(F)
    if fam != "resident":  # (the resident series is one launch: it has no term-by-term entry point)
        _prepare(ctx, step)
        ctx.power_series_begin()
        t = ctx.get_term(dim)
        assert _exact_zero(t, k) and rel(t, terms[0]) < t0, rel(t, terms[0])
        worst = 0.0
        for i in range(1, M + 1):
            ctx.power_series_step()
            t = ctx.get_term(dim)
            assert _exact_zero(t, k), i
            worst = max(worst, rel(t, terms[i]))
            assert rel(t, terms[i]) < tk, (i, rel(t, terms[i]))
        inc = ctx.get_increment(dim)
        print(f"{name} {fam} step {step}: worst term {worst:.3e}, sum {rel(inc, ref):.3e}")
        assert _exact_zero(inc, k) and rel(inc, ref) < ts
    if step == 1:
        inc, it, st, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
    else:
        inc, it, st, rc = ctx.solve_joint(LAM, M)
    assert rc == 0 and it == M
    assert _exact_zero(inc, k) and np.all(np.isfinite(inc)) and rel(inc, ref) < ts, rel(inc, ref)
    assert np.abs(inc.reshape(-1, dim)[np.setdiff1d(np.arange(p.n_cams), F)]).max(1).min() > 0
    assert _families()[fam][4](ctx.layout_info(), step == 2), fam
    ctx.close()


@pytest.mark.parametrize("fam,step", [(f, s) for s in (1, 2) for f in ("e0_lpl", "e0_ck", "det", "resident", "no_graph", "auto")] +
                         [("fp32", 1)])  # (the fp32 terms are step 1's)
def test_series_on_the_edge_graph(monkeypatch, fam, step):
    """A hub, a one-observation camera, the unobserved camera and the last camera fixed, in every forced family: their
    entries of the increment are exactly zero, every free camera that observes moves, and the deterministic family gives
    the same bits in two contexts."""
    from povar_amd import capi
    p, F = _edge(step)
    dim = 12 if step == 1 else 11
    k = FR.fixed_coords(p.n_cams, dim, F)
    out = []
    for _ in range(2 if fam == "det" else 1):
        ctx = _series_context(monkeypatch, fam, p.n_cams, p.lm_off, p.cam_idx, p.obs, p.cams, p.lms, step)
        ctx.set_fixed_cameras(F)
        inc, it, st, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, 10) if step == 1 else ctx.solve_joint(p.lam, 10)
        assert rc == 0 and np.all(np.isfinite(inc)) and _exact_zero(inc, k)
        moved = np.abs(inc.reshape(-1, dim)).max(1) > 0
        free = np.setdiff1d(np.arange(p.n_cams), F)
        assert moved[free][p.n_c[free] > 0].all()
        assert _families()[fam][4](ctx.layout_info(), step == 2), fam
        out.append(inc)
        ctx.close()
    if fam == "det":
        assert np.array_equal(out[0], out[1])


# ------------------------------------------------------------------------------------------ 6. PCG / RIPCG
def _sc_context(name, step, flags=0):
    """As tests/test_gpu_camera_covariance.py::_context: LinearizorSC's linearisation (no Jl column scaling in step 1)."""
    from povar_amd import capi
    p, cams, lms, obs = _small_state(name, step)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs, flags=flags)
    ctx.set_cameras(cams)
    if step == 1:
        ctx.set_landmarks(lms)
        ctx.set_jl_col_scaling(False)
        assert ctx.linearize_pose(ALPHA)
    else:
        ctx.set_landmarks_homogeneous(lms)
        assert ctx.linearize_homogeneous()
    return ctx


_SC = {}


def _sc_system(name, step, lam):
    if (name, step, lam) not in _SC:
        p = R.problem(name)
        _SC[(name, step, lam)] = R.system_pose(p, lam) if step == 1 else R.system_joint(p, lam)
    return _SC[(name, step, lam)]


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("name", ["small", "p22"])
def test_pcg(name, step):
    """The iteration count and termination of the oracle's PCG with zeroed inverse blocks; the increments after 1, 3 and 12
    (11) iterations and at eta = 1e-2 inside the tolerances tests/test_gpu_sc_solvers.py uses for those counts; exact zeros
    on F; the preconditioner's blocks zero on F."""
    from povar_amd import capi
    from oracle import povar_oracle as O
    p = R.problem(name)
    F = FR.SETS[name]
    sys_ = _sc_system(name, step, LAM)
    S, b = sys_[0], sys_[-1]
    dim = 12 if step == 1 else 11
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    minv = FR.masked(orc.block_jacobi_inverse(S, dim), F)
    k = FR.fixed_coords(p.n_cams, dim, F)
    ctx = _sc_context(name, step)
    ctx.set_fixed_cameras(F)

    def solve(min_it, max_it, eta):
        if step == 1:
            return ctx.solve_pose_sc(LAM, capi.SC_PCG, min_it, max_it, eta)
        return ctx.solve_joint_sc(LAM, min_it, max_it, eta)

    ref, it_o, st_o = orc.pcg(S, b, minv, dim=dim, eta=1e-2, max_iterations=500)
    inc, it, status, rc = solve(0, 500, 1e-2)
    assert rc == 0 and (it, status) == (it_o, st_o) and status == capi.SUCCESS
    assert _exact_zero(inc, k) and rel(inc, ref) < (1e-9 if step == 1 else 1e-8), rel(inc, ref)
    X = ctx.get_buffer(capi.BUF_SC_PRECOND, joint=step == 2).reshape(p.n_cams, -1)
    assert np.all(X[list(F)] == 0.0) and rel(X, minv) < (1e-8 if step == 1 else 1e-7)
    for n_it, tol in ([(1, 1e-11), (3, 1e-10), (12, 1e-7)] if step == 1 else [(1, 1e-10), (3, 1e-9), (11, 1e-6)]):
        ref_k, it_k, st_k = orc.pcg(S, b, minv, dim=dim, eta=0.0, max_iterations=n_it)
        inc_k, it_g, st_g, rc = solve(0, n_it, 0.0)
        print(f"{name} step {step} PCG {n_it} iterations: {rel(inc_k, ref_k):.3e}")
        assert rc == 0 and it_g == it_k == n_it and st_g == st_k
        assert _exact_zero(inc_k, k) and rel(inc_k, ref_k) < tol, n_it
    ctx.close()


# ------------------------------------------------------------------------------------------ 7. CHOLESKY / RICHOLESKY
_DENSE = {}


def _dense_case(name, step):
    """sc_bounds.dense_system of the case with A the decoupled matrix: S, b and their operand errors replaced on F by the
    identity's rows and columns and a zero right-hand side, which the device writes exactly (no error there)."""
    if (name, step) not in _DENSE:
        from povar_amd import synth
        n_c, n_l, n_o, seed = R.REGULAR[name]
        s = synth.make_problem(n_c, n_l, n_o, seed=seed)
        sy = SB.dense_system(SB.pose_case(s, "NONE", LAM) if step == 1 else SB.joint_case(s, "NONE", LAM), step == 2)
        sy = copy.copy(sy)
        k = FR.fixed_coords(n_c, sy.dim, FR.SETS[name])
        S, ES, b, Eb = sy.S.copy(), sy.ES.copy(), np.array(sy.b, copy=True), np.array(sy.Eb, copy=True)
        S[k, :], S[:, k], ES[k, :], ES[:, k] = 0, 0, 0, 0
        S[k, k] = 1
        b[k], Eb[k] = 0, 0
        sy.S, sy.ES, sy.b, sy.Eb = S, ES, b, Eb
        _DENSE[(name, step)] = sy
    return _DENSE[(name, step)]


@pytest.mark.parametrize("assembly", [1, 2], ids=["atomic", "ordered"])
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("name", ["small", "p22"])
def test_cholesky(name, step, assembly):
    """Through POVAR_BUF_SC_FACTOR: the rows of F are exactly identity rows with y = x = 0; |A - R^T R|, |b + R^T y| and
    |R x - y| inside the entrywise bounds of tests/sc_bounds.py with A the decoupled matrix; the increment exactly zero on F
    and the restricted solve on the rest; the ordered assembly bitwise equal across two calls."""
    from povar_amd import capi
    sy = _dense_case(name, step)
    p, n, N, dim = sy.p, sy.n, sy.N, sy.dim
    F = FR.SETS[name]
    k = FR.fixed_coords(p.n_cams, dim, F)
    if name == "p22" and step == 1:
        assert 60 <= k[12 * 2] < 64 <= k[12 * 3 - 1] and N == 320  # camera 5 straddles the first 64-row block; five blocks
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    ctx.set_sc_assembly(assembly)
    ctx.set_fixed_cameras(F)
    ctx.set_cameras(p.cams)

    def solve():
        if step == 1:
            ctx.set_landmarks(p.lms)
            ctx.set_jl_col_scaling(False)
            assert ctx.linearize_pose(p.alpha)
            return ctx.solve_pose_sc(p.lam, capi.SC_CHOLESKY)
        ctx.set_landmarks_homogeneous(p.lms)
        assert ctx.linearize_homogeneous()
        return ctx.solve_joint_sc(p.lam, method=capi.SC_CHOLESKY)

    inc, it, status, rc = solve()
    assert rc == 0 and it == 0 and status == capi.SUCCESS and ctx.sc_assembly() == assembly
    buf = ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
    Rf, y, x = np.triu(buf[:, :N]), buf[:, N], buf[:, N + 1]
    for i in k:
        assert Rf[i, i] == 1.0 and np.all(Rf[i, i + 1:] == 0.0) and np.all(Rf[:i, i] == 0.0), i
        assert y[i] == 0.0 and x[i] == 0.0, i
    fc = SB.factor_check(sy, buf)
    assert not fc.pop("padding")
    for what, (err, bound) in fc.items():
        r, i, over = SB.worst(err, bound)
        print(f"SCBOUND fixed {name} step {step} assembly {assembly} {what}={r:.3g}")
        assert not over, (what, r, i)
    assert np.array_equal(inc, x[:n]) and _exact_zero(inc, k)
    S64, b64 = np.asarray(sy.S, dtype=np.float64), np.asarray(sy.b, dtype=np.float64)
    S64 = np.triu(S64) + np.triu(S64, 1).T
    assert rel(inc, np.linalg.solve(S64, -b64)) < 1e-8  # (tests/test_gpu_sc_solvers.py::test_cholesky_pose's tolerance)
    bd = ctx.get_buffer(capi.BUF_SC_BLOCKDIAG, joint=step == 2).reshape(-1, dim, dim)
    assert np.all(np.abs((bd - sy.B).astype(np.float64)) <= sy.EB)  # unchanged on F too
    if assembly == 2:
        inc2, _, _, rc2 = solve()
        assert rc2 == 0 and np.array_equal(inc2, inc)
        assert np.array_equal(ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2), buf)
    ctx.close()


# ------------------------------------------------------------------------------------------ 8. apply
def test_apply_pose_keeps_the_fixed_cameras():
    """After apply_pose the cameras of F are bitwise the caller's; landmarks and l_diff against the oracle's back
    substitution called with the masked increment, at the apply tolerances of tests/test_gpu_step1.py::test_apply."""
    from povar_amd import capi
    ref, terms, s = _masked_series("small", 1)
    orc, st, hll, b, binv, sigma, lms = s
    p, F = R.problem("small"), list(FR.SETS["small"])
    cams = np.asarray(p.cams, dtype=np.float64).reshape(-1, 12)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    ctx.set_fixed_cameras(F)
    ctx.set_cameras(cams)
    ctx.set_landmarks(lms)
    assert ctx.linearize_pose(ALPHA)
    inc, _, _, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
    assert rc == 0 and rel(inc, ref) < 1e-10
    ld = ctx.apply_pose(capi.POWER_VARPROJ, ALPHA, inc)
    got = ctx.get_cameras().reshape(-1, 12)
    assert np.array_equal(got[F].view(np.int64), cams[F].view(np.int64))
    inc_s = inc * sigma  # (the device's own increment: its entries on F may be -0.0)
    cams_new = cams + inc_s.reshape(-1, 12)
    ld_o, lms_new = orc.back_substitute_pose(ALPHA, st, cams_new, lms, inc_s * (1.0 / sigma))
    assert rel(got, cams_new) < 1e-14 and rel(ctx.get_landmarks(), lms_new) < 1e-9
    assert abs(ld - ld_o) <= 1e-9 * abs(ld_o)
    ctx.close()


def test_apply_joint_keeps_the_fixed_cameras():
    """The same for apply_joint (tolerances of tests/test_gpu_step2.py); povar_normalize_joint then rescales every camera,
    fixed ones too: the same projective camera."""
    from povar_amd import capi
    ref, terms, s = _masked_series("small", 2)
    orc, st_h, st_n, hll, b, binv, sigma, jls, cams, lms_h, obs = s
    p, F = R.problem("small"), list(FR.SETS["small"])
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs)
    ctx.set_fixed_cameras(F)
    ctx.set_cameras(cams)
    ctx.set_landmarks_homogeneous(lms_h)
    assert ctx.linearize_homogeneous()
    inc, _, _, rc = ctx.solve_joint(LAM, M)
    assert rc == 0 and rel(inc, ref) < 1e-10
    ld = ctx.apply_joint(inc)
    got = ctx.get_cameras().reshape(-1, 12)
    assert np.array_equal(got[F].view(np.int64), cams[F].view(np.int64))
    ld_o, lms_new = orc.back_substitute_joint(st_h, jls, LAM, cams, lms_h, inc)
    cams_new = orc.apply_cam_inc_joint(cams, inc, sigma)
    assert abs(ld - ld_o) <= 1e-9 * abs(ld_o)
    assert rel(got, cams_new) < 1e-13 and rel(ctx.get_landmarks_homogeneous(), lms_new) < 1e-10
    ctx.normalize_joint()
    after = ctx.get_cameras().reshape(-1, 12)
    assert np.allclose(np.linalg.norm(after, axis=1), 1.0, rtol=0, atol=1e-15)
    assert rel(after[F], cams[F] / np.linalg.norm(cams[F], axis=1, keepdims=True)) < 1e-15
    ctx.close()


def test_three_lm_steps_keep_the_fixed_cameras():
    """Three steps of each stage through the binding (linearise, solve, apply): the cameras of F keep every bit, the others move."""
    from povar_amd import capi
    p, F = R.problem("small"), list(FR.SETS["small"])
    cams = np.asarray(p.cams, dtype=np.float64).reshape(-1, 12)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    ctx.set_fixed_cameras(F)
    ctx.set_cameras(cams)
    ctx.init_landmarks_pose(ALPHA)
    for _ in range(3):
        assert ctx.linearize_pose(ALPHA)
        inc, _, _, rc = ctx.solve_pose(1e-2, capi.POWER_VARPROJ, M)
        assert rc == 0
        ctx.apply_pose(capi.POWER_VARPROJ, ALPHA, inc)
    got = ctx.get_cameras().reshape(-1, 12)
    free = np.setdiff1d(np.arange(p.n_cams), F)
    assert np.array_equal(got[F].view(np.int64), cams[F].view(np.int64))
    assert np.all(np.abs(got[free] - cams[free]).max(1) > 0)
    ctx.close()
    cams2, lms_h, obs = R.state2(p)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs)
    ctx.set_fixed_cameras(F)
    ctx.set_cameras(cams2)
    ctx.set_landmarks_homogeneous(lms_h)
    for _ in range(3):
        assert ctx.linearize_homogeneous()
        inc, _, _, rc = ctx.solve_joint(1e-2, M)
        assert rc == 0
        ctx.apply_joint(inc)
    got = ctx.get_cameras().reshape(-1, 12)
    assert np.array_equal(got[F].view(np.int64), cams2[F].view(np.int64))
    assert np.all(np.abs(got[free] - cams2[free]).max(1) > 0)
    ctx.close()


# ------------------------------------------------------------------------------------------ 9. covariance
def _cov_context(name, step):
    """As tests/test_gpu_landmark_covariance.py::_context."""
    from povar_amd import capi
    p = L.problem(name)
    cams, lms, obs = L.state(p, step)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs)
    ctx.set_cameras(cams)
    if step == 1:
        ctx.set_landmarks(lms)
        assert ctx.linearize_pose(L.ALPHA)
    else:
        ctx.set_landmarks_homogeneous(lms)
        assert ctx.linearize_homogeneous()
    return ctx


def _block_err(got, want):
    return np.linalg.norm((np.asarray(got).astype(np.longdouble) - want).astype(np.float64), axis=(-2, -1))


@pytest.mark.parametrize("mode", ["fixed", "damped"])
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("name", ["small", "p22"])
def test_covariance(name, step, mode):
    """POVAR_COV_FIXED_GAUGE (lambda = 0) and POVAR_COV_DAMPED with F, both coords: the camera blocks per block inside
    n u cond_2(A) |A^-1|_2 with A = S_ff (the bound of tests/test_gpu_camera_covariance.py) and exactly zero on F; landmark,
    observation, hat and pair outputs against the existing reference modules' formulas fed the zero-padded C, at those
    modules' m u cond_2(K) |K^-1|_2 rule with K the matrix without the fixed cameras; pair blocks with a member in F exactly
    zero; in the fixed gauge sum h_i = DIM (n_cams - |F|) + 3 n_lms inside the summed bound, as the observation test holds
    its rank identity."""
    from povar_amd import capi
    import pair_covariance_reference as PC
    F = list(FR.SETS[name])
    lam, gauge = (0.0, capi.COV_FIXED_GAUGE) if mode == "fixed" else (LAM, capi.COV_DAMPED)
    ref = FR.cov_case(name, step, lam, F)
    s, osys = ref.sys, ref.osys
    ctx = _cov_context(name, step)
    ctx.set_fixed_cameras(F)
    tag = f"{mode} step {step} {name}"
    for coords in (capi.COV_SOLVER_COORDS, capi.COV_CAMERA_COORDS):
        lm, cam, rc = ctx.landmark_covariance(step=step, lam=lam, gauge=gauge, coords=coords, with_cameras=True)
        cam_only, rc2 = ctx.camera_covariance(step=step, lam=lam, gauge=gauge, coords=coords)
        assert rc == 0 and rc2 == 0, tag
        param = coords == capi.COV_CAMERA_COORDS
        want = R.to_camera_coords(ref.cam_blocks, s.sigma, step, s.cams) if param else ref.cam_blocks
        bound = ref.cam_bound * (float(s.sigma.max() ** 2) if param else 1.0)
        for got in (cam, cam_only):
            assert got.shape == want.shape and np.all(np.isfinite(got))
            err = _block_err(got, want)
            print(f"{tag} coords {coords}: camera blocks worst {err.max():.3e} = {err.max() / (bound / ref.cam_bound * ref.cam_unit):.3g} "
                  f"x u cond |A^-1| (bound {bound:.3e})")
            assert np.all(err <= bound), (tag, err.max(), bound)
            assert np.all(got[F] == 0.0) and np.array_equal(got, got.transpose(0, 2, 1))
        want = s.to_landmark_coords(ref.lm_blocks) if param else ref.lm_blocks
        scale = float(s.s.max() ** 2) if param else 1.0
        err = _block_err(lm, want)
        print(f"{tag} coords {coords}: landmark blocks worst {err.max():.3e} = {err.max() / (ref.full_unit * scale):.3g} x u cond |K^-1|")
        assert lm.shape == want.shape and np.all(err <= ref.full_bound * scale), (tag, err.max())
        assert np.array_equal(lm, lm.transpose(0, 2, 1))
        # pairs: every kind, with and without a member in F, both orders of the mixed kind
        rng = np.random.default_rng(step)
        cc, cl, ll = PC.sample_pairs(rng, s.n_cams, s.n_lms, 12)
        l0 = int(rng.integers(0, s.n_lms))
        pairs = cc + cl + ll + [(0, F[0], 0, F[1]), (0, F[0], 0, 0), (0, 0, 0, F[1]), (0, F[0], 1, l0), (1, l0, 0, F[1]), (0, F[1], 0, F[1])]
        blocks, rc = ctx.covariance_blocks(pairs, step=step, lam=lam, gauge=gauge, coords=coords)
        assert rc == 0
        worst = 0.0
        for pair, got in zip(pairs, blocks):
            want = ref.pairs.want(pair, param)
            bound = ref.full_bound * ref.pairs.scale(pair, param)
            e = float(_block_err(got, want))
            worst = max(worst, e / bound)
            assert got.shape == want.shape and e <= bound, (tag, pair, e, bound)
            if (pair[0] == 0 and pair[1] in F) or (pair[2] == 0 and pair[3] in F):
                assert np.all(got == 0.0), (tag, pair)
        print(f"{tag} coords {coords}: pair blocks worst err / bound {worst:.3g}")
    rows, rc = ctx.observation_covariance(step=step, lam=lam, gauge=gauge)
    assert rc == 0 and rows.shape == ref.obs_rows.shape and np.all(np.isfinite(rows[:, 0]))
    err = np.abs((rows.astype(np.longdouble) - ref.obs_rows).astype(np.float64))
    print(f"{tag}: observation rows worst err / bound {np.max(err / np.maximum(ref.obs_bound, 1e-300)):.3g}; sum h = {rows[:, 0].sum():.12f}, "
          f"free parameters {ref.rank}, summed bound {ref.obs_bound[:, 0].sum():.3e}")
    assert np.all(err <= ref.obs_bound), tag
    if mode == "fixed":
        assert abs(rows[:, 0].sum() - ref.rank) <= ref.obs_bound[:, 0].sum(), tag
    r, P, rc = ctx.observation_hat(step=step, lam=lam, gauge=gauge)
    assert rc == 0 and P.shape == ref.hat_blocks.shape and np.all(np.isfinite(P))
    err = np.abs((P.astype(np.longdouble) - ref.hat_blocks).astype(np.float64))
    print(f"{tag}: hat blocks worst err / bound {np.max(err / np.maximum(ref.hat_bound, 1e-300)):.3g}")
    assert np.all(err <= ref.hat_bound), tag
    # no gauge basis was built
    with pytest.raises(capi.PovarError):
        ctx.get_buffer(capi.BUF_COV_GAUGE, joint=step == 2)
    ctx.close()


# ------------------------------------------------------------------------------------------ 10. singular and argument cases
@pytest.mark.parametrize("step", [1, 2])
def test_one_fixed_camera_is_reported_as_singular(step):
    """F = {0} leaves a 4-dimensional null space in S_ff(0) (tests/test_fixed_cameras_reference.py): all-NaN output and
    POVAR_NUMERIC_FAILURE from every covariance family; with a second camera the same context answers."""
    from povar_amd import capi
    ctx = _sc_context("small", step)
    ctx.set_fixed_cameras([0])
    for coords in (0, 1):
        got, rc = ctx.camera_covariance(step=step, lam=0.0, gauge=capi.COV_FIXED_GAUGE, coords=coords)
        assert rc == capi.NUMERIC_FAILURE and np.all(np.isnan(got))
    lm, cam, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=capi.COV_FIXED_GAUGE, with_cameras=True)
    assert rc == capi.NUMERIC_FAILURE and np.all(np.isnan(lm)) and np.all(np.isnan(cam))
    rows, rc = ctx.observation_covariance(step=step, lam=0.0, gauge=capi.COV_FIXED_GAUGE)
    assert rc == capi.NUMERIC_FAILURE and np.all(np.isnan(rows))
    blocks, rc = ctx.covariance_blocks([(0, 1, 0, 2), (0, 0, 1, 3)], step=step, lam=0.0, gauge=capi.COV_FIXED_GAUGE)
    assert rc == capi.NUMERIC_FAILURE and all(np.all(np.isnan(b)) for b in blocks)
    ctx.set_fixed_cameras([0, 1])
    got, rc = ctx.camera_covariance(step=step, lam=0.0, gauge=capi.COV_FIXED_GAUGE)
    assert rc == 0 and np.all(np.isfinite(got)) and np.all(got[[0, 1]] == 0.0)
    ctx.close()


def test_argument_errors():
    import ctypes as C
    from povar_amd import capi
    ctx = _sc_context("small", 1)
    out = np.zeros(144 * ctx.n_cams)

    def call(lam, gauge):
        return ctx.L.povar_camera_covariance_pose(ctx.h, C.c_double(lam), C.c_int32(gauge), C.c_int32(0), C.c_void_p(out.ctypes.data))

    assert call(0.0, capi.COV_FIXED_GAUGE) < 0                      # no fixed cameras
    assert b"POVAR_COV_FIXED_GAUGE" in ctx.L.povar_last_error()
    ctx.set_fixed_cameras([1, 4])
    assert call(1e-4, capi.COV_FIXED_GAUGE) < 0                     # lambda != 0
    assert call(0.0, capi.COV_FREE_GAUGE) < 0                       # the free gauge with fixed cameras
    assert b"POVAR_COV_FIXED_GAUGE" in ctx.L.povar_last_error()    # ... and the message names the gauge to ask for
    assert call(0.0, 3) < 0 and call(0.0, capi.COV_DAMPED) < 0
    # an id out of range: an error, and the set is what it was
    for bad in ([1, ctx.n_cams], [-1], [0, 2, 99]):
        ids = np.asarray(bad, dtype=np.int32)
        assert ctx.L.povar_set_fixed_cameras(ctx.h, C.c_void_p(ids.ctypes.data), C.c_int32(ids.size)) < 0
        assert list(ctx.fixed_cameras()) == [1, 4]
    assert ctx.L.povar_fixed_cameras(ctx.h, None) == 2
    assert call(0.0, capi.COV_FIXED_GAUGE) == 0
    # a null pointer clears the set
    assert ctx.L.povar_set_fixed_cameras(ctx.h, None, C.c_int32(3)) == 0 and ctx.fixed_cameras().size == 0
    assert call(0.0, capi.COV_FREE_GAUGE) == 0
    ctx.close()


def test_two_shards_hold_the_same_cameras():
    """Two shard contexts over the host all-reduce hook, F set on both ranks: the increments of the power series and of
    CHOLESKY equal the unsharded ones within the sharded tests' 1e-11 (tests/test_gpu_sharded.py), zeros on F exactly."""
    from povar_amd import capi
    p, cams, lms, obs = _small_state("p22", 1)
    F = list(FR.SETS["p22"])
    k = FR.fixed_coords(p.n_cams, 12, F)

    def run(ctx, lb, le):
        ctx.set_fixed_cameras(F)
        ctx.set_cameras(cams)
        ctx.set_landmarks(lms[lb:le])
        assert ctx.linearize_pose(ALPHA)
        inc, _, _, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
        inc_c, _, _, rc_c = ctx.solve_pose_sc(LAM, capi.SC_CHOLESKY)
        assert rc == 0 and rc_c == 0
        return inc, inc_c

    one = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs)
    ref = run(one, 0, p.n_lms)
    one.close()
    world = 2
    ar = HostAllReduce(world)
    out = [None] * world

    def worker(rank):
        try:
            lb, le = capi.shard_range(p.lm_off, world, rank)
            ob, oe = int(p.lm_off[lb]), int(p.lm_off[le])
            ctx = capi.Context(p.n_cams, p.lm_off[lb:le + 1] - p.lm_off[lb], p.cam_idx[ob:oe], obs[ob:oe])
            ctx.comm_init_host(world, rank, ar.fn(rank))
            out[rank] = run(ctx, lb, le)
            ctx.close()
        except BaseException:
            ar.bar.abort()  # a failed rank must not leave the other one waiting
            raise

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert all(o is not None for o in out)
    for o in out:
        for got, want in zip(o, ref):
            assert _exact_zero(got, k) and _exact_zero(want, k) and rel(got, want) < 1e-11, rel(got, want)


# ------------------------------------------------------------------------------------------ 11. bal
def test_bal_fixed_cameras(tmp_path):
    """`bal --fixed-cameras 0,1` with the direct solvers of both steps: exits 0, announces the set and writes a covariance file that names the gauge, with all-zero blocks 0 and 1 and finite symmetric blocks elsewhere."""
    from povar_amd import synth
    # The datum has to agree with the observations: two cameras held at arbitrary matrices impose a fundamental matrix the
    # image points contradict (landmarks run off to infinity and the report is, rightly, "singular").  So the start is the
    # known-answer tests': ground-truth cameras perturbed by 1 %, with cameras 0 and 1 -- the datum -- unperturbed.
    p = synth.make_problem(10, 300, 1300, seed=21, init="gt", init_noise=0.01)
    p.cams[:2] = synth.make_problem(10, 300, 1300, seed=21, init="gt", init_noise=0.0).cams[:2]
    f = str(tmp_path / "problem-10-300.txt")
    synth.write_data_custom(f, p)
    out = str(tmp_path / "cov.txt")
    cmd = [os.path.join(ROOT, "bin/bal"), "--input", f, "--quiet", "--max-num-iterations-step-1", "6", "--max-num-iterations-step-2", "3",
           "--log-log-path", str(tmp_path / "log.json"), "--fixed-cameras", "0,1", "--solver-type-step-1", "CHOLESKY",
           "--solver-type-step-2", "RICHOLESKY", "--camera-covariance-path", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "fixed cameras: 2 of 10\n" in r.stdout
    lines = open(out).read().split("\n")
    head = lines[0].split()
    assert int(head[0]) == p.n_cams and "fixed-gauge" in head[1:]
    blocks = np.array([[float(x) for x in ln.split()] for ln in lines[1:1 + p.n_cams]]).reshape(p.n_cams, 12, 12)
    assert np.all(blocks[:2] == 0.0)
    assert np.all(np.isfinite(blocks[2:])) and np.array_equal(blocks, blocks.transpose(0, 2, 1))
    assert np.all(np.linalg.norm(blocks[2:], axis=(1, 2)) > 0)
    assert "[WARN]" not in r.stdout
