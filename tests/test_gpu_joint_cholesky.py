"""Step 2's direct solve (povar_solve_joint_sc_method with POVAR_SC_CHOLESKY; `bal --solver-type-step-2 RICHOLESKY`) and
povar_right_mul_e0_joint against the CPU oracle, through the C ABI.

The oracle forms the dense joint system block by block as add_Hb_joint does (get_hb_joint) and solves it by Cholesky
(cholesky_solve); the device assembles the same S in closed form (sc_dense_offdiag_h / sc_dense_diag<11>, fp64 atomics)
and factors it with the kernels of step 1's CHOLESKY.  On every shape used here S is positive definite with
cond(S) <= 7.7e4 for NONE and HUBER at lambda = 1e-4 and 1.0, and the oracle's Cholesky agrees with an LU solve to 4.3e-12,
so the bounds of a direct solve are those of test_cholesky_pose: rel(inc, ref) < 1e-8 and rel(S inc, -b) < 1e-9.
(The assembly, the factor and both triangular solves are held entry by entry in tests/test_gpu_sc_bounds.py.)
"""
import threading

import numpy as np
import pytest

from conftest import rel

pytestmark = pytest.mark.gpu

ALPHA, LAM = 0.01, 1e-4


def _state2(n_cams, n_lms, seed=11):
    """The step-2 state of tests/test_gpu_sc_solvers.py::_state2: random normalised cameras, X_w = 1 landmarks."""
    rng = np.random.default_rng(seed)
    cams = rng.normal(size=(n_cams, 12))
    cams[:, 8:11] *= 0.1
    cams[:, 11] = 5 + rng.random(n_cams)
    cams /= np.linalg.norm(cams, axis=1, keepdims=True)
    lms_h = np.concatenate([rng.normal(size=(n_lms, 3)), np.ones((n_lms, 1))], 1)
    return cams, lms_h, rng


def _oracle_joint(orc, cams, lms_h, lam):
    # LinearizorSC::linearize_projective_space_homogeneous + solve_joint (linearizor_sc.cpp:196-303)
    st_h, ok = orc.linearize_homogeneous(cams, lms_h)
    diag2 = orc.jp_diag2_homogeneous(st_h)
    jls = orc.scale_jl_cols_homogeneous(st_h)
    sigma = 1.0 / (1e-5 + np.sqrt(diag2))
    orc.scale_jp_cols_joint(st_h, sigma)
    st_n = orc.linearize_nullspace(cams, lms_h, st_h)
    S, b = orc.get_hb_joint(st_h, st_n, lam)
    return st_h, jls, sigma, S, b


def _context(capi, n_cams, lm_off, cam_idx, obs, cams, lms_h, **kw):
    ctx = capi.Context(n_cams, lm_off, cam_idx, obs, **kw)
    ctx.set_cameras(cams)
    ctx.set_landmarks_homogeneous(lms_h)
    assert ctx.linearize_homogeneous()
    return ctx


def _check_direct(capi, orc, ctx, cams, lms_h, lam):
    st_h, jls, sigma, S, b = _oracle_joint(orc, cams, lms_h, lam)
    ref, bad = orc.cholesky_solve(S, b)
    assert bad == 0
    inc, it, status, rc = ctx.solve_joint_sc(lam, method=capi.SC_CHOLESKY)
    e_inc, e_res = rel(inc, ref), rel(S @ inc, -b)
    print(f"lambda {lam:g}: rel(inc, ref) {e_inc:.3e}  rel(S inc, -b) {e_res:.3e}")
    assert rc == 0 and it == 0 and status == capi.SUCCESS
    assert e_inc < 1e-8, lam
    assert e_res < 1e-9, lam
    return st_h, jls, sigma, S, b, ref, inc


@pytest.mark.parametrize("which,norm", [("small", "NONE"), ("small", "HUBER"), ("medium", "NONE"), ("p64", "NONE")])
def test_richolesky_joint(which, norm, small_problem, medium_problem):
    """Parity with the oracle's dense Cholesky: n = 66, n = 539 (padded to 576) and n = 704 = 11 * 64 (no padding)."""
    from povar_amd import capi, synth
    from oracle import povar_oracle as O
    p = {"small": small_problem, "medium": medium_problem}.get(which) or synth.make_problem(64, 400, 1800, seed=64)
    assert which != "p64" or (11 * p.n_cams) % 64 == 0
    cams, lms_h, _ = _state2(p.n_cams, p.n_lms)
    obs = p.obs / 500.0
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, obs, robust_norm=norm, huber=0.5)
    ctx = _context(capi, p.n_cams, p.lm_off, p.cam_idx, obs, cams, lms_h, robust_norm=norm, huber=0.5)
    for lam in (1.0, LAM):
        st_h, jls, sigma, S, b, ref, inc = _check_direct(capi, orc, ctx, cams, lms_h, lam)
    # the inspection buffers keep their meaning after a direct solve
    assert rel(ctx.get_buffer(capi.BUF_SC_PRECOND, joint=True), orc.block_jacobi_inverse(S, 11).ravel()) < 1e-7
    # apply_joint consumes the direct increment exactly as the RIPOBA / RIPCG one (tolerances of test_ripcg_joint)
    ld = ctx.apply_joint(inc)
    ld_o, lms_new = orc.back_substitute_joint(st_h, jls, LAM, cams, lms_h, inc)
    cams_new = orc.apply_cam_inc_joint(cams, inc, sigma)
    assert abs(ld - ld_o) <= 1e-9 * abs(ld_o)
    assert rel(ctx.get_cameras(), cams_new) < 1e-13 and rel(ctx.get_landmarks_homogeneous(), lms_new) < 1e-10
    with pytest.raises(capi.PovarError):
        ctx.solve_joint_sc(LAM, method=7)
    ctx.close()


def _edge_graph():
    """The graph of test_edge_cases_long_landmarks_and_unobserved_cameras: landmarks of 140, 97, 65 and 64 observations
    (several staging chunks in both chunk loops of sc_dense_offdiag_h), 120 two-view landmarks, cameras nobody observes."""
    rng = np.random.default_rng(17)
    n_c = 150
    used = np.setdiff1d(np.arange(n_c), [3, 77, 149])
    degs = [140, 97, 65, 64] + [2] * 120 + list(rng.integers(3, 9, size=150))
    cam_idx = np.concatenate([np.sort(rng.choice(used, k, replace=False)) for k in degs]).astype(np.int32)
    lm_off = np.concatenate([[0], np.cumsum(degs)]).astype(np.int32)
    return n_c, used, degs, cam_idx, lm_off


@pytest.mark.parametrize("norm", ["NONE", "HUBER"])
def test_richolesky_edge_graph(norm):
    from povar_amd import capi
    from oracle import povar_oracle as O
    n_c, used, degs, cam_idx, lm_off = _edge_graph()
    n_l = len(degs)
    cams, lms_h, rng = _state2(n_c, n_l)
    lm_of = np.repeat(np.arange(n_l), degs)
    pc = np.einsum("nij,nj->ni", cams[cam_idx].reshape(-1, 3, 4), lms_h[lm_of])
    assert np.abs(pc[:, 2]).min() > 0.5  # (0.66: no observation near the plane at infinity of its camera)
    obs = pc[:, :2] / pc[:, 2:3] + rng.normal(scale=0.05, size=(len(cam_idx), 2))
    orc = O.Oracle(n_c, lm_off, cam_idx, obs, robust_norm=norm, huber=0.05)
    ctx = _context(capi, n_c, lm_off, cam_idx, obs, cams, lms_h, robust_norm=norm, huber=0.05)
    st_h, jls, sigma, S, b, ref, inc = _check_direct(capi, orc, ctx, cams, lms_h, LAM)
    unused = np.setdiff1d(np.arange(n_c), used)
    assert np.all(ref.reshape(n_c, 11)[unused] == 0) and np.all(inc.reshape(n_c, 11)[unused] == 0)
    ctx.close()


def test_richolesky_is_the_limit_of_ripcg_and_ripoba(medium_problem):
    """The step-2 copy of the last lines of test_full_size_properties: RIPCG approaches the direct increment monotonically
    with the forcing sequence, and more terms of the RIPOBA series move towards it."""
    from povar_amd import capi
    p = medium_problem
    cams, lms_h, _ = _state2(p.n_cams, p.n_lms)
    ctx = _context(capi, p.n_cams, p.lm_off, p.cam_idx, p.obs / 500.0, cams, lms_h)
    x_c, it, st, rc = ctx.solve_joint_sc(LAM, method=capi.SC_CHOLESKY)
    assert rc == 0 and it == 0
    errs = []
    for eta in (1e-1, 1e-3, 1e-6):
        x, it, st, rc = ctx.solve_joint_sc(LAM, 0, 500, eta)
        assert rc == 0 and st == capi.SUCCESS and 0 < it < 500
        errs.append(rel(x, x_c))
    e20 = rel(ctx.solve_joint(LAM, 20)[0], x_c)
    e80 = rel(ctx.solve_joint(LAM, 80)[0], x_c)
    print("RIPCG errors", errs, "RIPOBA e20, e80", e20, e80)
    assert errs[0] > errs[1] > errs[2]
    assert e80 < e20 < 1.0
    ctx.close()


@pytest.mark.parametrize("which", ["small", "medium"])
def test_right_mul_e0_joint(which, small_problem, medium_problem):
    """B x - right_mul_e0_joint(x) == S x with the oracle's dense S: the bound of one E0 application (1e-11)."""
    from povar_amd import capi
    from oracle import povar_oracle as O
    p = small_problem if which == "small" else medium_problem
    cams, lms_h, rng = _state2(p.n_cams, p.n_lms)
    obs = p.obs / 500.0
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, obs)
    ctx = _context(capi, p.n_cams, p.lm_off, p.cam_idx, obs, cams, lms_h)
    st_h, jls, sigma, S, b = _oracle_joint(orc, cams, lms_h, LAM)
    inc, it, st, rc = ctx.solve_joint_sc(LAM, method=capi.SC_CHOLESKY)
    assert rc == 0
    bm = ctx.get_buffer(capi.BUF_SC_BLOCKDIAG, joint=True).reshape(p.n_cams, 11, 11)
    x = rng.normal(size=11 * p.n_cams)
    Sx = np.einsum("cij,cj->ci", bm, x.reshape(-1, 11)).ravel() - ctx.right_mul_e0_joint(x)
    err = rel(Sx, S @ x)
    print("rel(B x - E0 x, S x)", err)
    assert err < 1e-11
    ctx.close()


def test_right_mul_e0_joint_needs_the_joint_system(small_problem):
    from povar_amd import capi
    p = small_problem
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    x = np.ones(11 * p.n_cams)
    with pytest.raises(capi.PovarError, match="joint"):  # nothing prepared yet
        ctx.right_mul_e0_joint(x)
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(ALPHA)
    assert ctx.linearize_pose(ALPHA)
    ctx.solve_pose(LAM, capi.POWER_VARPROJ, 3)
    with pytest.raises(capi.PovarError, match="joint"):  # the prepared system is step 1's
        ctx.right_mul_e0_joint(x)
    assert np.all(np.isfinite(ctx.solve_pose(LAM, capi.POWER_VARPROJ, 3)[0]))  # the context is still usable
    ctx.close()


def test_richolesky_at_size():
    """trafalgar-257 (n = 2827): the oracle's dense S is out of reach for the suite, so the direct solve is checked through
    the residual |B x - E0 x + b| / |b| with E0 applied by the independent povar_right_mul_e0_joint entry point."""
    from povar_amd import capi, synth
    p = synth.make_bal_problem("trafalgar-257")
    cams, lms_h, _ = _state2(p.n_cams, p.n_lms)  # (the state of test_step2_at_size)
    ctx = _context(capi, p.n_cams, p.lm_off, p.cam_idx, p.obs / 500.0, cams, lms_h, e0_mode=capi.E0_IMPLICIT_LDSACC)
    lam = 1e-2

    def residual(x):
        bm = ctx.get_buffer(capi.BUF_SC_BLOCKDIAG, joint=True).reshape(p.n_cams, 11, 11)
        b = ctx.get_buffer(capi.BUF_B_JOINT)
        Sx = np.einsum("cij,cj->ci", bm, x.reshape(-1, 11)).ravel() - ctx.right_mul_e0_joint(x)
        return np.linalg.norm(Sx + b) / np.linalg.norm(b)

    x_c, it, st, rc = ctx.solve_joint_sc(lam, method=capi.SC_CHOLESKY)
    assert rc == 0 and it == 0
    r_c = residual(x_c)
    res = []
    for eta in (1e-1, 1e-3, 1e-6):
        x, it, st, rc = ctx.solve_joint_sc(lam, 0, 500, eta)
        assert rc == 0 and st == capi.SUCCESS and 0 < it < 500
        res.append(residual(x))
    print("direct residual", r_c, "RIPCG residuals", res)
    assert res[0] > res[1] > res[2] > r_c
    assert r_c < 1e-11
    ctx.close()


class HostAllReduce:
    def __init__(self, world):
        self.world, self.bar = world, threading.Barrier(world)
        self.bufs = [None] * world

    def fn(self, rank):
        def f(buf):
            self.bufs[rank] = buf.copy()
            self.bar.wait()
            tot = sum(self.bufs[r] for r in range(self.world))  # fixed order on every rank
            self.bar.wait()
            buf[:] = tot
        return f


def test_richolesky_sharded_matches_single():
    """Two landmark shards in one process over the host exchange hook (as test_sharded_explicit_sc_solvers_match_single):
    each shard assembles its landmarks' part of S, B_c / rhs / padding come from rank 0, the matrix is all-reduced."""
    from povar_amd import capi, synth
    p = synth.make_problem(30, 1500, 6500, seed=14)
    cams, lms_h, _ = _state2(p.n_cams, p.n_lms)
    obs = p.obs / 500.0

    def run(ctx, lb, le):
        ctx.set_cameras(cams)
        ctx.set_landmarks_homogeneous(lms_h[lb:le])
        ok = ctx.linearize_homogeneous()
        return ok, ctx.solve_joint_sc(LAM, method=capi.SC_CHOLESKY)

    ref_ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs, e0_mode=0)
    ok, (inc_r, it_r, st_r, rc_r) = run(ref_ctx, 0, p.n_lms)
    ref_ctx.close()
    assert ok and rc_r == 0 and it_r == 0
    world = 2
    ar = HostAllReduce(world)
    out = [None] * world

    def worker(rank):
        lb, le = capi.shard_range(p.lm_off, world, rank)
        ob, oe = int(p.lm_off[lb]), int(p.lm_off[le])
        ctx = capi.Context(p.n_cams, p.lm_off[lb:le + 1] - p.lm_off[lb], p.cam_idx[ob:oe], obs[ob:oe], e0_mode=0)
        ctx.comm_init_host(world, rank, ar.fn(rank))
        out[rank] = run(ctx, lb, le)
        ctx.close()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=300) for t in th]
    for o in out:
        assert o is not None and o[0]
        inc, it, st, rc = o[1]
        assert rc == 0 and (it, st) == (it_r, st_r) and rel(inc, inc_r) < 1e-9


@pytest.mark.parametrize("order", ["1-2-1", "2-1"])
def test_cholesky_in_both_steps_of_one_context(order, medium_problem):
    """One context, CHOLESKY in step 1 (n = 588, padded to 640) and in step 2 (n = 539, padded to 576): the dense buffer
    is reused for the smaller system and grown for the larger, and every solve stays within its bound.  The context's
    observations are the normalised ones of the step-2 tests (obs / 500); step 1 runs on the problem's cameras in the
    same units (the first two rows of every P divided by 500)."""
    from povar_amd import capi
    from oracle import povar_oracle as O
    p = medium_problem
    obs = p.obs / 500.0
    cams1 = p.cams.copy()
    cams1[:, :8] /= 500.0
    cams2, lms_h, _ = _state2(p.n_cams, p.n_lms)
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, obs)
    lms = orc.init_landmarks_pose(ALPHA, cams1)
    st = orc.linearize_pose(ALPHA, cams1, lms)[0]
    orc.scale_jp_cols_pose(st, 1.0 / (1e-5 + np.sqrt(orc.jp_diag2_pose(st))))
    S1, b1 = orc.get_hb_pose(st, LAM)
    ref1, bad = orc.cholesky_solve(S1, b1)
    assert bad == 0
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs)

    def step1():
        ctx.set_cameras(cams1)
        ctx.set_landmarks(lms)
        ctx.set_jl_col_scaling(False)
        assert ctx.linearize_pose(ALPHA)
        inc, it, status, rc = ctx.solve_pose_sc(LAM, capi.SC_CHOLESKY)
        e_inc, e_res = rel(inc, ref1), rel(S1 @ inc, -b1)
        print(f"step 1: rel(inc, ref) {e_inc:.3e}  rel(S inc, -b) {e_res:.3e}")
        assert rc == 0 and it == 0 and e_inc < 1e-8 and e_res < 1e-9

    def step2():
        ctx.set_cameras(cams2)
        ctx.set_landmarks_homogeneous(lms_h)
        assert ctx.linearize_homogeneous()
        _check_direct(capi, orc, ctx, cams2, lms_h, LAM)

    for s in order.split("-"):
        (step1 if s == "1" else step2)()
    ctx.close()
