"""The explicit-Schur-complement path held, entry by entry, to the long-double references and derived bounds of
tests/sc_bounds.py: POVAR_BUF_SC_BLOCKDIAG (cam_build_sc without moments), POVAR_BUF_SC_PRECOND (cm_gram_sc, cam_sum_parts60,
cam_build_sc: right residual and symmetry), and through POVAR_BUF_SC_FACTOR the dense assembly (sc_dense_diag,
sc_dense_offdiag[_h]), the blocked factorisation (chol_diag, chol_trsm, chol_syrk, chol_syrk_outer) and both triangular solves
(chol_back_solve, chol_back_update) of CHOLESKY and RICHOLESKY:
    factor    |S_ref - R^T R|_ij <= g(k_f) (|R^T| |R|)_ij + E(S)_ij  for every i <= j < n
    forward   |b_ref + R^T y|_i  <= g(k_f) (|R^T| |y|)_i + E(b)_i
    back      |R x - y|_i        <= g(k_b) (|R| |x|)_i
    padding   rows and columns [n, N) of R are the identity, y and x are 0 there; inc == x[:n] bit for bit
    chains    the diagonal blocks of R^T R against BLOCKDIAG_dev - (the reference's E0 diagonal): the dense assembly and
              the preconditioner's chain form S_cc independently
with the device's own R, y, x and references built from what the caller set alone (graph, image points, cameras, landmarks,
alpha, lambda, robust norm): no condition number, no entry excluded.  tests/test_sc_bounds.py shows on the CPU that every
shape used here meets the helper's conditions and that the defects a relative 2-norm lets through are reported.

Shapes (n -> N = n rounded up to 64):
  step 1  make_problem(5, 30, 120)     60 -> 64     chol_diag and chol_trsm on the rhs column only; a padding of 4
          16 cameras                   192 = N      chol_syrk inside one block; no padding, no outer update
          26 cameras                   312 -> 320   one chol_syrk_outer whose only tile reaches into the slack rows and holds the rhs
          medium_problem               588 -> 640   two outer updates, several 128-tiles, the rhs in the last j-tile
  step 2  small_problem                66 -> 128
          29 cameras                   319 -> 320   a padding of 1
          make_problem(64, 400, 1800)  704 = N
  both    the edge graph               1800 -> 1856, 1650 -> 1664: landmarks of 140 / 97 / 65 / 64 / 33 observations (both
          staging chunk sizes), 120 two-view landmarks, three cameras nobody observes
Variants: NONE and HUBER and lambda = 1e-4 and 1.0 on the small shapes; the automatic kernel family and the lane-per-landmark
one (ensure_legacy rebuilds what cm_gram_sc reads); one two-shard case over the host all-reduce hook.

Measured on an MI355X when these tests were written (largest err / bound per check over the cases of a shape; every figure
is printed as "SCBOUND ..." before it is asserted; for information, no bound is tuned by them):
  shape (its cases)      BLOCKDIAG  PRECOND   symmetry  factor  forward  back    chains
  pose-5 (5)             0.052      0.019     0.0015    0.044   0.014    0.024   0.029
  16 cameras (2)         0.077      0.011     0.00058   0.032   0.0094   0.027   0.022
  26 cameras (2)         0.12       0.029     0.00099   0.032   0.019    0.027   0.026
  medium_problem (2)     0.12       0.022     0.0013    0.33    0.016    0.032   0.020
  edge graph, step 1 (2) 0.12       0.012     8.1e-5    0.030   0.013    0.021   0.016
  small_problem (5)      0.029      0.0091    0.00047   0.019   0.0019   0.019   0.012
  29 cameras (2)         0.029      0.013     0.00097   0.029   0.0027   0.029   0.018
  29 cameras, two shards 0.024      0.00075   2.0e-5    0.027   0.00042  0.010   0.0040
  64 cameras (2)         0.026      0.015     0.00095   0.051   0.0050   0.035   0.013
  edge graph, step 2 (2) 0.026      0.013     4.8e-5    0.031   0.0038   0.015   0.0068
The operand perturbations (sigma, Hll^-1, the weights) carry most of E(S) and E(B_c), which is why the ratios are small; the
factor's 0.33 is medium_problem at lambda = 1, where E(S) is smallest against g(k_f) |R^T| |R|.  The fp64 emulations of
tests/test_sc_bounds.py land on the same figures (0.32 for that entry).  No case exposed a defect: the kernels are unchanged.
"""
import threading

import numpy as np
import pytest

import sc_bounds as SB
import test_gpu_operand_bounds as G
import test_sc_bounds as T

pytestmark = pytest.mark.gpu
F = np.float64
_REF = {}


def _reference(name, robust, lam, shards=1):
    """The reference of one case, computed once and left unchanged."""
    if shards == 1:
        return T.system(name, robust, lam)
    key = (name, robust, lam, shards)
    if key not in _REF:
        step, make = T.SHAPES[name]
        _REF[key] = SB.dense_system(make(robust, lam), step == 2, shards=shards)
    return _REF[key]


def _context(monkeypatch, fam, p):
    from povar_amd import capi
    if fam == "lpl":
        return G._create(monkeypatch, "lpl", p)
    for k in G._OVERRIDES + ("POVAR_E0_V1",):
        monkeypatch.delenv(k, raising=False)
    return capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=p.robust, huber=p.huber, eps=p.eps)


def _solve(ctx, sy, lms=None):
    """Linearise at the case's point and solve directly; (inc, rc)."""
    from povar_amd import capi
    p = sy.p
    ctx.set_cameras(p.cams)
    if sy.joint:
        ctx.set_landmarks_homogeneous(p.lms if lms is None else lms)
        assert ctx.linearize_homogeneous()
        inc, it, status, rc = ctx.solve_joint_sc(p.lam, method=capi.SC_CHOLESKY)
    else:
        ctx.set_landmarks(p.lms if lms is None else lms)
        ctx.set_jl_col_scaling(False)
        assert ctx.linearize_pose(p.alpha)
        inc, it, status, rc = ctx.solve_pose_sc(p.lam, capi.SC_CHOLESKY)
    assert rc == 0 and it == 0 and status == capi.SUCCESS
    return inc


def _where(sy, what, i):
    n, dim = sy.n, sy.dim
    if what == "factor":
        r, c = divmod(i, n)
        return f"entry ({r}, {c}): cameras ({r // dim}, {c // dim}), panel {r // 64}, block {r // 256}, 16-tile ({r // 16}, {c // 16})"
    if what in ("forward", "back"):
        return f"row {i}: camera {i // dim}, panel {i // 64}, block {i // 256}"
    return f"camera {i // (dim * dim)}, entry {i % (dim * dim)} (n_obs = {int(sy.p.n_c[min(i // (dim * dim), sy.p.n_cams - 1)])})"


def check_case(ctx, sy, inc, label):
    """Every assertion of the module docstring on one solved context; returns {check: worst err / bound}."""
    from povar_amd import capi
    p, n, N, dim = sy.p, sy.n, sy.N, sy.dim
    bd = ctx.get_buffer(capi.BUF_SC_BLOCKDIAG, joint=sy.joint).reshape(-1, dim, dim)
    X = ctx.get_buffer(capi.BUF_SC_PRECOND, joint=sy.joint).reshape(-1, dim, dim)
    buf = ctx.get_buffer(capi.BUF_SC_FACTOR, joint=sy.joint)
    assert buf.shape == (N, N + 2) and np.all(np.isfinite(bd)) and np.all(np.isfinite(X))
    checks = {"blockdiag": (np.abs((bd - sy.B).astype(F)), sy.EB)}
    res, Rb, asym, ab = SB.precond_check(sy, X)
    checks["precond"], checks["precond_sym"] = (res, Rb), (asym, ab)
    fc = SB.factor_check(sy, buf, bd)
    pad = fc.pop("padding")
    checks.update(fc)
    out, bad = {}, list(pad)
    for what, (err, bound) in checks.items():
        r, i, over = SB.worst(err, bound)
        out[what] = r
        if over:
            bad.append(f"{what}: {over} entries over their bound, the worst err / bound = {r:.3g} at {_where(sy, what, i)}")
    print(f"SCBOUND {label} " + " ".join(f"{k}={v:.3g}" for k, v in out.items()))
    assert not bad, "\n".join(bad)
    assert np.array_equal(inc, buf[:n, N + 1]), "inc is not x[:n] bit for bit"
    # the cameras nobody observes: B_c = lambda I, S_cc^-1 = I / lambda to gamma_3, a zero step
    for c in np.flatnonzero(p.n_c == 0):
        assert np.array_equal(bd[c], p.lam * np.eye(dim)) and np.all(inc[dim * c:dim * c + dim] == 0.0), c
        off = X[c] - np.diag(np.diag(X[c]))
        assert np.all(off == 0.0) and np.all(np.abs(np.diag(X[c]) * p.lam - 1) <= SB.g(3)), c
    return out


# (shape, robust, lambda, family)
CASES = [(s, r, lam, "auto") for s in ("pose-5", "joint-small") for r in ("NONE", "HUBER") for lam in T.LAMS]
CASES += [("pose-5", "HUBER", SB.LAM, "lpl"), ("joint-small", "HUBER", SB.LAM, "lpl"),
          ("pose-16", "NONE", SB.LAM, "auto"), ("pose-16", "HUBER", 1.0, "auto"),
          ("pose-26", "NONE", SB.LAM, "auto"), ("pose-26", "NONE", 1.0, "lpl"),
          ("pose-medium", "NONE", SB.LAM, "auto"), ("pose-medium", "NONE", 1.0, "lpl"),
          ("joint-29", "NONE", SB.LAM, "auto"), ("joint-29", "NONE", 1.0, "lpl"),
          ("joint-64", "NONE", SB.LAM, "auto"), ("joint-64", "NONE", 1.0, "lpl"),
          ("pose-edge", "NONE", SB.LAM, "auto"), ("pose-edge", "HUBER", SB.LAM, "lpl"),
          ("joint-edge", "NONE", SB.LAM, "auto"), ("joint-edge", "HUBER", SB.LAM, "lpl")]


@pytest.mark.parametrize("name,robust,lam,fam", CASES, ids=["-".join([s, r, f"{lam:g}", f]) for s, r, lam, f in CASES])
def test_explicit_sc_within_componentwise_bounds(monkeypatch, name, robust, lam, fam):
    if name.endswith("edge") and robust == "HUBER":  # (not kept by the CPU module: its conditions are asserted there)
        step, make = T.SHAPES[name]
        sy = _REF.setdefault((name, robust, lam, 1), SB.dense_system(make(robust, lam), step == 2))
    else:
        sy = _reference(name, robust, lam)
    ctx = _context(monkeypatch, fam, sy.p)
    inc = _solve(ctx, sy)
    if fam == "lpl":
        assert ctx.layout_info().lane_per_landmark == 1
    if robust == "HUBER":
        assert (sy.R.aux["w"] < 1).any(), "the robust norm down-weights nothing on this case"
    check_case(ctx, sy, inc, f"{name}/{robust}/lam={lam:g}/{fam}")
    ctx.close()


def test_two_shards_over_the_host_all_reduce():
    """Two landmark shards in one process (the pattern of test_richolesky_sharded_matches_single): each shard assembles its
    landmarks' part of S, B_c / rhs / padding come from rank 0, the matrix is all-reduced and every rank factors it: every
    rank's buffers are held to the bounds of the whole problem with one more rounding per entry."""
    from povar_amd import capi
    import test_gpu_joint_cholesky as J
    sy = _reference("joint-29", "NONE", SB.LAM, shards=2)
    p = sy.p
    world = 2
    ar = J.HostAllReduce(world)
    out, err = [None] * world, [None] * world

    def worker(rank):
        try:
            lb, le = capi.shard_range(p.lm_off, world, rank)
            ob, oe = int(p.lm_off[lb]), int(p.lm_off[le])
            ctx = capi.Context(p.n_cams, p.lm_off[lb:le + 1] - p.lm_off[lb], p.cam_idx[ob:oe], p.obs[ob:oe], e0_mode=0)
            ctx.comm_init_host(world, rank, ar.fn(rank))
            inc = _solve(ctx, sy, p.lms[lb:le])
            bufs = [ctx.get_buffer(b, joint=True) for b in (capi.BUF_SC_BLOCKDIAG, capi.BUF_SC_PRECOND, capi.BUF_SC_FACTOR)]
            ctx.close()
            out[rank] = (inc, bufs)
        except BaseException as e:  # noqa: BLE001 (reported by the main thread)
            err[rank] = e
            ar.bar.abort()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert err == [None] * world, err

    class Held:  # (check_case reads a context: hand it the buffers a rank exported)
        def __init__(self, bufs):
            self.bufs = dict(zip((capi.BUF_SC_BLOCKDIAG, capi.BUF_SC_PRECOND, capi.BUF_SC_FACTOR), bufs))

        def get_buffer(self, which, joint=False):
            return self.bufs[which]

    for rank in range(world):
        inc, bufs = out[rank]
        check_case(Held(bufs), sy, inc, f"joint-29/NONE/two-shards/rank{rank}")
    assert np.array_equal(out[0][1][2], out[1][1][2])  # (the same all-reduced matrix, factored by the same kernels)


def test_the_factor_buffer_names_its_preconditions(monkeypatch):
    """An argument error before any direct solve, after a PCG-only solve on a fresh context, after a covariance call (R has
    become R^-1) and after a failed factorisation; PCG and the power series leave a factor in place; a later power-series
    solve still works."""
    from povar_amd import capi
    sy = _reference("pose-5", "NONE", SB.LAM)
    p = sy.p
    ctx = _context(monkeypatch, "auto", p)
    ctx.set_cameras(p.cams)
    ctx.set_landmarks(p.lms)
    ctx.set_jl_col_scaling(False)
    assert ctx.linearize_pose(p.alpha)
    with pytest.raises(capi.PovarError, match="POVAR_BUF_SC_FACTOR"):
        ctx.get_buffer(capi.BUF_SC_FACTOR)
    inc_p, it, st, rc = ctx.solve_pose_sc(p.lam, capi.SC_PCG, 0, 500, 1e-2)
    assert rc == 0
    with pytest.raises(capi.PovarError, match="POVAR_BUF_SC_FACTOR"):
        ctx.get_buffer(capi.BUF_SC_FACTOR)
    inc, it, st, rc = ctx.solve_pose_sc(p.lam, capi.SC_CHOLESKY)
    assert rc == 0
    buf = ctx.get_buffer(capi.BUF_SC_FACTOR)
    # PCG and the power series do not write the dense matrix: the factor stays
    assert ctx.solve_pose_sc(p.lam, capi.SC_PCG, 0, 500, 1e-2)[3] == 0
    assert np.all(np.isfinite(ctx.solve_pose(p.lam, capi.POWER_VARPROJ, 5)[0]))
    assert np.array_equal(ctx.get_buffer(capi.BUF_SC_FACTOR), buf)
    cov, rc = ctx.camera_covariance(1, p.lam, capi.COV_DAMPED, capi.COV_SOLVER_COORDS)
    assert rc == 0
    with pytest.raises(capi.PovarError, match="POVAR_BUF_SC_FACTOR"):
        ctx.get_buffer(capi.BUF_SC_FACTOR)
    assert ctx.solve_pose_sc(p.lam, capi.SC_CHOLESKY)[3] == 0
    assert ctx.get_buffer(capi.BUF_SC_FACTOR).shape == buf.shape
    # a failed factorisation: lambda = -2 leaves no positive pivot in the Jacobi-scaled system
    inc_f, it, st, rc = ctx.solve_pose_sc(-2.0, capi.SC_CHOLESKY)
    assert rc == capi.NUMERIC_FAILURE and np.all(np.isnan(inc_f))
    with pytest.raises(capi.PovarError, match="POVAR_BUF_SC_FACTOR"):
        ctx.get_buffer(capi.BUF_SC_FACTOR)
    inc_s = ctx.solve_pose(p.lam, capi.POWER_VARPROJ, 20)[0]
    assert np.all(np.isfinite(inc_s)) and np.linalg.norm(inc_s - inc) < np.linalg.norm(inc)
    ctx.close()
