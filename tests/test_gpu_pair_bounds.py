"""The covariance blocks of parameter pairs (povar_covariance_blocks_pose / _joint: pair_cc, pair_cl, pair_ll) held entry by
entry to the condition-free bounds of tests/pair_bounds.py, on the device's own intermediates (povar_set_cov_inspect,
POVAR_BUF_COV_FACTOR / _INVERSE / _PANEL / _GAUGE as the call leaves them: the state of a landmark call):
    pair_cc   every entry of every camera-camera block against C[a, b] - Q_a Q_b^T          (damped, solver coordinates: bit for bit)
    pair_cl   every entry of every camera-landmark block against -sum_j C[c, c_j] W_j + Q_c T_l, in both request orders
    pair_ll   every entry of every landmark-landmark block against delta_lm Hll^-1 + sum_ij W_i^T C[c_i, c_j] W_j - T_l^T T_m
with C as cov_at reads it and Q of the block's own call, in both coordinate systems; the exact facts of pair_bounds.pair_check
(finite, (b, a) the bitwise transpose of (a, b), (a, a) symmetric, duplicates the same bits, a zero bound means the
reference's value, no entry skipped).  Each case makes one covariance_blocks call per coordinate system and also runs the
assembly, gauge, span, inverse and lauum checks of tests/cov_bounds.py on the buffers of that call.  err <= bound on every
entry; no bound is tuned to what is measured.  tests/test_pair_bounds.py shows on the CPU that the bounds are satisfiable on
these requests and report the defects they are meant for; tests/test_gpu_pair_covariance.py stays the independent end-to-end
route through the full matrix K.

Requests (pair_bounds.case_pairs): small: all 36 camera pairs, the 240 camera-landmark pairs in both orders, the 1 600
landmark pairs, 40 duplicates, shuffled (camera 5 straddles column 64); tracks (66 cameras, tracks of 2, 15-17, 31-33, 63-65):
the 100 ordered pairs of the ten edge-length landmarks, those ten with cameras 0, 5, 65 in both orders, the camera pairs among
{0, 4, 5, 6, 65}; long: the two landmarks of >= 65 observations with each other and themselves, the three of 33..64 against
them, a seeded 100 of each kind; medium (lambda = 1): a seeded 200 of each kind; p22 on two shards: a seeded 60 of each kind per rank.
Every case prints "COVBOUND ..." with its worst err / bound per check before it asserts.

Measured on an MI355X when these tests were written (largest err / bound per check over the two calls of a case; for
information, no bound is tuned by them):
  (s = solver, p = parameter coordinates)
  case                          assembly  gauge   span     inverse  lauum   cc s   cc p    cl s     cl p     ll s     ll p
  small step 1, free            0.020     0.032   3.7e-5   0.89     0.054   0.81   0.083   0.0097   0.0072   0.0057   0.0037
  small step 1, lambda 1e-4     0.0087    -       -        0.94     0.044   0      0.088   0.0098   0.0097   0.0049   0.0040
  small step 2, free            0.0035    0.098   6.9e-4   0.88     0.066   0.92   0.038   0.0011   0.0013   3.4e-4   2.6e-4
  small step 2, lambda 1e-4     0.0066    -       -        0.90     0.030   0      0.037   0.0012   0.0021   2.9e-4   2.2e-4
  small HUBER step 1            0.035     0.038   3.8e-5   0.86     0.073   0.75   0.082   0.0035   0.0036   0.0014   0.0010
  small HUBER step 2            0.0042    0.094   6.7e-4   0.93     0.051   0.86   0.038   0.0019   0.0012   4.7e-4   5.2e-4
  tracks step 1, free           0.040     0.0089  5.1e-5   0.97     0.11    0.86   0.14    6.7e-4   0.0011   1.2e-4   1.3e-4
  tracks step 2, free           0.037     0.023   3.6e-4   0.96     0.10    0.93   0.044   5.1e-4   5.4e-4   4.9e-5   4.0e-5
  long step 1, free             0.040     0.0063  3.1e-5   0.96     0.11    0.52   0.078   0.0070   0.0047   5.6e-4   5.1e-4
  long step 2, free             0.013     0.015   2.6e-4   0.95     0.11    0.94   0.051   8.3e-4   6.4e-4   9.8e-5   5.1e-5
  medium step 1, lambda 1       0.30      -       -        0.87     0.097   0      0.18    0.010    0.0073   0.0022   0.0016
  medium step 2, lambda 1       0.30      -       -        0.79     0.11    0      0.048   0.0038   0.0039   0.0015   5.4e-4
  small lane-per-landmark 1     0.041     0.032   3.7e-5   0.89     0.055   0.81   0.091   0.0093   0.0069   0.0043   0.0050
  small lane-per-landmark 2     0.0036    0.098   6.9e-4   0.92     0.062   0.92   0.036   0.0012   0.0015   3.7e-4   2.8e-4
  p22 step 2, two shards        0.013     0.039   4.9e-4   0.96     0.13    0.93   0.036   0.0012   8.7e-4   4.8e-4   3.6e-4
  small deterministic 1 / 2     0.017     0.098   6.9e-4   0.91     0.047   0.89   -       1.6e-4   -        0.0065   -
and in the deterministic context |pair(c, c) - camera(c)| reached 0.047 and |pair(l, l) - landmark(l)| 0.0014 of the summed bounds.
The slowest case took 1.6 s (long, step 2), the module 11 s.  The fp64 emulations of tests/test_pair_bounds.py land on the same
figures.  No case exposed a defect: the kernels are unchanged.  (A scratch build of pair_cl without the `accp` merge, run once
when this was written: pair_cl over its bound on exactly the 13 140 entries of `small` that pair_bounds.mutations_pairs lists for
cl_no_merge, in both coordinate systems, worst 1e13 times the bound, every other check clean.)
pair_cc sits next to 1 by nature in the free gauge's solver coordinates (one rounding of C against a bound of one rounding);
pair_cl and pair_ll are carried by the operand bounds of sigma, Hll^-1 and the column scales, as landmark's are.
"""
import threading

import numpy as np
import pytest

import cov_bounds as CB
import pair_bounds as PB
import pair_covariance_reference as P
import sc_bounds as SB
from test_gpu_cov_bounds import _buffers, _context, _linearise

pytestmark = pytest.mark.gpu
F = np.float64
CAM, LM = P.CAMERA, P.LANDMARK
STAGES = {"assembly", "inverse", "lauum"}


def check_pair_call(ctx, sy, pairs, coords, label, want_pairs=None):
    """One covariance_blocks call, the four buffers it leaves, the stage checks of cov_bounds on them and pair_check on every
    block against the C and Q of this call.  want_pairs: the same pairs with the ids `sy` knows them by (a shard's landmarks).
    Returns (blocks, pair_check's result, the buffers)."""
    p = sy.p
    free = p.lam == 0.0
    got, rc = ctx.covariance_blocks(pairs, step=2 if sy.joint else 1, lam=p.lam, gauge=0 if free else 1, coords=coords)
    assert rc == 0 and len(got) == len(pairs), label
    d = _buffers(ctx, sy, free)
    out, bad = CB.check_all(sy, d)
    assert STAGES <= set(out) and ("gauge" in out and "span" in out) == free
    res = PB.pair_check(sy, CB.c_symmetric(d["inv"], d["panel"]), d["Q"], pairs if want_pairs is None else want_pairs, got, coords)
    total = int(PB.layout(pairs, sy.dim, coords)[1][-1])
    assert all(res[k][0].shape == (total,) for k in PB.CHECKS)  # none skipped (and pair_check's own count of every entry)
    bad = bad + res["exact"]
    out.update({k: res[k] for k in PB.CHECKS})
    PB.report(f"{label} coords {coords}", out, bad)
    return got, res, d


def _id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-{c[3]:g}"


@pytest.mark.parametrize("name,step,robust,lam", PB.PAIR_CASES, ids=[_id(c) for c in PB.PAIR_CASES])
def test_pair_blocks_within_componentwise_bounds(name, step, robust, lam):
    sy = CB.system(name, step, robust, lam)
    pairs = PB.case_pairs(name, sy.p, step)
    ctx = _context(sy)
    for coords in (1, 0):
        got, res, d = check_pair_call(ctx, sy, pairs, coords, f"{name} step {step} {robust} lambda {lam:g} pairs")
        if lam > 0 and coords == 1:  # damped, solver coordinates: the camera-camera blocks are C's entries bit for bit
            Cs, dim = CB.c_symmetric(d["inv"], d["panel"]), sy.dim
            assert not np.any(res["pair_cc"][1])
            n_cc = 0
            for (ka, a, kb, b), blk in zip(pairs, got):
                if ka == kb == CAM:
                    assert np.array_equal(blk, Cs[dim * a:dim * a + dim, dim * b:dim * b + dim]), (a, b)
                    n_cc += 1
            assert n_cc >= 36
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_pair_blocks_after_a_lane_per_landmark_linearisation(step, monkeypatch):
    """POVAR_E0_V1=0: the per-slot arrays the staging of pair_cl and pair_ll reads come from the lane-per-landmark linearisation."""
    monkeypatch.setenv("POVAR_E0_V1", "0")
    sy = CB.system("small", step, "NONE", 0.0)
    ctx = _context(sy)
    assert ctx.layout_info().lane_per_landmark == 1
    pairs = PB.case_pairs("small", sy.p, step)
    for coords in (1, 0):
        check_pair_call(ctx, sy, pairs, coords, f"small step {step} lane-per-landmark pairs")
    ctx.close()


def test_pair_blocks_of_two_shards():
    """p22, step 2, two shard contexts through the host all-reduce hook: every rank requests pairs of its own landmarks (ids of
    its shard) and any cameras; each rank's blocks against the buffers of its own context, the shard-local landmark ids mapped
    to the problem's as tests/test_gpu_pair_covariance.py::test_sharded_matches_single maps them."""
    from povar_amd import capi
    from test_gpu_sharded import HostAllReduce
    step = 2
    p = CB.case_problem("p22", step, "NONE", 0.0)
    sy = SB.dense_system(p, True, shards=2, R=CB.system("p22", step, "NONE", 0.0).R)
    world = 2
    ar = HostAllReduce(world)
    out = [None] * world

    def worker(rank):
        try:
            lb, le = capi.shard_range(p.lm_off, world, rank)
            ob, oe = int(p.lm_off[lb]), int(p.lm_off[le])
            ctx = capi.Context(p.n_cams, p.lm_off[lb:le + 1] - p.lm_off[lb], p.cam_idx[ob:oe], p.obs[ob:oe])
            ctx.comm_init_host(world, rank, ar.fn(rank))
            ctx.set_cov_inspect(True)
            _linearise(ctx, sy, p.lms[lb:le])
            cc, cl, ll = P.sample_pairs(np.random.default_rng(40 + rank), p.n_cams, le - lb, 60)
            pairs = cc + cl + ll + [(LM, 0, LM, 0), (CAM, 3, LM, 1), (LM, 1, CAM, 3), (LM, 2, LM, 5), (LM, 5, LM, 2)]
            res = []
            for coords in (1, 0):
                got, rc = ctx.covariance_blocks(pairs, step=step, lam=0.0, gauge=0, coords=coords)
                res.append((coords, rc, got, _buffers(ctx, sy, True)))
            out[rank] = (lb, le, pairs, res)
            ctx.close()
        except BaseException:
            ar.bar.abort()  # a failed rank must not leave the other one waiting
            raise

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert all(o is not None for o in out)
    for rank, (lb, le, pairs, res) in enumerate(out):
        glob = [(ka, a + (lb if ka == LM else 0), kb, b + (lb if kb == LM else 0)) for ka, a, kb, b in pairs]
        assert all(lb <= a < le for ka, a, _, _ in glob if ka == LM) and all(lb <= b < le for _, _, kb, b in glob if kb == LM)
        for coords, rc, got, d in res:
            assert rc == 0
            o, bad = CB.check_all(sy, d)
            r = PB.pair_check(sy, CB.c_symmetric(d["inv"], d["panel"]), d["Q"], glob, got, coords)
            o.update({k: r[k] for k in PB.CHECKS})
            PB.report(f"p22 step {step} two shards rank {rank} pairs coords {coords}", o, bad + r["exact"])


@pytest.mark.parametrize("step", [1, 2])
def test_deterministic_context_ties_the_diagonal_to_the_older_calls(step):
    """POVAR_FLAG_DETERMINISTIC: a pair call, a landmark call and a camera call read the same bits of C.  With every check's
    reference formed from that one C (camera_check's from W: cov_lauum's bound on the block's entries of C is added),
        |pair(l, l) - landmark(l)| <= bound_pair + bound_landmark,   |pair(c, c) - camera(c)| <= bound_pair + bound_camera + bound_lauum
    entry by entry: the diagonal of the new call is tied to the two older calls without a condition number."""
    from povar_amd import capi
    sy = CB.system("small", step, "NONE", 0.0)
    p, dim = sy.p, sy.dim
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=p.robust, huber=p.huber, eps=p.eps, flags=capi.FLAG_DETERMINISTIC)
    ctx.set_cov_inspect(True)
    _linearise(ctx, sy)
    pairs = [(CAM, c, CAM, c) for c in range(p.n_cams)] + [(LM, l, LM, l) for l in range(p.n_lms)] + [(CAM, 5, LM, 0), (LM, 3, LM, 7)]
    got, res, d = check_pair_call(ctx, sy, pairs, 1, f"small step {step} deterministic pairs")
    assert ctx.sc_assembly() == 2
    lm, cam, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=1, with_cameras=True)
    assert rc == 0
    d2 = _buffers(ctx, sy, True)
    for k in ("R", "inv", "panel", "Q"):
        assert np.array_equal(d[k], d2[k]), f"the landmark call left other bits in {k}"
    cam2, rc = ctx.camera_covariance(step=step, lam=0.0, gauge=0, coords=1)
    assert rc == 0 and np.array_equal(cam, cam2)
    Cs = CB.c_symmetric(d["inv"], d["panel"])[:sy.n, :sy.n]
    b_lm = CB.landmark_check(sy, Cs, d["Q"], lm)
    b_cam = CB.camera_check(d["inv"], d["Q"], cam, sy.n, dim, 1, sy)
    b_lauum = CB.lauum_check(d["inv"], d["panel"])["lauum"][1]
    b_lauum = np.maximum(b_lauum, b_lauum.T)  # (cov_at reads the lower triangle for either order)
    assert not b_lm["exact"] and not b_cam["exact"] and not CB.flagged(*b_lm["landmark"]) and not CB.flagged(*b_cam["camera"])
    _, off = PB.layout(pairs, dim, 1)
    worst_c = worst_l = 0.0
    for c in range(p.n_cams):
        bp = res["pair_cc"][1][off[c]:off[c + 1]].reshape(dim, dim)
        room = bp + b_cam["camera"][1][c] + b_lauum[dim * c:dim * c + dim, dim * c:dim * c + dim]
        gap = np.abs(got[c] - cam[c])
        worst_c = max(worst_c, float((gap / room).max()))
        assert np.all(gap <= room), (c, float((gap / room).max()))
    for l in range(p.n_lms):
        t = p.n_cams + l
        room = res["pair_ll"][1][off[t]:off[t + 1]].reshape(3, 3) + b_lm["landmark"][1][l]
        gap = np.abs(got[t] - lm[l])
        worst_l = max(worst_l, float((gap / room).max()))
        assert np.all(gap <= room), (l, float((gap / room).max()))
    print(f"COVBOUND small step {step} deterministic: |pair(c, c) - camera(c)| {worst_c:.3g}, |pair(l, l) - landmark(l)| {worst_l:.3g} of the summed bounds")
    ctx.close()
