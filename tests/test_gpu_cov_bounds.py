"""The covariance path held, stage by stage and entry by entry, to the condition-free bounds of tests/cov_bounds.py, on the
device's own intermediates (povar_set_cov_inspect, POVAR_BUF_COV_FACTOR / _INVERSE / _PANEL / _GAUGE):
    assembly  |S_ref(lambda) + Q Q^T - R^T R|   the kept factor against sc_bounds.dense_system at the call's lambda
    gauge     |Q^T Q - I| and the span of the long-double generators
    inverse   |W R - I|, zeros below the diagonal of W's diagonal blocks, identity padding
    camera    every entry of every camera block against (W W^T)_cc - Q_J Q_J^T, in both coordinate systems
    lauum     every entry of C (strictly lower 64 x 64 blocks and the panel) against W W^T
    landmark  every entry of every requested landmark block against Hll^-1 + sum G^T K G - T^T T from C as cov_at reads it
    observation_h / _c  every entry of every row (h; c_uu, c_uv, c_vv) of an observation call against K_ii - R L^T - L R^T +
              L Sigma_l L^T from the C of that call, Sigma_l without the gauge correction (obs_cov, the last kernel of the path)
Each case makes one landmark call with the camera blocks in each coordinate system, reads the four buffers and runs all six
checks; err <= bound on every entry, an entry whose bound is zero is exactly zero, none is skipped.  That cov_lauum leaves W
alone bit for bit is seen in the two-shard case: both ranks invert the same all-reduced matrix, one stops before cov_lauum,
the other runs it, and their upper block triangles agree bitwise (two calls of one context cannot be compared so: the
assembly adds with atomics).  The observation tests make one observation call for all landmarks, run the assembly, gauge,
inverse and lauum checks on the buffers it leaves (as a landmark call does) and every row against the C of its own call,
then an id list in reversed order with one landmark twice (the same bits).  tests/test_cov_bounds.py shows on the CPU that
the bounds are satisfiable on every shape used here and that they report the defects they are meant for.

Shapes (landmark_covariance_reference.problem): small N = 128 (camera 5 straddles column 64), p22 step 2 N = 256 (ends on the
outer block), p24 N = 320 (five block rows), medium N = 640 / 576 (damped; ten K steps of cov_lauum), long N = 832 / 768 (both
chunk loops of lm_cov repeat); the observation rows: small, medium and tracks N = 832 / 768 (66 cameras, tracks of 2, 15, 16,
17, 31, 32, 33, 63, 64, 65: every loop edge of obs_cov in both steps).  Every case prints "COVBOUND ..." with its worst
err / bound per check before it asserts.

Measured on an MI355X when these tests were written (largest err / bound per check over the calls of a case; for information,
no bound is tuned by them):
  case                          assembly  gauge   span     inverse  camera  lauum   landmark
  small step 1, free            0.025     0.032   3.7e-5   0.92     0.23    0.051   0.0042
  small step 1, lambda 1e-4     0.0075    -       -        0.91     0.25    0.054   0.0042
  small step 2, free            0.0035    0.098   6.9e-4   0.92     0.18    0.041   0.00034
  small step 2, lambda 1e-4     0.0056    -       -        0.90     0.22    0.043   0.00028
  p22 step 2, free              0.015     0.034   4.2e-4   0.94     0.32    0.13    0.0011
  p24 step 1 / 2, free          0.037     0.043   4.9e-4   0.98     0.35    0.11    0.0077
  medium step 1, 1e-4 / 1       0.30      -       -        0.97     0.44    0.14    0.011
  medium step 2, 1e-4 / 1       0.30      -       -        0.97     0.44    0.12    0.0049
  long step 1 / 2, free         0.041     0.015   2.6e-4   0.95     0.42    0.12    0.0058
  small HUBER step 1 / 2        0.043     0.094   6.7e-4   0.95     0.20    0.062   0.0013
  small lane-per-landmark       0.023     0.098   6.9e-4   0.93     0.23    0.062   0.0043
  p22 step 2, two shards        0.013     0.039   4.9e-4   0.96     0.36    0.13    0.0014
The observation calls (largest over the all-landmark call and the id list; the assembly ... lauum figures of their buffers are
those of the rows above, on tracks 0.038, 0.023, 3.6e-4, 0.96, -, 0.094):
  case                          observation_h  observation_c
  small step 1, free            0.00099        0.0020
  small step 1, lambda 1e-4     0.00061        0.00070
  small step 2, free            0.00031        0.00026
  small step 2, lambda 1e-4     5.7e-5         7.1e-5
  small HUBER step 1 / 2        0.00035        0.0010
  medium step 1, 1e-4 / 1       0.0061         0.0090
  medium step 2, 1e-4 / 1       0.0032         0.0072
  tracks step 1, free           0.0017         0.0054
  tracks step 2, free           0.00043        0.0011
  small lane-per-landmark       0.00090        0.0015
  p22 step 2, two shards        0.0010         0.0011
(the operand bounds of sigma, Hll^-1 and the column scales carry them, as they carry landmark's).
inverse sits next to 1 by nature: the entries next to the diagonal of a diagonal block pass one or two roundings and the bound
is g(1).  assembly's 0.30 is medium at lambda = 1, as in tests/test_gpu_sc_bounds.py.  The fp64 emulations of
tests/test_cov_bounds.py land on the same figures.  No case exposed a defect: the kernels are unchanged.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import cov_bounds as CB
import sc_bounds as SB

pytestmark = pytest.mark.gpu
F = np.float64


def _linearise(ctx, sy, lms=None):
    p = sy.p
    ctx.set_cameras(p.cams)
    if sy.joint:
        ctx.set_landmarks_homogeneous(p.lms if lms is None else lms)
        assert ctx.linearize_homogeneous()
    else:
        ctx.set_landmarks(p.lms if lms is None else lms)
        assert ctx.linearize_pose(p.alpha)


def _context(sy):
    from povar_amd import capi
    p = sy.p
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=p.robust, huber=p.huber, eps=p.eps)
    ctx.set_cov_inspect(True)
    _linearise(ctx, sy)
    return ctx


def _buffers(ctx, sy, free):
    from povar_amd import capi
    j = sy.joint
    d = dict(R=ctx.get_buffer(capi.BUF_COV_FACTOR, joint=j), inv=ctx.get_buffer(capi.BUF_COV_INVERSE, joint=j),
             panel=ctx.get_buffer(capi.BUF_COV_PANEL, joint=j), Q=ctx.get_buffer(capi.BUF_COV_GAUGE, joint=j) if free else None)
    if not free:
        with pytest.raises(capi.PovarError, match="POVAR_BUF_COV_GAUGE"):
            ctx.get_buffer(capi.BUF_COV_GAUGE, joint=j)
    return d


def check_call(ctx, sy, coords, label, ids=None):
    """One landmark call with the camera blocks, the four buffers, all six checks; {check: worst err / bound}."""
    p = sy.p
    free = p.lam == 0.0
    lm, cam, rc = ctx.landmark_covariance(step=2 if sy.joint else 1, lam=p.lam, gauge=0 if free else 1, coords=coords, ids=ids,
                                          with_cameras=True)
    assert rc == 0, label
    d = _buffers(ctx, sy, free)
    d.update(cam=cam, lm=lm)
    out, bad = CB.check_all(sy, d, coords=coords, ids=ids)
    CB.report(f"{label} coords {coords}", out, bad)
    return {k: CB.worst(*v)[0] for k, v in out.items()}


def _id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-{c[3]:g}"


@pytest.mark.parametrize("name,step,robust,lam", CB.CASES, ids=[_id(c) for c in CB.CASES])
def test_covariance_stages_within_componentwise_bounds(name, step, robust, lam):
    sy = CB.system(name, step, robust, lam)
    ctx = _context(sy)
    for coords in (1, 0):
        check_call(ctx, sy, coords, f"{name} step {step} {robust} lambda {lam:g}")
    # a shuffled subset with a duplicate: each requested block against its own landmark, from the C of its own call
    from povar_amd import capi
    rng = np.random.default_rng(step)
    ids = np.r_[rng.permutation(sy.p.n_lms)[:5], 0, 0]
    free = lam == 0.0
    lm, rc = ctx.landmark_covariance(step=step, lam=lam, gauge=0 if free else 1, coords=1, ids=ids)
    assert rc == 0
    Cs = CB.c_symmetric(ctx.get_buffer(capi.BUF_COV_INVERSE, joint=sy.joint), ctx.get_buffer(capi.BUF_COV_PANEL, joint=sy.joint))
    res = CB.landmark_check(sy, Cs[:sy.n, :sy.n], ctx.get_buffer(capi.BUF_COV_GAUGE, joint=sy.joint) if free else None, lm, ids, 1)
    CB.report(f"{name} step {step} {robust} lambda {lam:g} subset", {"landmark": res["landmark"]}, res["exact"])
    assert np.array_equal(lm[5], lm[6])  # given C a block is reproducible
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_after_a_lane_per_landmark_linearisation(step, monkeypatch):
    """POVAR_E0_V1=0: the per-slot arrays the staging reads come from the lane-per-landmark linearisation (ensure_legacy)."""
    monkeypatch.setenv("POVAR_E0_V1", "0")
    sy = CB.system("small", step, "NONE", 0.0)
    ctx = _context(sy)
    assert ctx.layout_info().lane_per_landmark == 1
    for coords in (1, 0):
        check_call(ctx, sy, coords, f"small step {step} lane-per-landmark")
    ctx.close()


@pytest.mark.parametrize("step", [2])
def test_two_shards_add_the_gauge_term_once(step):
    """p22 on two shard contexts through the host all-reduce hook: Q Q^T enters the all-reduced matrix once (a second copy
    would be an error of order one in ASSEMBLY), every rank inverts the all-reduced matrix and answers for its own landmarks."""
    from povar_amd import capi
    from test_gpu_sharded import HostAllReduce
    p = CB.case_problem("p22", step, "NONE", 0.0)
    sy = SB.dense_system(p, step == 2, shards=2, R=CB.system("p22", step, "NONE", 0.0).R)
    world = 2
    ar = HostAllReduce(world)
    out, w_after = [None] * world, [None] * world

    def worker(rank):
        try:
            lb, le = capi.shard_range(p.lm_off, world, rank)
            ob, oe = int(p.lm_off[lb]), int(p.lm_off[le])
            ctx = capi.Context(p.n_cams, p.lm_off[lb:le + 1] - p.lm_off[lb], p.cam_idx[ob:oe], p.obs[ob:oe])
            ctx.comm_init_host(world, rank, ar.fn(rank))
            ctx.set_cov_inspect(True)
            _linearise(ctx, sy, p.lms[lb:le])
            res = []
            for coords in (1, 0):
                lm, cam, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=coords, with_cameras=True)
                d = _buffers(ctx, sy, True)
                d.update(cam=cam, lm=lm)
                res.append((coords, rc, d))
            # one more collective call on the same all-reduced matrix: rank 0 asks for no landmark (cov_lauum does not run),
            # rank 1 for all of its own
            ids = np.zeros(0, dtype=np.int32) if rank == 0 else None
            _, _, rc = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=1, ids=ids, with_cameras=True)
            assert rc == 0
            w_after[rank] = (ctx.get_buffer(capi.BUF_COV_FACTOR, joint=sy.joint), ctx.get_buffer(capi.BUF_COV_INVERSE, joint=sy.joint))
            out[rank] = (lb, le, res)
            ctx.close()
        except BaseException:
            ar.bar.abort()  # a failed rank must not leave the other one waiting
            raise

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert all(o is not None for o in out)
    covered = 0
    for rank, (lb, le, res) in enumerate(out):
        for coords, rc, d in res:
            assert rc == 0
            o, bad = CB.check_all(sy, d, coords=coords, ids=np.arange(lb, le))
            CB.report(f"p22 step {step} two shards rank {rank} coords {coords}", o, bad)
        covered += le - lb
    assert covered == p.n_lms
    # W is unchanged, bit for bit, by the landmark part of a call: both ranks factor and invert the same all-reduced matrix
    # (no atomics after the all-reduce), rank 0 stopped before cov_lauum, rank 1 ran it and lm_cov
    blk = np.arange(sy.N) // 64
    up = blk[:, None] <= blk[None, :]
    assert np.array_equal(np.triu(w_after[0][0]), np.triu(w_after[1][0])), "the two ranks hold different factors"
    assert np.array_equal(w_after[0][1][up], w_after[1][1][up]), "cov_lauum or lm_cov changed W"


def test_buffer_preconditions():
    """The switch off, a camera call against a landmark call, after a failure, after a direct solve; POVAR_BUF_SC_FACTOR's
    own rule is unchanged."""
    from povar_amd import capi
    cov = (capi.BUF_COV_FACTOR, capi.BUF_COV_INVERSE, capi.BUF_COV_PANEL, capi.BUF_COV_GAUGE)
    sy = CB.system("small", 1, "NONE", 0.0)
    p = sy.p
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    _linearise(ctx, sy)

    def refused(which, joint=False, c=None):
        with pytest.raises(capi.PovarError, match="POVAR_BUF_COV"):
            (c or ctx).get_buffer(which, joint=joint)

    for w in cov:  # no call yet
        refused(w)
    bytes0 = ctx.device_bytes()
    # the switch off (default): everything but the kept factor
    _, _, rc = ctx.landmark_covariance(step=1, lam=0.0, gauge=0, coords=1, with_cameras=True)
    assert rc == 0
    bytes_off = ctx.device_bytes()
    refused(capi.BUF_COV_FACTOR)
    inv, panel, Q = (ctx.get_buffer(w) for w in cov[1:])
    assert inv.shape == (128, 128) and panel.shape == (128, 64) and Q.shape == (72, 12)
    out = CB.lauum_check(inv, panel)
    assert CB.worst(*out["lauum"])[2] == 0
    # a second call with the switch off allocates nothing more; with it on: exactly the N x N copy
    _, _, rc = ctx.landmark_covariance(step=1, lam=0.0, gauge=0, coords=1, with_cameras=True)
    assert rc == 0 and ctx.device_bytes() == bytes_off > bytes0
    ctx.set_cov_inspect(True)
    _, rc = ctx.camera_covariance(step=1, lam=0.0, gauge=0, coords=1)
    assert rc == 0 and ctx.device_bytes() == bytes_off + 8 * 128 * 128
    # a camera call: R, W and Q, no panel; the lower blocks are unspecified and not looked at
    Rk, inv = ctx.get_buffer(capi.BUF_COV_FACTOR), ctx.get_buffer(capi.BUF_COV_INVERSE)
    assert ctx.get_buffer(capi.BUF_COV_GAUGE).shape == (72, 12)
    refused(capi.BUF_COV_PANEL)
    res = CB.inverse_check(Rk, inv, sy.n)
    assert not res["exact"] and CB.worst(*res["inverse"])[2] == 0
    # a landmark call without landmarks is a camera call
    _, _, rc = ctx.landmark_covariance(step=1, lam=0.0, gauge=0, coords=1, ids=np.zeros(0, dtype=np.int32), with_cameras=True)
    assert rc == 0
    refused(capi.BUF_COV_PANEL)
    # damped: no gauge basis
    _, rc = ctx.landmark_covariance(step=1, lam=1.0, gauge=1, coords=1)
    assert rc == 0 and ctx.get_buffer(capi.BUF_COV_PANEL).shape == (128, 64)
    refused(capi.BUF_COV_GAUGE)
    # switched off again: the copy of an earlier call is not handed out for this one
    ctx.set_cov_inspect(False)
    _, rc = ctx.landmark_covariance(step=1, lam=1.0, gauge=1, coords=1)
    assert rc == 0
    refused(capi.BUF_COV_FACTOR)
    ctx.get_buffer(capi.BUF_COV_INVERSE)
    # the solver's factor: an argument error after a covariance call, as before; a direct solve since ends the covariance buffers
    with pytest.raises(capi.PovarError, match="POVAR_BUF_SC_FACTOR"):
        ctx.get_buffer(capi.BUF_SC_FACTOR)
    inc, it, status, rc = ctx.solve_pose_sc(1e-4, capi.SC_CHOLESKY)
    assert rc == 0 and ctx.get_buffer(capi.BUF_SC_FACTOR).shape == (128, 130)
    for w in cov:
        refused(w)
    # an argument error of a covariance call leaves the buffers of the call before it
    ctx.set_cov_inspect(True)
    _, rc = ctx.landmark_covariance(step=1, lam=0.0, gauge=0, coords=1)
    assert rc == 0
    with pytest.raises(capi.PovarError):
        ctx.landmark_covariance(step=1, lam=1.0, gauge=capi.COV_FREE_GAUGE)
    assert ctx.get_buffer(capi.BUF_COV_FACTOR).shape == (128, 128)
    # wrong size
    bad = np.zeros(5)
    assert ctx.L.povar_get_buffer(ctx.h, C.c_int32(capi.BUF_COV_INVERSE), C.c_void_p(bad.ctypes.data), C.c_int64(5)) < 0
    ctx.close()
    # after a failure: medium in the free gauge is singular beyond its gauge
    sm = CB.system("medium", 1, "NONE", 1e-4)
    ctx = _context(sm)
    _, rc = ctx.landmark_covariance(step=1, lam=1e-4, gauge=1, coords=1)
    assert rc == 0 and ctx.get_buffer(capi.BUF_COV_FACTOR).shape == (640, 640)
    got, cam, rc = ctx.landmark_covariance(step=1, lam=0.0, gauge=0, coords=1, with_cameras=True)
    assert rc == capi.NUMERIC_FAILURE and np.all(np.isnan(got))
    for w in cov:
        refused(w, c=ctx)
    ctx.close()


# ======== OBSERVATION: the rows of povar_observation_covariance_* against the C of their own call
def check_observation_call(ctx, sy, label, ids=None, stages=True):
    """One observation call and the buffers it leaves (as a landmark call does: povar_cov.hip: cov_call): the assembly, gauge,
    inverse and lauum checks on them (stages) and every entry of every row against cov_bounds.observation_reference."""
    p = sy.p
    free = p.lam == 0.0
    rows, rc = ctx.observation_covariance(step=2 if sy.joint else 1, lam=p.lam, gauge=0 if free else 1, lm_ids=ids)
    assert rc == 0, label
    d = _buffers(ctx, sy, free)
    n_rows = len(p.cam_idx) if ids is None else int(p.n_l[np.asarray(ids)].sum())
    assert rows.shape == (n_rows, 4)
    if stages:
        d["obs"] = rows
        out, bad = CB.check_all(sy, d, ids=ids)
        assert {"assembly", "inverse", "lauum"} <= set(out) and ("gauge" in out and "span" in out) == free
    else:
        out = CB.observation_check(sy, CB.c_symmetric(d["inv"], d["panel"])[:sy.n, :sy.n], rows, ids)
        bad = out.pop("exact")
    assert out["observation_h"][0].shape == (n_rows,) and out["observation_c"][0].shape == (n_rows, 3)  # none skipped
    CB.report(label, out, bad)
    return rows


def _obs_id_list(p):
    """Reversed order, one landmark twice: row0 and ids index differently from the workgroup's number."""
    k = p.n_l
    pick = sorted({int(np.argmax(k)), int(np.argmin(k)), p.n_lms - 1, 0, int(np.flatnonzero(k >= 3)[0])})
    return np.array(pick[::-1] + [pick[-1]], dtype=np.int32)


@pytest.mark.parametrize("name,step,robust,lam", CB.OBS_CASES, ids=[_id(c) for c in CB.OBS_CASES])
def test_observation_rows_within_componentwise_bounds(name, step, robust, lam):
    sy = CB.system(name, step, robust, lam)
    p = sy.p
    ctx = _context(sy)
    label = f"{name} step {step} {robust} lambda {lam:g} observations"
    rows = check_observation_call(ctx, sy, label)
    # the id list: each row against its own landmark, from the C of its own call; a landmark asked for twice: the same bits
    ids = _obs_id_list(p)
    sub = check_observation_call(ctx, sy, label + " id list", ids, stages=False)
    start = np.r_[0, np.cumsum(p.n_l[ids])]
    assert ids[0] == ids[-1] and start[1] > 0
    assert np.array_equal(sub[start[0]:start[1]], sub[start[-2]:start[-1]])
    assert rows.shape[0] == len(p.cam_idx)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_observation_rows_after_a_lane_per_landmark_linearisation(step, monkeypatch):
    """POVAR_E0_V1=0: the per-slot arrays obs_cov's staging and its lane 0 read come from the lane-per-landmark linearisation."""
    monkeypatch.setenv("POVAR_E0_V1", "0")
    sy = CB.system("small", step, "NONE", 0.0)
    ctx = _context(sy)
    assert ctx.layout_info().lane_per_landmark == 1
    check_observation_call(ctx, sy, f"small step {step} lane-per-landmark observations")
    ctx.close()


def test_observation_rows_of_two_shards():
    """p22, step 2, two shard contexts through the host all-reduce hook: every rank inverts the all-reduced matrix and answers
    for the observations of its own landmarks; each rank's rows against the buffers of its own context."""
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
            rows, rc = ctx.observation_covariance(step=step, lam=0.0, gauge=0)
            d = _buffers(ctx, sy, True)
            d["obs"] = rows
            out[rank] = (lb, le, rc, d)
            ctx.close()
        except BaseException:
            ar.bar.abort()  # a failed rank must not leave the other one waiting
            raise

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert all(o is not None for o in out)
    covered = 0
    for rank, (lb, le, rc, d) in enumerate(out):
        assert rc == 0 and d["obs"].shape == (int(p.lm_off[le] - p.lm_off[lb]), 4)
        o, bad = CB.check_all(sy, d, ids=np.arange(lb, le))
        assert {"assembly", "gauge", "span", "inverse", "lauum", "observation_h", "observation_c"} <= set(o)
        CB.report(f"p22 step {step} two shards rank {rank} observations", o, bad)
        covered += le - lb
    assert covered == p.n_lms
