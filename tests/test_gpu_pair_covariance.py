"""Covariance blocks of parameter pairs (povar_covariance_blocks_pose / _joint) against the long-double reference of
tests/pair_covariance_reference.py, through the C ABI.

Tolerance, both modes, per block: |got - want|_F <= m u cond_2(K) |K^-1|_2 f_a f_b -- the bound of the landmark test
(landmark_covariance_reference.Reference.bound: K the full matrix that is actually inverted, m its dimension, u = 2^-53) with
f = 1 in solver coordinates and f_cam = max sigma, f_lm = max s in parameter coordinates.  tests/test_pair_covariance_reference.py
holds every case here to bound <= 1e-4 of its smallest diagonal block.  Every case prints its worst error in units of the bound;
the bound is not tightened to it.  This is the end-to-end route through the full matrix K; the entrywise, condition-free bound of
every block on the device's own C and Q is tests/pair_bounds.py (tests/test_pair_bounds.py, tests/test_gpu_pair_bounds.py).
"""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import covariance_reference as R
import landmark_covariance_reference as L
import pair_covariance_reference as P
from conftest import rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 1e-4
CAM, LM = P.CAMERA, P.LANDMARK


def _linearise(ctx, step, cams, lms):
    ctx.set_cameras(cams)
    if step == 1:
        ctx.set_landmarks(lms)
        assert ctx.linearize_pose(L.ALPHA)
    else:
        ctx.set_landmarks_homogeneous(lms)
        assert ctx.linearize_homogeneous()


def _context(name, step, norm="NONE", flags=0):
    from povar_amd import capi
    p = L.problem(name)
    cams, lms, obs = L.state(p, step)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs, robust_norm=norm, huber=L.HUBER[step], flags=flags)
    _linearise(ctx, step, cams, lms)
    return ctx


def _sides(step, coords):
    return {CAM: 11 if (step == 2 and coords == 1) else 12, LM: 4 if (step == 2 and coords == 0) else 3}


def _check(tag, ref, pairs, got, rc, coords, want_pairs=None):
    """Every block under the bound; the worst error in units of the bound.  want_pairs: the same pairs with the ids the
    reference knows them by (a shard's landmarks)."""
    assert rc == 0 and len(got) == len(pairs), tag
    side = _sides(ref.step, coords)
    worst = 0.0
    for k, (pair, blk) in enumerate(zip(pairs, got)):
        assert blk.shape == (side[pair[0]], side[pair[2]]) and np.all(np.isfinite(blk)), (tag, pair)
        wp = pair if want_pairs is None else want_pairs[k]
        err = float(np.linalg.norm((blk.astype(np.longdouble) - ref.want(wp, coords == 0)).astype(np.float64)))
        bound = ref.bound * ref.scale(wp, coords == 0)
        worst = max(worst, err / bound)
        assert err <= bound, (tag, pair, err, bound)
    print(f"{tag}: {len(pairs)} pairs, worst block error {worst:.3g} x the bound (m {ref.ref.m} x u cond |K^-1| = {ref.bound:.3e})")
    return worst


def _check_bits(tag, pairs, got):
    """(b, a) is the bitwise transpose of (a, b), (a, a) is symmetric bit for bit, duplicates are the same bits."""
    first = {}
    n_dup = n_tr = n_sym = 0
    for k, pair in enumerate(pairs):
        if pair in first:
            assert np.array_equal(got[k], got[first[pair]]), (tag, pair)
            n_dup += 1
        else:
            first[pair] = k
    for pair, k in first.items():
        back = (pair[2], pair[3], pair[0], pair[1])
        if back == pair:
            assert np.array_equal(got[k], got[k].T), (tag, pair)
            n_sym += 1
        elif back in first:
            assert np.array_equal(got[k], got[first[back]].T), (tag, pair)
            n_tr += 1
    return n_dup, n_tr, n_sym


@pytest.mark.parametrize("coords", [0, 1], ids=["parameter", "solver"])
@pytest.mark.parametrize("norm", ["NONE", "HUBER"])
@pytest.mark.parametrize("step", [1, 2])
def test_small_free_gauge_every_pair(step, norm, coords):
    """small: 6 cameras, 40 landmarks, n = 72 / 66, N = 128: camera 5 straddles the 64-edge in both steps.  All 36 camera
    pairs, all 240 camera-landmark pairs in both orders and all 1 600 landmark pairs in one request, shuffled, with duplicates."""
    ref = P.reference("small", step, norm, 0.0, True)
    s = ref.sys
    assert (s.n_cams, s.n_lms) == (6, 40)
    cc, cl, ll = P.all_pairs(s.n_cams, s.n_lms)
    pairs = cc + cl + [(kb, b, ka, a) for ka, a, kb, b in cl] + ll
    assert len(cc) == 36 and len(cl) == 240 and len(ll) == 1600
    rng = np.random.default_rng(100 * step + coords)
    pairs = pairs + [pairs[i] for i in rng.integers(0, len(pairs), size=40)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    ctx = _context("small", step, norm)
    tag = f"free gauge step {step} small {norm} coords {coords}"
    got, rc = ctx.covariance_blocks(pairs, step=step, lam=0.0, gauge=0, coords=coords)
    _check(tag, ref, pairs, got, rc, coords)
    n_dup, n_tr, n_sym = _check_bits(tag, pairs, got)
    assert n_dup == 40 and n_sym == 46 and n_tr == 30 + 480 + 1560
    at = {pair: k for k, pair in enumerate(pairs)}
    # the diagonal blocks against the calls that return them
    cam, rc_c = ctx.camera_covariance(step=step, lam=0.0, gauge=0, coords=coords)
    lms, rc_l = ctx.landmark_covariance(step=step, lam=0.0, gauge=0, coords=coords)
    assert rc_c == 0 and rc_l == 0
    cam_bound = ref.ref.cameras.bound * (float(s.sigma.max() ** 2) if coords == 0 else 1.0)
    lm_bound = ref.bound * ref.ref.scale(coords == 0)
    for c in range(s.n_cams):
        assert np.linalg.norm(got[at[(CAM, c, CAM, c)]] - cam[c]) <= cam_bound, (tag, c)
    for l in range(s.n_lms):
        assert np.linalg.norm(got[at[(LM, l, LM, l)]] - lms[l]) <= lm_bound, (tag, l)
    if coords == 1:  # the joint covariance of an observed (camera, landmark) pair is positive semi-definite
        p = L.problem("small")
        low = 0.0
        for l in range(s.n_lms):
            for c in np.unique(p.cam_idx[p.lm_off[l]:p.lm_off[l + 1]]):
                c = int(c)
                J = np.block([[got[at[(CAM, c, CAM, c)]], got[at[(CAM, c, LM, l)]]], [got[at[(LM, l, CAM, c)]], got[at[(LM, l, LM, l)]]]])
                assert np.array_equal(J, J.T)
                low = min(low, float(np.linalg.eigvalsh(J)[0]))
        print(f"{tag}: smallest eigenvalue of an observed pair's joint block {low:.3e} (bound {ref.bound:.3e})")
        assert low >= -ref.bound
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_p22_free_gauge(step):
    """p22: N = 320 / 256: the camera pairs reach into the off-diagonal tiles of C.  All 484 camera pairs, 300 seeded pairs of
    each of the other two kinds."""
    ref = P.reference("p22", step, "NONE", 0.0, True)
    s = ref.sys
    rng = np.random.default_rng(22 + step)
    cc = P.all_pairs(s.n_cams, 0)[0]
    _, cl, ll = P.sample_pairs(rng, s.n_cams, s.n_lms, 300)
    assert len(cc) == 484
    pairs = cc + cl + ll
    ctx = _context("p22", step)
    for coords in (1, 0):
        tag = f"free gauge step {step} p22 coords {coords}"
        got, rc = ctx.covariance_blocks(pairs, step=step, lam=0.0, gauge=0, coords=coords)
        _check(tag, ref, pairs, got, rc, coords)
        _check_bits(tag, pairs, got)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_tracks_free_gauge(step):
    """tracks: 66 cameras, track lengths 2, 15-17, 31-33, 63-65: the staging chunks of 64 (step 1) and 32 (step 2) repeat on
    either side of a landmark pair.  All 100 ordered pairs of the ten edge-length landmarks, and those ten with cameras 0, 5
    and 65 in both orders; solver coordinates."""
    ref = P.reference("tracks", step, "NONE", 0.0, True)
    s = ref.sys
    assert tuple(int(k) for k in s.track[:10]) == L.TRACK_EDGES
    ll = [(LM, l, LM, m) for l in range(10) for m in range(10)]
    cl = [(CAM, c, LM, l) for c in (0, 5, 65) for l in range(10)]
    pairs = ll + cl + [(kb, b, ka, a) for ka, a, kb, b in cl]
    ctx = _context("tracks", step)
    tag = f"free gauge step {step} tracks"
    got, rc = ctx.covariance_blocks(pairs, step=step, lam=0.0, gauge=0, coords=1)
    _check(tag, ref, pairs, got, rc, 1)
    n_dup, n_tr, n_sym = _check_bits(tag, pairs, got)
    assert (n_dup, n_tr, n_sym) == (0, 90 + 60, 10)
    ctx.close()


@pytest.mark.parametrize("lam", [1e-4, 1.0])
@pytest.mark.parametrize("name", ["small", "medium"])
@pytest.mark.parametrize("step", [1, 2])
def test_damped(step, name, lam):
    """The blocks of H(lambda)^-1: a seeded sample of 200 pairs of each kind; medium: n = 588 / 539, N = 640 / 576."""
    ref = P.reference(name, step, "NONE", lam, False)
    s = ref.sys
    cc, cl, ll = P.sample_pairs(np.random.default_rng(7 + step), s.n_cams, s.n_lms, 200)
    pairs = cc + cl + ll
    ctx = _context(name, step)
    for coords in (1, 0):
        tag = f"damped step {step} {name} lambda {lam:g} coords {coords}"
        got, rc = ctx.covariance_blocks(pairs, step=step, lam=lam, gauge=1, coords=coords)
        _check(tag, ref, pairs, got, rc, coords)
        _check_bits(tag, pairs, got)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_deterministic_context_returns_the_same_bits(step):
    """POVAR_FLAG_DETERMINISTIC: the ordered assembly makes C bit-reproducible, and the pair kernels add in a fixed order."""
    from povar_amd import capi
    ref = P.reference("small", step, "NONE", 0.0, True)
    s = ref.sys
    cc, cl, ll = P.sample_pairs(np.random.default_rng(3), s.n_cams, s.n_lms, 60)
    pairs = cc + cl + ll
    ctx = _context("small", step, flags=capi.FLAG_DETERMINISTIC)
    a, rc_a = ctx.covariance_blocks(pairs, step=step, lam=0.0, gauge=0, coords=0)
    assert ctx.sc_assembly() == 2
    b, rc_b = ctx.covariance_blocks(pairs, step=step, lam=0.0, gauge=0, coords=0)
    _check(f"deterministic step {step}", ref, pairs, a, rc_a, 0)
    assert rc_b == 0 and all(np.array_equal(x, y) for x, y in zip(a, b))
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_sharded_matches_single(step):
    """Two shard contexts on one device through the host all-reduce hook: every rank requests pairs of its own landmarks (ids
    of its shard) and any cameras."""
    from povar_amd import capi
    from test_gpu_sharded import HostAllReduce
    p = L.problem("p22")
    ref = P.reference("p22", step, "NONE", 0.0, True)
    cams, lms, obs = L.state(p, step)
    world = 2
    ar = HostAllReduce(world)
    out = [None] * world

    def worker(rank):
        try:
            lb, le = capi.shard_range(p.lm_off, world, rank)
            ob, oe = int(p.lm_off[lb]), int(p.lm_off[le])
            ctx = capi.Context(p.n_cams, p.lm_off[lb:le + 1] - p.lm_off[lb], p.cam_idx[ob:oe], obs[ob:oe])
            ctx.comm_init_host(world, rank, ar.fn(rank))
            _linearise(ctx, step, cams, lms[lb:le])
            cc, cl, ll = P.sample_pairs(np.random.default_rng(40 + rank), p.n_cams, le - lb, 60)
            pairs = cc + cl + ll
            got, rc = ctx.covariance_blocks(pairs, step=step, lam=0.0, gauge=0, coords=0)
            out[rank] = (lb, pairs, got, rc)
            ctx.close()
        except BaseException:
            ar.bar.abort()  # a failed rank must not leave the other one waiting
            raise

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert all(o is not None for o in out)
    for rank, (lb, pairs, got, rc) in enumerate(out):
        glob = [(ka, a + (lb if ka == LM else 0), kb, b + (lb if kb == LM else 0)) for ka, a, kb, b in pairs]
        _check(f"sharded step {step} rank {rank}", ref, pairs, got, rc, 0, want_pairs=glob)


def test_argument_errors():
    from povar_amd import capi
    p = L.problem("small")
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(L.ALPHA)
    n_lms = p.lm_off.shape[0] - 1
    out = np.zeros(4 * 144)
    good = [(CAM, 0, CAM, 1), (CAM, 2, LM, 3), (LM, 4, LM, 5)]
    size = {1: 144 + 36 + 9, 2: 144 + 48 + 16}

    def call(step, lam, gauge, coords, pairs=good, n_out=None, null_pairs=False, null_out=False):
        fn = ctx.L.povar_covariance_blocks_pose if step == 1 else ctx.L.povar_covariance_blocks_joint
        arr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 4)
        n_out = size[step] if n_out is None else n_out
        return fn(ctx.h, C.c_double(lam), C.c_int32(gauge), C.c_int32(coords), None if null_pairs else C.c_void_p(arr.ctypes.data),
                  C.c_int32(arr.shape[0]), None if null_out else C.c_void_p(out.ctypes.data), C.c_int64(n_out))

    # no linearisation in force
    assert call(1, 0.0, 0, 0) < 0 and call(2, 0.0, 0, 0) < 0
    assert ctx.linearize_pose(L.ALPHA)
    assert call(2, 0.0, 0, 0) < 0  # step 1's linearisation does not serve step 2
    assert call(1, 1e-4, capi.COV_FREE_GAUGE, 0) < 0   # free gauge with lambda != 0
    assert call(1, 0.0, capi.COV_DAMPED, 0) < 0 and call(1, -1.0, capi.COV_DAMPED, 0) < 0  # damped with lambda <= 0
    assert call(1, 0.0, 2, 0) < 0 and call(1, 0.0, 0, 2) < 0 and call(1, 0.0, -1, 0) < 0  # unknown gauge, coords
    assert call(1, 0.0, 0, 0, pairs=[(2, 0, CAM, 1)], n_out=144) < 0 and call(1, 0.0, 0, 0, pairs=[(CAM, 0, -1, 1)], n_out=144) < 0
    assert call(1, 0.0, 0, 0, pairs=[(CAM, p.n_cams, CAM, 0)], n_out=144) < 0 and call(1, 0.0, 0, 0, pairs=[(CAM, 0, CAM, -1)], n_out=144) < 0
    assert call(1, 0.0, 0, 0, pairs=[(LM, n_lms, LM, 0)], n_out=9) < 0 and call(1, 0.0, 0, 0, pairs=[(CAM, 0, LM, -1)], n_out=36) < 0
    assert call(1, 0.0, 0, 0, pairs=[(LM, p.n_cams, CAM, 0)], n_out=36) == 0  # (a landmark id may exceed n_cams)
    assert call(1, 0.0, 0, 0, n_out=size[1] - 1) < 0 and call(1, 0.0, 0, 0, n_out=size[1] + 1) < 0 and call(1, 0.0, 0, 0, n_out=0) < 0
    assert call(1, 0.0, 0, 1, n_out=size[1]) == 0 and call(1, 0.0, 0, 0, n_out=size[2]) < 0
    assert call(1, 0.0, 0, 0, null_pairs=True) < 0 and call(1, 0.0, 0, 0, null_out=True) < 0  # null pointers, n_pairs > 0
    with pytest.raises(capi.PovarError):
        ctx.covariance_blocks(good, step=1, lam=1.0, gauge=capi.COV_FREE_GAUGE)
    with pytest.raises(capi.PovarError):
        ctx.covariance_blocks([(3, 0, CAM, 0)], step=1)
    assert call(1, 0.0, 0, 0) == 0
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_empty_request_leaves_w_alone(step):
    """n_pairs = 0 returns 0 with the inspection state of a camera call (W, no panel); a non-empty request that of a landmark
    call (C off the diagonal, the panel, the gauge basis)."""
    from povar_amd import capi
    ctx = _context("small", step)
    joint = step == 2
    got, rc = ctx.covariance_blocks(np.zeros((0, 4), dtype=np.int32), step=step, lam=0.0, gauge=0, coords=0)
    assert rc == 0 and got == []
    fn = ctx.L.povar_covariance_blocks_pose if step == 1 else ctx.L.povar_covariance_blocks_joint
    assert fn(ctx.h, C.c_double(0.0), C.c_int32(0), C.c_int32(0), None, C.c_int32(0), None, C.c_int64(0)) == 0
    ctx.get_buffer(capi.BUF_COV_INVERSE, joint=joint)
    with pytest.raises(capi.PovarError):
        ctx.get_buffer(capi.BUF_COV_PANEL, joint=joint)
    got, rc = ctx.covariance_blocks([(CAM, 0, LM, 0)], step=step, lam=0.0, gauge=0, coords=0)
    assert rc == 0
    n = (11 if joint else 12) * 6
    assert ctx.get_buffer(capi.BUF_COV_PANEL, joint=joint).shape == (128, 64)
    assert ctx.get_buffer(capi.BUF_COV_GAUGE, joint=joint).shape == (n, 15 if joint else 12)
    ctx.get_buffer(capi.BUF_COV_INVERSE, joint=joint)
    ctx.close()


@pytest.mark.parametrize("step", [1, 2])
def test_free_gauge_reports_degeneracy_beyond_the_gauge(step):
    """medium_problem: null dimension 21 / 30 instead of 12 / 15: POVAR_NUMERIC_FAILURE and every output NaN."""
    from povar_amd import capi
    ctx = _context("medium", step)
    pairs = [(CAM, 0, CAM, 48), (CAM, 3, LM, 7), (LM, 7, CAM, 3), (LM, 1, LM, 299), (LM, 5, LM, 5)]
    for coords in (0, 1):
        got, rc = ctx.covariance_blocks(pairs, step=step, lam=0.0, gauge=0, coords=coords)
        assert rc == capi.NUMERIC_FAILURE and len(got) == len(pairs)
        assert all(b.size > 0 and np.all(np.isnan(b)) for b in got)
    ctx.close()


def test_solvers_unchanged_after_a_pair_covariance_call():
    """Nothing of the call leaks into the next assembly: CHOLESKY / RICHOLESKY increments after it match those before it (the
    assembly adds with atomics: 1e-8, the tolerance of the camera and landmark tests), and POVAR_BUF_SC_FACTOR is an argument
    error until the next direct solve."""
    from povar_amd import capi
    pairs = [(CAM, 0, CAM, 5), (CAM, 5, LM, 3), (LM, 3, LM, 39)]
    for step in (1, 2):
        ctx = _context("small", step)

        def solve():
            if step == 1:
                inc, it, status, rc = ctx.solve_pose_sc(LAM, capi.SC_CHOLESKY)
            else:
                inc, it, status, rc = ctx.solve_joint_sc(LAM, method=capi.SC_CHOLESKY)
            assert rc == 0 and it == 0
            return inc

        before = solve()
        ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
        for gauge, lam in ((capi.COV_FREE_GAUGE, 0.0), (capi.COV_DAMPED, 1.0)):
            _, rc = ctx.covariance_blocks(pairs, step=step, lam=lam, gauge=gauge)
            assert rc == 0
            with pytest.raises(capi.PovarError):
                ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
            after = solve()
            assert rel(after, before) < 1e-8, (step, gauge)
            ctx.get_buffer(capi.BUF_SC_FACTOR, joint=step == 2)
        ctx.close()


def test_bal_writes_the_covariance_blocks(tmp_path):
    """`bal --covariance-pairs-path IN --covariance-blocks-path OUT`: the number of pairs, then `rows cols` and the block per
    pair: free gauge, parameter coordinates, at the final state of the last step that ran.  With no LM iteration in either step
    that state is one a caller can set up too: there the file agrees with the ABI call.  --gpus 2 is refused."""
    from povar_amd import capi, synth
    p = synth.make_problem(10, 300, 1300, seed=21)
    f = str(tmp_path / "problem-10-300.txt")
    synth.write_data_custom(f, p)
    q = synth.read_data_custom(f)
    n_lms = q.lm_off.shape[0] - 1
    cc, cl, ll = P.sample_pairs(np.random.default_rng(5), q.n_cams, n_lms, 20)
    pairs = cc + cl + ll + [(CAM, 9, CAM, 9), (LM, n_lms - 1, LM, n_lms - 1)]
    pairs_file, out = str(tmp_path / "pairs.txt"), str(tmp_path / "blocks.txt")
    with open(pairs_file, "w") as fh:
        fh.write(f"{len(pairs)}\n" + "".join(f"{'cl'[ka]} {a} {'cl'[kb]} {b}\n" for ka, a, kb, b in pairs))
    base = [os.path.join(ROOT, "bin/bal"), "--input", f, "--quiet", "--power-sc-iterations", "20", "--log-disable-all",
            "--max-num-iterations-step-1", "0", "--max-num-iterations-step-2", "0",
            "--covariance-pairs-path", pairs_file, "--covariance-blocks-path", out]
    r = subprocess.run(base, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = open(out).read().split("\n")
    assert int(lines[0]) == len(pairs)
    ctx = capi.Context(q.n_cams, q.lm_off, q.cam_idx, q.obs)
    ctx.set_cameras(q.cams)
    ctx.init_landmarks_pose(L.ALPHA)
    assert ctx.linearize_pose(L.ALPHA)
    want, rc = ctx.covariance_blocks(pairs, step=1, lam=0.0, gauge=0, coords=0)
    ctx.close()
    assert rc == 0
    worst = 0.0
    for k, blk in enumerate(want):
        v = lines[1 + k].split()
        assert (int(v[0]), int(v[1])) == blk.shape and len(v) == 2 + blk.size
        worst = max(worst, rel(np.array([float(x) for x in v[2:]]).reshape(blk.shape), blk))
    print(f"bal against the ABI call: worst block {worst:.2e}")
    assert worst < 1e-9
    r = subprocess.run(base + ["--gpus", "2"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode != 0 and "--covariance-pairs-path" in r.stderr
