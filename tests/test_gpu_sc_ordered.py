"""The ordered assembly of the dense reduced camera matrix (sc_dense_ordered, povar_set_sc_assembly; what a context created with
POVAR_FLAG_DETERMINISTIC runs): CHOLESKY, RICHOLESKY and the three covariance families behind it.

  bounds    the ordered kernel adds the terms of sc_dense_offdiag[_h] (one expression: Step::term) in another order, and the
            componentwise bounds of tests/sc_bounds.py do not depend on the order: check_case of tests/test_gpu_sc_bounds.py runs
            unchanged, with its references, on cases of that module's CASES -- after set_sc_assembly(2) on a default context and
            on a context created with the flag alone.  The column tile is 32 cameras: 5 cameras (one partial tile, padding 4),
            26 and 29 (under one tile), 64 (two full tiles), 49, and the edge graphs' 150 (four full tiles and a partial one;
            tracks of 140 / 97 / 65 / 64 / 33 observations, three cameras nobody observes: block rows with no walk).
  bits      with the flag, two fresh contexts and two solves of one context leave the same increment and the same R (columns
            j >= i), y and x bit for bit; two contexts return the same camera, landmark and observation covariances.
  shards    two landmark shards over the host all-reduce hook (which sums in rank order): the bounds on both ranks, and two
            runs agree bit for bit.
  default   a default context still runs the atomics; the value povar_sc_assembly reports; the setter's argument check; the
            pinned setter of a deterministic context.
  bal       `bal --deterministic` with CHOLESKY, RICHOLESKY and the three covariance files, twice: the same costs digit for
            digit and byte-identical files.
"""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import sc_bounds as SB
import test_gpu_operand_bounds as G
import test_gpu_sc_bounds as S
import test_sc_bounds as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ORDERED = [("pose-5", "NONE", SB.LAM, "auto"), ("pose-5", "HUBER", SB.LAM, "auto"), ("pose-26", "NONE", 1.0, "lpl"),
           ("joint-29", "NONE", SB.LAM, "auto"), ("joint-64", "NONE", SB.LAM, "auto"), ("pose-medium", "NONE", SB.LAM, "auto"),
           ("pose-edge", "NONE", SB.LAM, "auto"), ("joint-edge", "HUBER", SB.LAM, "lpl")]
assert all(c in S.CASES for c in ORDERED)


def _system(name, robust, lam):
    """The reference the bounds module keeps for the case (computed once, shared with it, left unchanged)."""
    if name.endswith("edge") and robust == "HUBER":
        key = (name, robust, lam, 1)
        if key not in S._REF:
            step, make = T.SHAPES[name]
            S._REF[key] = SB.dense_system(make(robust, lam), step == 2)
        return S._REF[key]
    return S._reference(name, robust, lam)


def _det_context(monkeypatch, p):
    """A context created with POVAR_FLAG_DETERMINISTIC and nothing else set."""
    from povar_amd import capi
    for k in G._OVERRIDES + ("POVAR_E0_V1", "POVAR_DETERMINISTIC", "POVAR_LPL_PLACE"):
        monkeypatch.delenv(k, raising=False)
    return capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=p.robust, huber=p.huber, eps=p.eps,
                        flags=capi.FLAG_DETERMINISTIC)


@pytest.mark.parametrize("how", ["set", "flag"])
@pytest.mark.parametrize("name,robust,lam,fam", ORDERED, ids=["-".join([s, r, f"{lam:g}", f]) for s, r, lam, f in ORDERED])
def test_ordered_assembly_within_componentwise_bounds(monkeypatch, name, robust, lam, fam, how):
    sy = _system(name, robust, lam)
    if how == "set":
        ctx = S._context(monkeypatch, fam, sy.p)
        assert ctx.sc_assembly() == 0
        ctx.set_sc_assembly(2)
    else:
        ctx = _det_context(monkeypatch, sy.p)
    inc = S._solve(ctx, sy)
    assert ctx.sc_assembly() == 2
    if robust == "HUBER":
        assert (sy.R.aux["w"] < 1).any(), "the robust norm down-weights nothing on this case"
    S.check_case(ctx, sy, inc, f"ordered/{how}/{name}/{robust}/lam={lam:g}/{fam}")
    ctx.close()


def _factor(ctx, sy):
    """What the header specifies of POVAR_BUF_SC_FACTOR: the columns j >= i of R, then y and x."""
    from povar_amd import capi
    buf = ctx.get_buffer(capi.BUF_SC_FACTOR, joint=sy.joint)
    return np.triu(buf[:, :sy.N]), buf[:, sy.N].copy(), buf[:, sy.N + 1].copy()


def _same(a, b, what):
    for x, y, part in zip(a, b, ("inc", "R", "y", "x")):
        assert np.array_equal(x, y), f"{what}: {part} differs in {np.count_nonzero(x != y)} entries, max {np.abs(x - y).max():.3g}"


@pytest.mark.parametrize("name", ["pose-edge", "joint-edge"])
def test_direct_solves_are_bit_reproducible_with_the_flag(monkeypatch, name):
    from povar_amd import capi
    sy = _system(name, "NONE", SB.LAM)
    runs = []
    for k in range(2):
        ctx = _det_context(monkeypatch, sy.p)
        inc = S._solve(ctx, sy)
        assert ctx.sc_assembly() == 2
        runs.append((inc,) + _factor(ctx, sy))
        if k == 1:  # the same context once more
            inc2 = S._solve(ctx, sy)
            _same(runs[1], (inc2,) + _factor(ctx, sy), f"{name}: two solves of one context")
        ctx.close()
    _same(runs[0], runs[1], f"{name}: two contexts")


@pytest.mark.parametrize("name", ["pose-edge", "joint-edge"])
def test_pcg_is_bit_reproducible_with_the_flag(monkeypatch, name):
    """PCG / RIPCG assemble nothing: expected to hold before the ordered assembly as well."""
    from povar_amd import capi
    sy = _system(name, "NONE", SB.LAM)
    p = sy.p

    def pcg(ctx):
        inc, it, st, rc = ctx.solve_joint_sc(p.lam, 0, 500, 1e-2) if sy.joint else ctx.solve_pose_sc(p.lam, capi.SC_PCG, 0, 500, 1e-2)
        assert rc == 0 and it > 0
        return inc, it

    out = []
    for k in range(2):
        ctx = _det_context(monkeypatch, p)
        S._solve(ctx, sy)
        out.append(pcg(ctx))
        assert ctx.sc_assembly() == 2  # (left alone by PCG)
        if k == 1:
            again = pcg(ctx)
            assert again[1] == out[1][1] and np.array_equal(again[0], out[1][0]), f"{name}: two PCG solves of one context"
        ctx.close()
    assert out[0][1] == out[1][1] and np.array_equal(out[0][0], out[1][0]), f"{name}: PCG on two contexts"


def _cov_system(name):
    if name == "cov-small-2":  # a step-2 state whose free-gauge covariance exists (tests/cov_bounds.py: CASES)
        import cov_bounds as CB
        return CB.system("small", 2, "NONE", 0.0)
    return _system(name, "NONE", SB.LAM)


# joint-29 in the free gauge is singular beyond its gauge: the undamped reference S of that random step-2 state has more than 20
# eigenvalues under 3e-16 against a largest of 3.98 (15 belong to the gauge), so both contexts return POVAR_NUMERIC_FAILURE and
# all-NaN outputs -- the same ones.  Step 2's covariances themselves are compared on joint-29 damped and on cov-small-2.
@pytest.mark.parametrize("name,damped,exists", [("pose-26", False, True), ("joint-29", False, False), ("pose-26", True, True),
                                                ("joint-29", True, True), ("cov-small-2", False, True)])
def test_covariances_are_bit_reproducible_with_the_flag(monkeypatch, name, damped, exists):
    from povar_amd import capi
    import test_gpu_cov_bounds as CV
    sy = _cov_system(name)
    step = 2 if sy.joint else 1
    lam, gauge = (SB.LAM, capi.COV_DAMPED) if damped else (0.0, capi.COV_FREE_GAUGE)
    out = []
    for _ in range(2):
        ctx = _det_context(monkeypatch, sy.p)
        CV._linearise(ctx, sy)
        cam, rc0 = ctx.camera_covariance(step, lam, gauge)
        assert ctx.sc_assembly() == 2
        lm, cam2, rc1 = ctx.landmark_covariance(step, lam, gauge, with_cameras=True)
        rows, rc2 = ctx.observation_covariance(step, lam, gauge)
        assert (rc0, rc1, rc2) == ((0, 0, 0) if exists else (capi.NUMERIC_FAILURE,) * 3), (name, rc0, rc1, rc2)
        if exists:
            assert np.all(np.isfinite(cam)) and np.all(np.isfinite(lm)) and np.all(np.isfinite(rows[:, 0]))
        else:
            assert np.all(np.isnan(cam)) and np.all(np.isnan(lm)) and np.all(np.isnan(rows))
        out.append((cam, lm, cam2, rows))
        ctx.close()
    for a, b, what in zip(out[0], out[1], ("camera", "landmark", "camera blocks of the landmark call", "observation")):
        assert np.array_equal(a, b, equal_nan=True), f"{name}: {what} covariance differs in {np.count_nonzero(a != b)} entries"
    assert np.array_equal(out[0][0], out[0][2], equal_nan=True)  # (one C: the camera call's blocks and the landmark call's)


def _two_shards(sy):
    """test_two_shards_over_the_host_all_reduce with the deterministic flag: per rank (inc, [BLOCKDIAG, PRECOND, FACTOR], assembly)."""
    from povar_amd import capi
    import test_gpu_joint_cholesky as J
    p, world = sy.p, 2
    ar = J.HostAllReduce(world)
    out, err = [None] * world, [None] * world

    def worker(rank):
        try:
            lb, le = capi.shard_range(p.lm_off, world, rank)
            ob, oe = int(p.lm_off[lb]), int(p.lm_off[le])
            ctx = capi.Context(p.n_cams, p.lm_off[lb:le + 1] - p.lm_off[lb], p.cam_idx[ob:oe], p.obs[ob:oe], e0_mode=0,
                               flags=capi.FLAG_DETERMINISTIC)
            ctx.comm_init_host(world, rank, ar.fn(rank))
            inc = S._solve(ctx, sy, p.lms[lb:le])
            bufs = [ctx.get_buffer(b, joint=True) for b in (capi.BUF_SC_BLOCKDIAG, capi.BUF_SC_PRECOND, capi.BUF_SC_FACTOR)]
            out[rank] = (inc, bufs, ctx.sc_assembly())
            ctx.close()
        except BaseException as e:  # noqa: BLE001 (reported by the main thread)
            err[rank] = e
            ar.bar.abort()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert err == [None] * world, err
    return out


def test_two_shards_ordered_over_the_host_all_reduce(monkeypatch):
    from povar_amd import capi
    for k in G._OVERRIDES + ("POVAR_E0_V1", "POVAR_DETERMINISTIC", "POVAR_LPL_PLACE"):
        monkeypatch.delenv(k, raising=False)
    sy = S._reference("joint-29", "NONE", SB.LAM, shards=2)
    ids = (capi.BUF_SC_BLOCKDIAG, capi.BUF_SC_PRECOND, capi.BUF_SC_FACTOR)

    class Held:  # (check_case reads a context: hand it the buffers a rank exported)
        def __init__(self, bufs):
            self.bufs = dict(zip(ids, bufs))

        def get_buffer(self, which, joint=False):
            return self.bufs[which]

    runs = [_two_shards(sy), _two_shards(sy)]
    for rank in range(2):
        inc, bufs, asm = runs[0][rank]
        assert asm == 2
        S.check_case(Held(bufs), sy, inc, f"ordered/joint-29/NONE/two-shards/rank{rank}")
        inc_b, bufs_b, _ = runs[1][rank]
        tri = lambda f: (np.triu(f[:, :sy.N]), f[:, sy.N], f[:, sy.N + 1])  # noqa: E731
        _same((inc,) + tri(bufs[2]), (inc_b,) + tri(bufs_b[2]), f"two runs, rank {rank}")


def test_the_default_assembly_is_untouched(monkeypatch):
    from povar_amd import capi
    sy = _system("pose-5", "NONE", SB.LAM)
    p = sy.p
    ctx = S._context(monkeypatch, "auto", p)
    det_env = os.environ.get("POVAR_DETERMINISTIC") == "1"  # (the forced-mode suite: every context is deterministic)
    want = 2 if det_env else 1
    assert ctx.sc_assembly() == 0
    S._solve(ctx, sy)
    assert ctx.sc_assembly() == want
    assert ctx.solve_pose_sc(p.lam, capi.SC_PCG, 0, 500, 1e-2)[3] == 0
    assert ctx.sc_assembly() == want
    with pytest.raises(capi.PovarError, match="assembly"):
        ctx.set_sc_assembly(7)
    ctx.set_sc_assembly(2)
    ctx.set_sc_assembly(-1)  # back to the library's choice
    S._solve(ctx, sy)
    assert ctx.sc_assembly() == want
    ctx.close()
    det = _det_context(monkeypatch, p)
    det.set_sc_assembly(1)  # pinned: returns 0, changes nothing
    inc = S._solve(det, sy)
    assert det.sc_assembly() == 2
    S.check_case(det, sy, inc, "ordered/pinned/pose-5")
    det.close()


def test_bal_direct_solves_and_covariances_are_bit_reproducible(tmp_path):
    """`bal --deterministic --solver-type-step-1 CHOLESKY --solver-type-step-2 RICHOLESKY` with the three covariance files, twice
    on a small data_custom problem: the same per-iteration costs digit for digit (the log prints 17 significant digits), the
    same accept / reject sequence, byte-identical covariance files."""
    from povar_amd import synth
    p = synth.make_problem(10, 300, 1300, seed=21)
    f = str(tmp_path / "problem-10-300.txt")
    synth.write_data_custom(f, p)
    files = ("camera", "landmark", "observation")

    def run(tag):
        env = dict(os.environ)
        env.pop("POVAR_DETERMINISTIC", None)
        log = str(tmp_path / f"{tag}.json")
        cmd = [os.path.join(ROOT, "bin/bal"), "--input", f, "--log-log-path", log, "--quiet", "--deterministic",
               "--solver-type-step-1", "CHOLESKY", "--solver-type-step-2", "RICHOLESKY",
               "--max-num-iterations-step-1", "8", "--max-num-iterations-step-2", "4"]
        for k in files:
            cmd += [f"--{k}-covariance-path", str(tmp_path / f"{tag}_{k}.txt")]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return json.load(open(log)), [open(str(tmp_path / f"{tag}_{k}.txt"), "rb").read() for k in files]

    (a, fa), (b, fb) = run("det1"), run("det2")
    assert len(a["cost"]) > 4
    assert a["cost"] == b["cost"] and a["step_is_successful"] == b["step_is_successful"] and a["iteration"] == b["iteration"]
    for k, x, y in zip(files, fa, fb):
        assert len(x) > 100 and x == y, f"the {k} covariance files of two runs differ"
