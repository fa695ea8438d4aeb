"""The context's state bookkeeping behind the LM loop (povar_lm.hip): compute_error_* of an unchanged state is answered
from the last evaluation (the reference's loop asks again at the top of every iteration,
bal_bundle_adjustment.cpp:302-310 / 600-605), the lane-per-landmark linearisation keeps the linearisation point in lane
order only and the landmark-order copy follows on demand, normalize_joint keeps the lane-ordered mirror current.
None of it may change a number: the sequences below run on two contexts, one of them with POVAR_NO_ERR_MEMO=1 (every call
evaluates), and must agree bit for bit; the exports are compared with the CPU oracle at the usual tolerances."""
import os

import numpy as np
import pytest

from conftest import rel

pytestmark = pytest.mark.gpu

ALPHA, LAM, M = 0.01, 1e-4, 6


def _ctx(p, memo, finalize=True, **kw):
    from povar_amd import capi
    old = os.environ.get("POVAR_NO_ERR_MEMO")
    os.environ["POVAR_NO_ERR_MEMO"] = "0" if memo else "1"
    try:
        ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, **kw)
        # Two contexts are compared number by number below: both run on the placed rows from the start.  (With the rows
        # placed on a host thread -- POVAR_LPL_PLACE=async -- each context would otherwise swap them in at whichever
        # linearisation finds them ready: a different summation order from a different iteration on, which is timing, not
        # the memo.  ADVICE r03.)
        if finalize:
            ctx.layout_finalize(True)
        return ctx
    finally:
        if old is None:
            del os.environ["POVAR_NO_ERR_MEMO"]
        else:
            os.environ["POVAR_NO_ERR_MEMO"] = old


def _ri(r):
    return (r.all_error, r.all_residual_sum, r.all_num_obs, r.valid_error, r.valid_residual_sum, r.valid_num_obs,
            r.is_numerically_valid)


def _same(a, b, exact, tol=1e-9):
    """two logs of tuples of numbers: identical, or equal to tol (costs of states that went through LM steps whose
    increments differ in the last bits; step 2 amplifies them: SURVEY 8(c) asks 1e-6 of an end-to-end cost)"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if exact:
            assert x == y
        else:
            assert len(x) == len(y) and all(abs(u - v) <= tol * max(abs(u), abs(v), 1e-300) for u, v in zip(x, y)), (x, y)


def _step1_sequence(ctx, p, log):
    from povar_amd import capi
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(ALPHA)
    log.append(_ri(ctx.error_pose(ALPHA)))
    log.append(_ri(ctx.error_pose(ALPHA)))            # unchanged state
    log.append(_ri(ctx.error_pose(0.1)))              # another alpha is another cost
    for it in range(3):
        log.append(_ri(ctx.error_pose(ALPHA)))
        assert ctx.linearize_pose(ALPHA)
        inc, _, _, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
        assert rc == 0
        ctx.backup_pose()
        ctx.apply_pose(capi.POWER_VARPROJ, ALPHA, inc)
        log.append(_ri(ctx.error_pose(ALPHA)))        # new state
        if it == 1:
            ctx.restore_pose()
            log.append(_ri(ctx.error_pose(ALPHA)))    # the backup again
    cams = ctx.get_cameras()
    cams[0, :] *= 1.0 + 1e-9
    ctx.set_cameras(cams)
    log.append(_ri(ctx.error_pose(ALPHA)))
    lms = ctx.get_landmarks()
    lms[0] += 1e-2                                    # (at the VarPro optimum the cost is flat to first order)
    ctx.set_landmarks(lms)
    log.append(_ri(ctx.error_pose(ALPHA)))
    log.append(_ri(ctx.error_pose(0.1)))              # (affine initial cameras make the cost independent of alpha)
    return ctx.get_cameras(), ctx.get_landmarks()


@pytest.mark.parametrize("e0_mode", [0, 2])
@pytest.mark.parametrize("which", ["small", "medium"])
def test_error_memo_changes_no_number_step1(which, e0_mode, small_problem, medium_problem):
    p = small_problem if which == "small" else medium_problem
    logs, states = [], []
    for memo in (True, False):
        ctx = _ctx(p, memo, e0_mode=e0_mode)
        log = []
        states.append(_step1_sequence(ctx, p, log))
        logs.append(log)
        ctx.close()
    # e0_mode 0 is bit-reproducible from context to context; the LDS-accumulating mode sums in the order its atomics
    # arrive (same numbers to rounding).  Inside ONE context an unchanged state must give the identical answer either way.
    _same(logs[0], logs[1], exact=e0_mode == 0)
    assert logs[0][0] == logs[0][1] and logs[0][-1] != logs[0][-2]
    if e0_mode == 0:
        assert np.array_equal(states[0][0], states[1][0]) and np.array_equal(states[0][1], states[1][1])
    else:
        assert rel(states[0][0], states[1][0]) < 1e-11 and rel(states[0][1], states[1][1]) < 1e-9
    # the values move when the state moves (a memo that never invalidates would pass the comparison above only if
    # the other context were broken the same way: check against the sequence itself)
    errs = [e[0] for e in logs[0]]
    assert errs[3] == errs[0] and errs[4] != errs[3] and errs[-2] != errs[-3]


@pytest.mark.parametrize("e0_mode", [0, 2])
def test_error_memo_changes_no_number_step2(e0_mode, small_problem):
    p = small_problem
    logs = []
    for memo in (True, False):
        ctx = _ctx(p, memo, e0_mode=e0_mode)
        ctx.set_cameras(p.cams)
        ctx.init_landmarks_pose(ALPHA)
        lms = ctx.get_landmarks()
        ctx.set_landmarks_homogeneous(np.concatenate([lms, np.ones((p.n_lms, 1))], axis=1))
        ctx.normalize_joint()
        log = [_ri(ctx.error_homogeneous()), _ri(ctx.error_homogeneous())]
        for it in range(3):
            assert ctx.linearize_homogeneous()
            inc, _, _, rc = ctx.solve_joint(LAM, M)
            assert rc == 0
            ctx.backup_joint()
            ctx.apply_joint(inc)
            log.append(_ri(ctx.error_homogeneous()))
            ctx.normalize_joint()                      # rescales cameras and landmarks: the cost is a new evaluation
            log.append(_ri(ctx.error_homogeneous()))
            if it == 1:
                ctx.restore_joint()
                log.append(_ri(ctx.error_homogeneous()))
        log.append(tuple(ctx.get_landmarks_homogeneous().ravel()[:64]))
        logs.append(log)
        ctx.close()
    _same(logs[0], logs[1], exact=e0_mode == 0, tol=1e-9 if e0_mode == 0 else 1e-6)


def test_normalize_joint_keeps_the_lane_mirror(medium_problem):
    """error_homogeneous reads the lane-ordered mirror; after normalize_joint it must see the normalised landmarks
    (checked against a context whose mirror is rebuilt from the landmark-order master by set_landmarks_homogeneous)."""
    p = medium_problem
    rng = np.random.default_rng(5)
    from povar_amd import capi
    a = _ctx(p, False, e0_mode=capi.E0_IMPLICIT_LDSACC)
    a.set_cameras(p.cams)
    a.init_landmarks_pose(ALPHA)
    lms = a.get_landmarks()
    X = np.concatenate([lms, np.ones((p.n_lms, 1))], axis=1) * rng.uniform(0.5, 2.0, (p.n_lms, 1))
    a.set_landmarks_homogeneous(X)
    a.error_homogeneous()                              # the mirror is current now
    a.normalize_joint()
    ra = _ri(a.error_homogeneous())
    Xn, Pn = a.get_landmarks_homogeneous(), a.get_cameras()
    assert np.array_equal(Xn, X / X[:, 3:4])
    b = _ctx(p, False, e0_mode=capi.E0_IMPLICIT_LDSACC)
    b.set_cameras(Pn)
    b.set_landmarks_homogeneous(Xn)
    _same([_ri(b.error_homogeneous())], [ra], exact=False)
    a.close()
    b.close()


@pytest.mark.parametrize("step", [1, 2])
def test_landmark_order_linearisation_point_follows_on_demand(step, small_problem):
    """Lane-per-landmark linearisation, then a move of the state, then a lane-per-observation consumer (the tile export,
    the legacy prepare): both must see the linearisation point, not the moved landmarks."""
    from povar_amd import capi
    from oracle import povar_oracle as O
    p = small_problem
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    ctx = _ctx(p, True, e0_mode=capi.E0_IMPLICIT_LDSACC)
    ctx.set_cameras(p.cams)
    lms = orc.init_landmarks_pose(ALPHA, p.cams)
    if step == 1:
        ctx.set_landmarks(lms)
        assert ctx.linearize_pose(ALPHA)
        inc, _, _, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
        assert rc == 0
        ctx.apply_pose(capi.POWER_VARPROJ, ALPHA, inc)     # lms4 moves; lms_lin4 has not been materialised yet
        assert rel(ctx.get_landmarks(), lms) > 1e-9
        st, diag2, jls, sigma, ok = orc.stage1_pose(ALPHA, p.cams, lms)
        orc.scale_jp_cols_pose(st, sigma)
        assert rel(ctx.get_buffer(capi.BUF_JL_COL_SCALE), jls.ravel()) < 1e-13
        assert rel(ctx.get_buffer(capi.BUF_STORAGE), st.ravel()) < 1e-13   # rebuilt from (cams_lin4, lms_lin4)
    else:
        X = np.concatenate([lms, np.ones((p.n_lms, 1))], axis=1)
        ctx.set_landmarks_homogeneous(X)
        ctx.normalize_joint()
        Xn, Pn = ctx.get_landmarks_homogeneous(), ctx.get_cameras()
        assert ctx.linearize_homogeneous()
        inc, _, _, rc = ctx.solve_joint(LAM, M)
        assert rc == 0
        ctx.apply_joint(inc)
        assert rel(ctx.get_landmarks_homogeneous(), Xn) > 1e-9
        ctx.set_e0_mode(capi.E0_IMPLICIT)                  # lane-per-observation kernels from here on
        ctx.prepare_joint(LAM)
        # second context: the same linearisation point, lane-per-observation kernels from the start
        ref = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, e0_mode=capi.E0_IMPLICIT)
        ref.set_cameras(Pn)
        ref.set_landmarks_homogeneous(Xn)
        assert ref.linearize_homogeneous()
        ref.prepare_joint(LAM)
        for which in (capi.BUF_B_JOINT, capi.BUF_JL_COL_SCALE_H, capi.BUF_B_INV_JOINT):
            assert rel(ctx.get_buffer(which), ref.get_buffer(which)) < 1e-11, which
        ref.close()
    ctx.close()


def _solve_once(ctx, p, step):
    from povar_amd import capi
    if step == 1:
        assert ctx.linearize_pose(ALPHA)
        inc, _, _, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
    else:
        assert ctx.linearize_homogeneous()
        inc, _, _, rc = ctx.solve_joint(LAM, M)
    assert rc == 0
    return inc


def _start(ctx, p, step):
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(ALPHA)
    if step == 2:
        lms = ctx.get_landmarks()
        ctx.set_landmarks_homogeneous(np.concatenate([lms, np.ones((p.n_lms, 1))], axis=1))
        ctx.normalize_joint()


@pytest.mark.parametrize("step", [1, 2])
def test_rows_placed_on_a_host_thread_are_swapped_in(step, medium_problem, monkeypatch):
    """POVAR_LPL_PLACE=async (the default from 2^20 observations on): povar_create returns on the natural row order, the
    placed rows arrive later.  On either order the results agree with POVAR_LPL_PLACE=sync to rounding (another summation
    order of the same numbers); the placement state goes 2 -> 3; a linearisation taken before povar_layout_finalize
    swapped the rows is dropped; povar_linearize_* swaps by itself once the thread has delivered."""
    import time
    from povar_amd import capi
    p = medium_problem
    kw = dict(e0_mode=capi.E0_IMPLICIT_LDSACC)
    monkeypatch.setenv("POVAR_E0_V1", "0")             # the lane-per-landmark kernels also under 65 536 observations
    monkeypatch.setenv("POVAR_LPL_PLACE", "sync")
    ref = _ctx(p, True, **kw)
    assert ref.layout_info().placement == 1 and ref.layout_finalize(wait=False)
    _start(ref, p, step)
    want = _solve_once(ref, p, step)
    monkeypatch.setenv("POVAR_LPL_PLACE", "none")
    nat = _ctx(p, True, **kw)
    assert nat.layout_info().placement == 0 and not nat.layout_finalize(wait=True)
    _start(nat, p, step)
    assert rel(_solve_once(nat, p, step), want) < 1e-10
    monkeypatch.setenv("POVAR_LPL_PLACE", "async")
    ctx = _ctx(p, True, finalize=False, **kw)
    assert ctx.layout_info().placement == 2
    _start(ctx, p, step)
    assert rel(_solve_once(ctx, p, step), want) < 1e-10      # on either row order, whichever the thread's progress allowed
    swapped_by_linearize = ctx.layout_info().placement == 3
    assert ctx.layout_finalize(wait=True)
    li = ctx.layout_info()
    assert li.placement == 3 and li.placement_ms > 0
    if not swapped_by_linearize:                       # the swap happened in povar_layout_finalize: linearise again
        with pytest.raises(capi.PovarError):
            ctx.prepare_pose(LAM) if step == 1 else ctx.prepare_joint(LAM)
    assert rel(_solve_once(ctx, p, step), want) < 1e-10
    # the swap inside povar_linearize_*: keep linearising until the thread has delivered
    auto = _ctx(p, True, **kw)
    _start(auto, p, step)
    for _ in range(400):
        got = _solve_once(auto, p, step)
        assert rel(got, want) < 1e-10
        if auto.layout_info().placement == 3:
            break
        time.sleep(0.01)
    assert auto.layout_info().placement == 3
    for c in (ref, nat, ctx, auto):
        c.close()


def _free_device_bytes():
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_destroy_does_not_wait_for_a_row_placement_nobody_will_use(monkeypatch):
    """povar_destroy cancels the host thread (checked between its work items) and joins it: a context dropped right
    after povar_create, at any point of the placement, neither hangs nor leaks the thread's device buffers."""
    import time
    from povar_amd import capi, synth
    monkeypatch.setenv("POVAR_LPL_PLACE", "async")
    p = synth.make_problem(300, 60000, 300000, seed=4)
    t_create = t_close = 0.0
    free0 = None
    for k in range(12):
        t0 = time.perf_counter()
        ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, e0_mode=capi.E0_IMPLICIT_LDSACC)
        t1 = time.perf_counter()
        assert ctx.layout_info().placement == 2
        time.sleep(0.004 * (k % 4))                     # drop it at different stages of the background build
        if k % 3 == 2:
            ctx.set_cameras(p.cams)
            ctx.init_landmarks_pose(ALPHA)
            assert ctx.linearize_pose(ALPHA)            # may or may not swap
        t2 = time.perf_counter()
        ctx.close()
        t_create += t1 - t0
        t_close += time.perf_counter() - t2
        free = _free_device_bytes()
        free0 = free if free0 is None else free0
        assert free >= free0 - (64 << 20), (k, free0, free)   # nothing accumulates from context to context
    assert t_close < t_create + 1.0


def test_graph_capture_while_the_placement_thread_uploads(monkeypatch):
    """A hipMalloc / hipMemcpy of the row-placement thread inside the caller's capture of the term loop invalidated the
    capture (error -1901 "operation failed due to a previous error during capture"): the two are serialised now.  First
    solves (= captures) at a range of delays after povar_create, so that some of them meet the thread's upload phase."""
    import time
    from povar_amd import capi, synth
    monkeypatch.setenv("POVAR_LPL_PLACE", "async")
    p = synth.make_problem(300, 60000, 300000, seed=4)
    ref = None
    for k in range(14):
        ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, e0_mode=capi.E0_IMPLICIT_LDSACC)
        ctx.set_cameras(p.cams)
        ctx.init_landmarks_pose(ALPHA)
        time.sleep(0.003 * k)
        for _ in range(3):                              # three captures in a row (another m: another graph)
            assert ctx.linearize_pose(ALPHA)
            inc, _, _, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M + _)
            assert rc == 0
        ref = inc if ref is None else ref
        assert rel(inc, ref) < 1e-10
        ctx.close()


@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
@pytest.mark.parametrize("form", ["fixed-point", "gather"])
@pytest.mark.parametrize("name", ["trafalgar-257", "venice-1778"])
def test_povar_deterministic_is_bit_reproducible(monkeypatch, name, form, robust):
    """POVAR_DETERMINISTIC=1 (fixed reduction order inside a GPU): whatever E0 mode the caller asks for, the
    context linearises and prepares in the gather mode (no atomics), the terms of step 1's series run the fixed-point form
    of e0_ck (integer LDS adds: associative) -- or, POVAR_DET_CK=0, the gather form of the operator --, and no run-time
    timing picks a kernel: two contexts on the same problem and repeated solves give BIT-identical increments, terms, model
    decreases and costs; the default mode agrees with them to rounding (1e-10 on the 20-term increment, as the parity tests
    against the oracle ask of every mode)."""
    from povar_amd import capi, synth
    if robust != "NONE" and form == "gather":
        pytest.skip("one robust case per size is enough for the gather form")
    p = synth.make_bal_problem(name)
    monkeypatch.setenv("POVAR_DET_CK", "1" if form == "fixed-point" else "0")

    def run(det):
        if det:
            monkeypatch.setenv("POVAR_DETERMINISTIC", "1")
        else:
            monkeypatch.delenv("POVAR_DETERMINISTIC", raising=False)
        ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=robust, e0_mode=capi.E0_IMPLICIT_LDSACC)
        ctx.layout_finalize(True)
        ctx.set_cameras(p.cams)
        ctx.init_landmarks_pose(0.01)
        assert ctx.linearize_pose(0.01)
        ctx.set_e0_kernel(0)          # (pinned in the deterministic mode: these calls change nothing there)
        ctx.set_series_kernel(0)
        incs = [ctx.solve_pose(1e-4, capi.POWER_VARPROJ, 20)[0] for _ in range(2)]
        term = ctx.get_term()
        ld = ctx.apply_pose(capi.POWER_VARPROJ, 0.01, incs[0])
        cost = ctx.error_pose(0.01).all_error
        li = ctx.layout_info()
        ctx.close()
        return incs, term, ld, cost, li

    (a0, a1), ta, lda, ca, lia = run(True)
    (b0, b1), tb, ldb, cb, lib = run(True)
    assert lia.e0_auto == 0 and lia.res_active == 0 and lia.res_auto == 0
    assert lia.e0_kernel == (7 if form == "fixed-point" else 0), "7: the fixed-point form of e0_ck"
    assert np.array_equal(a0, a1) and np.array_equal(a0, b0) and np.array_equal(b0, b1) and np.array_equal(ta, tb)
    assert lda == ldb and ca == cb
    (c0, _), tc, ldc, cc, _ = run(False)
    assert np.linalg.norm(c0 - a0) <= 1e-10 * np.linalg.norm(a0) and abs(cc / ca - 1) < 1e-9
    assert np.linalg.norm(tc - ta) <= 1e-9 * np.linalg.norm(ta)


def test_behaviour_switches_through_the_abi_flags_word(monkeypatch):
    """the behaviour switches of a context are fields of povar_options.flags (include/povar_hip.h:
    POVAR_FLAG_*, the reference's counterpart is SolverOptions, bal/solver_options.hpp:95-305) -- no environment variable
    involved.  POVAR_FLAG_DETERMINISTIC through the C ABI: the fixed-point camera-chunk kernel (7) runs the terms, two contexts
    give bit-identical increments; with POVAR_FLAG_DET_GATHER_TERMS the gather form (0) does; the kernel-choice fields pin the
    E0 kernel and the series form; POVAR_FLAG_NO_PACKED_ROWS keeps the 16-byte image points; an environment variable that is
    set still overrides its flag."""
    from povar_amd import capi, synth
    for k in ("POVAR_DETERMINISTIC", "POVAR_DET_CK", "POVAR_E0_CK", "POVAR_RES", "POVAR_LPL_PLACE", "POVAR_CK_PACK", "POVAR_E0_V1", "POVAR_NO_GRAPH",
              "POVAR_RES_WGS", "POVAR_E0_WGS"):  # (tools/forced_mode_suite.sh: the resident series over seven workgroups is not what the library would time)
        monkeypatch.delenv(k, raising=False)
    p = synth.make_bal_problem("trafalgar-257")

    def run(flags):
        ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, e0_mode=capi.E0_IMPLICIT_LDSACC, flags=flags)
        ctx.layout_finalize(True)
        ctx.set_cameras(p.cams)
        ctx.init_landmarks_pose(0.01)
        assert ctx.linearize_pose(0.01)
        inc = ctx.solve_pose(1e-4, capi.POWER_VARPROJ, 20)[0]
        li = ctx.layout_info()
        ctx.close()
        return inc, li

    a, lia = run(capi.FLAG_DETERMINISTIC)
    b, lib = run(capi.FLAG_DETERMINISTIC)
    assert lia.e0_kernel == 7 and lia.e0_auto == 0 and lia.res_active == 0 and lia.ck_packed == 0
    assert np.array_equal(a, b), "POVAR_FLAG_DETERMINISTIC: two contexts, two different increments"
    g, lig = run(capi.FLAG_DETERMINISTIC | capi.FLAG_DET_GATHER_TERMS)
    assert lig.e0_kernel == 0 and np.linalg.norm(g - a) <= 1e-12 * np.linalg.norm(a)
    d, lid = run(0)
    assert lid.e0_auto == 2 and lid.res_auto == 2 and np.linalg.norm(d - a) <= 1e-10 * np.linalg.norm(a)
    for k in (0, 1, 3):
        f, lif = run(capi.flag_e0_kernel(k) | capi.flag_series_kernel(0))
        assert lif.e0_kernel == k and lif.e0_auto == 0 and lif.res_auto == 0 and lif.res_active == 0
        assert np.linalg.norm(f - a) <= 1e-10 * np.linalg.norm(a)
    r, lir = run(capi.flag_series_kernel(1))
    assert lir.res_auto == 0 and lir.res_active == 1 and lir.res_failed == 0 and np.linalg.norm(r - a) <= 1e-10 * np.linalg.norm(a)
    assert run(capi.flag_e0_kernel(1))[1].ck_packed == 1 and run(capi.flag_e0_kernel(1) | capi.FLAG_NO_PACKED_ROWS)[1].ck_packed == 0
    assert run(capi.flag_placement(3))[1].placement == 0 and run(capi.flag_placement(1))[1].placement == 1
    monkeypatch.setenv("POVAR_DETERMINISTIC", "0")  # the variable wins over the flag
    assert run(capi.FLAG_DETERMINISTIC)[1].e0_kernel != 7


@pytest.mark.parametrize("e0_mode", [0, 2])
@pytest.mark.parametrize("v1", ["1", "0"])
def test_a_stage_before_its_linearisation_is_refused_and_changes_nothing(v1, e0_mode, small_problem, monkeypatch):
    """prepare_* / apply_* need the linearisation of their own step: before any, and after the other step's, they raise and
    name the missing call.  A refused call leaves no trace: from the same state, one LM step of the context that saw the
    refusals equals that of a context that never did -- bit for bit in e0_mode 0 (bit-reproducible from context to
    context), to 1e-11 where atomics order the sums (the LDS-accumulating mode, lane per landmark or per observation)."""
    from povar_amd import capi
    monkeypatch.setenv("POVAR_E0_V1", v1)
    p = small_problem
    ctx, ref = _ctx(p, True, e0_mode=e0_mode), _ctx(p, True, e0_mode=e0_mode)
    assert ctx.layout_info().lane_per_landmark == (1 if v1 == "0" else 0)
    zero12, zero11 = np.zeros(12 * p.n_cams), np.zeros(11 * p.n_cams)

    def refused(missing, *calls):
        for call in calls:
            with pytest.raises(capi.PovarError, match=f"before {missing}$"):
                call()

    step1_calls = (lambda: ctx.prepare_pose(LAM), lambda: ctx.apply_pose(capi.POWER_VARPROJ, ALPHA, zero12))
    step2_calls = (lambda: ctx.prepare_joint(LAM), lambda: ctx.apply_joint(zero11))
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(ALPHA)
    lms = ctx.get_landmarks()
    X = np.concatenate([lms, np.ones((p.n_lms, 1))], axis=1)
    refused("povar_linearize_pose", *step1_calls)
    refused("povar_linearize_homogeneous", *step2_calls)

    def lm_step(c, step, refuse):
        """one LM step from the same state in either context; refuse: the other step's calls, right after the linearisation"""
        c.set_cameras(p.cams)
        if step == 1:
            c.set_landmarks(lms)
            assert c.linearize_pose(ALPHA)
        else:
            c.set_landmarks_homogeneous(X)
            c.normalize_joint()
            assert c.linearize_homogeneous()
        refuse()
        inc, _, _, rc = c.solve_pose(LAM, capi.POWER_VARPROJ, M) if step == 1 else c.solve_joint(LAM, M)
        assert rc == 0
        ld = c.apply_pose(capi.POWER_VARPROJ, ALPHA, inc) if step == 1 else c.apply_joint(inc)
        return inc, np.array([ld]), c.get_cameras(), c.get_landmarks() if step == 1 else c.get_landmarks_homogeneous()

    # step 1 (step 2 was never linearised), step 2 (drops step 1's linearisation), step 1 again (drops step 2's)
    for step in (1, 2, 1):
        got = lm_step(ctx, step, lambda: refused("povar_linearize_homogeneous", *step2_calls) if step == 1
                      else refused("povar_linearize_pose", *step1_calls))
        want = lm_step(ref, step, lambda: None)
        for name, g, w in zip(("increment", "l_diff", "cameras", "landmarks"), got, want):
            print(f"step {step} {name}: rel {rel(g, w):.3e}")
            assert np.array_equal(g, w) if e0_mode == 0 else rel(g, w) <= 1e-11, (step, name)
    ctx.close()
    ref.close()
