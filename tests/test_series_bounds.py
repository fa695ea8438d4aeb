"""The launch identity of tests/series_bounds.py checked on the CPU: fp64 emulations of whole k-term series (sums in seeded
random orders) stay inside the componentwise bound on |R|, R = (S_k - x_0) - T_ref(S_k) + T_ref(x_k), and every defect that
is specific to a resident launch -- a stale z block, a dropped or stale partial record, a dropped observation, landmark sums
that were not re-zeroed -- injected at term j of k puts at least one entry over its bound, at every j.  Edge graphs of both
steps (rounding_bounds.edge_problem / edge_problem_joint), NONE and HUBER, k in KS.

Measured when these tests were written (every figure is one a test prints: SERIESBOUND / SERIESMUT lines under -s).

Clean emulations, three seeds, k = 1, 2, 3, 5, 8, smallest .. largest |R| / bound over every entry:
    step 1   NONE 2.2e-4 .. 3.7e-4     HUBER 2.3e-4 .. 5.3e-4
    step 2   NONE 2.7e-4 .. 5.6e-4     HUBER 1.3e-4 .. 2.1e-4
(the MI355X launches of tests/test_gpu_series_bounds.py: 1.2e-4 to 8.2e-4 on the edge graphs, 3e-5 to 9e-5 on ladybug-49) --
the slack of the one-term bounds of test_rounding_bounds.py, since the bound is dominated by tb(x_0).

Mutations at term j in {1, 2, k // 2, k}, smallest |R| / bound over the 13 (k, j) pairs; every one is over its bound, so the
largest k stays 8 (each overwrite rule and each parity half is then reused more than twice):
                                      step 1 NONE   step 1 HUBER   step 2 NONE   step 2 HUBER
    stale z, one-observation camera   7.3e4         2.2e5          3.9e6         2.2e7
    stale z, hub                      6.0e7         1.6e7          9.0e7         3.6e7
    dropped observation of a hub      3.8e4         1.3e4          8.0e3         3.3e2
    dropped observation, tail camera  1.7e5         6.7e4          1.7e5         6.9e5
    dropped record of a hub           1.6e6         1.0e7          3.2e5         6.8e3
    landmark sums not re-zeroed       4.4e9         4.7e8          7.6e10        2.1e11
    stale record of a hub             2.2e5         3.0e5          1.2e5         2.8e3

The same runs against the relative 2-norm of the increment (1e-10 in test_gpu_res*.py): on THESE graphs none of the 364 runs
stays under 1e-10 -- the smallest move is 5.8e-8 (stale z of a one-observation camera at the last of eight terms, step 1), the
dropped hub observation moves it by 2e-7 to 6e-7.  At lambda = 1e-4 the under-determined cameras of the edge graphs carry a
large share of the increment, so a 2-norm would see these defects here as well, had the edge graphs ever gone through a
resident launch; what the identity adds is the margin where the 2-norm's depends on the camera's weight in the norm (a factor
575 over the tolerance against 7.3e4 over the bound for that stale z; for the dropped hub observation of step 2 HUBER the
2-norm has the larger margin, 2e3 against 3.3e2), an index (camera, entry) for every violation, and a tolerance that is
derived instead of chosen.

The reference magnitudes: an independent fp64 run's own terms in place of the long-double series move no entry of the bound by
more than 4.3e-11 of itself (step 1; 2.5e-12 step 2).  A bound carried term by term, e_i = tb(x_{i-1}) + |T|_abs e_{i-1}: median
e_i / |x_i| = 1.9e-7 .. 4.5e-7 at i = 1, 0.44 .. 4.9 at i = 2, 2e6 .. 7e8 at i = 3.
"""
import os

import numpy as np
import pytest

import rounding_bounds as RB
import series_bounds as SB

HERE = os.path.dirname(os.path.abspath(__file__))
KS = (1, 2, 3, 5, 8)
SEEDS = (0, 1, 2)
ALPHA, LAM = 0.01, 1e-4
SYSTEMS = [(1, "NONE"), (1, "HUBER"), (2, "NONE"), (2, "HUBER")]
_SYS = {}


def _system(step, robust):
    """(prob, binv, x0, reference series of 8 terms, clean emulations by (k, seed)); built once."""
    key = (step, robust)
    if key not in _SYS:
        if step == 1:
            prob, _, _ = RB.system(*RB.edge_problem(0), ALPHA, robust, RB.EDGE_HUBER)
            binv, x0 = SB.pose_closed_form(prob, LAM)
        else:
            prob = RB.system_joint(*RB.edge_problem_joint(0), RB.EDGE_LAM_H, robust, RB.EDGE_HUBER_H)
            binv, x0 = None, prob.t0
        _SYS[key] = (prob, binv, x0, SB.reference_series(prob, binv, x0, max(KS)), {})
    return _SYS[key]


def _clean(step, robust, k, seed):
    prob, binv, x0, ref, runs = _system(step, robust)
    if (k, seed) not in runs:
        runs[(k, seed)] = SB.emulate_series(prob, binv, x0, k, seed)
    return runs[(k, seed)]


def _ratio(step, robust, run, k):
    prob, binv, x0, ref, _ = _system(step, robust)
    R, bound = SB.launch_identity(prob, binv, x0, run["xk"], run["Sk"], k, ref=ref)
    return SB.check(R, bound)


def test_pose_closed_form_against_the_dense_restatement():
    """B^-1 and x_0 = B^-1 (-b) of series_bounds.pose_closed_form against oracle/povar_numpy.step1 (dense Jacobians) on the
    golden problem, NONE and a HUBER threshold that weights every observation; three emulated terms give its increment."""
    from oracle import povar_numpy as PN
    g = np.load(os.path.join(HERE, "golden", "step1_small_none.npz"))
    n_c, alpha = int(g["n_cams"]), float(g["alpha"])
    for robust, huber in (("NONE", 1.0), ("HUBER", 0.5)):
        s1 = PN.step1(alpha, n_c, g["lm_off"], g["cam_idx"], g["obs"], g["cams"], g["lms"], LAM, 3, norm=robust, huber=huber)
        prob, _, _ = RB.system(n_c, g["lm_off"], g["cam_idx"], g["obs"], g["cams"], g["lms"], alpha, robust, huber)
        binv, x0 = SB.pose_closed_form(prob, LAM)
        assert robust == "NONE" or (s1["w"] < 1).mean() > 0.5
        assert np.abs(binv.reshape(n_c, 144) - s1["b_inv"]).max() <= 1e-11 * np.abs(s1["b_inv"]).max()
        assert np.linalg.norm(x0 - s1["terms"][0]) <= 1e-11 * np.linalg.norm(x0)
        inc = SB.emulate_series(prob, binv, x0, 3)["Sk"]
        assert np.linalg.norm(inc - s1["inc"]) <= 1e-11 * np.linalg.norm(inc)


@pytest.mark.parametrize("step,robust", SYSTEMS)
def test_clean_emulations_within_the_launch_bound(step, robust):
    prob, binv, x0, ref, _ = _system(step, robust)
    worst, least = 0.0, np.inf
    for k in KS:
        for seed in SEEDS:
            run = _clean(step, robust, k, seed)
            r, i, n_over = _ratio(step, robust, run, k)
            assert n_over == 0, (k, seed, r, i // SB.dim(prob), i % SB.dim(prob))
            worst, least = max(worst, r), min(least, r)
    print(f"SERIESBOUND emulation step={step} {robust} clean |R|/bound: {least:.3g} .. {worst:.3g}")
    assert least > 1e-5  # (not vacuous: a clean run uses a visible share of its bound)
    if step == 2:  # (the camera without observations: its terms are exactly 0 and so is its bound beyond gamma_k |x_0|)
        assert all(np.all(t[-11:] == 0) for t in _clean(step, robust, max(KS), 0)["terms"][1:])


def _mutations(prob):
    one = int(np.flatnonzero(prob.n_c == 1)[0])
    hub = int(np.argmax(prob.n_c))
    hub_rows = np.flatnonzero(prob.cam_idx == hub)
    n_l = len(prob.n_l)
    rec = (n_l // 4, n_l // 4 + n_l // 8)  # (a contiguous eighth of the landmarks: one workgroup's share of eight)
    return {
        "stale_z/one-observation camera": dict(kind="stale_z", cam=one),
        "stale_z/hub": dict(kind="stale_z", cam=hub),
        "drop_obs/hub": dict(kind="drop_obs", obs=int(hub_rows[len(hub_rows) // 2])),
        "drop_obs/tail": dict(kind="drop_obs", obs=int(np.flatnonzero(prob.cam_idx == one)[0])),
        "drop_record/hub": dict(kind="drop_record", cam=hub, lms=rec),
        "no_rezero": dict(kind="no_rezero"),
        "stale_record/hub": dict(kind="stale_record", cam=hub, lms=rec),
    }


MUTATION_NAMES = ["stale_z/one-observation camera", "stale_z/hub", "drop_obs/hub", "drop_obs/tail", "drop_record/hub", "no_rezero",
                  "stale_record/hub"]


@pytest.mark.parametrize("name", MUTATION_NAMES)
@pytest.mark.parametrize("step,robust", SYSTEMS)
def test_mutation_at_any_term_breaks_the_launch_bound(step, robust, name):
    """Each defect at term j in {1, 2, k // 2, k} of a k-term launch: at least one entry of R over its bound.  (At j = 1 the
    launch finds what an earlier launch of max(KS) terms on the same system left -- a replayed context; after an earlier
    launch of the same k, a stale record of term 1 at k = 1 would hold the right numbers.)  The same runs against the
    relative 2-norm of the increment that test_gpu_res*.py use: the smallest deviation and how many stay under 1e-10 are printed."""
    prob, binv, x0, ref, _ = _system(step, robust)
    mut = _mutations(prob)[name]
    least, unseen, runs, dev = np.inf, 0, 0, np.inf
    prior = _clean(step, robust, max(KS), 0)["state"]
    for k in KS:
        clean = _clean(step, robust, k, 0)
        for j in sorted({1, 2, k // 2, k} & set(range(1, k + 1))):
            bad = SB.emulate_series(prob, binv, x0, k, 0, mutate=dict(mut, term=j), prior=prior)
            r, i, n_over = _ratio(step, robust, bad, k)
            assert n_over >= 1, (name, k, j, r)
            least = min(least, r)
            runs += 1
            d2 = float(np.linalg.norm(bad["Sk"] - clean["Sk"]) / np.linalg.norm(clean["Sk"]))
            dev = min(dev, d2)
            unseen += d2 < 1e-10
    print(f"SERIESMUT step={step} {robust} {name}: smallest |R|/bound={least:.3g}; 2-norm of the increment: smallest move {dev:.3g}, "
          f"under 1e-10: {unseen} of {runs}")


@pytest.mark.parametrize("step,robust", SYSTEMS)
def test_reference_magnitudes_against_an_fp64_runs_own(step, robust):
    """The bound's magnitudes |x_i| come from the long-double series; an independent fp64 run's own terms in their place
    move no entry of the bound by more than the (1 + 1e-6) the bound modules already apply."""
    prob, binv, x0, ref, _ = _system(step, robust)
    k = max(KS)
    run = _clean(step, robust, k, 1)
    _, bound = SB.launch_identity(prob, binv, x0, run["xk"], run["Sk"], k, ref=ref)
    own = dict(ref, x=[t.astype(SB.LD) for t in run["terms"]],
               tb=[SB.apply_ref(prob, binv, t, ref["model"])[1] for t in run["terms"][:k]])
    _, bound2 = SB.launch_identity(prob, binv, x0, run["xk"], run["Sk"], k, ref=own)
    ok = bound > 0
    move = float(np.abs(bound2[ok] / bound[ok] - 1).max())
    print(f"SERIESBOUND emulation step={step} {robust} bound with the run's own magnitudes: moves by {move:.3g}")
    assert np.array_equal(bound2 > 0, ok) and move < 1e-6


@pytest.mark.parametrize("step,robust", SYSTEMS)
def test_a_bound_carried_term_by_term_is_vacuous(step, robust):
    """Why the identity and not e_i = tb(x_{i-1}) + |T|_abs e_{i-1}: the median of e_i / |x_i| over the entries is printed for
    i = 1, 2, 3; by the third term the carried bound is larger than the term it bounds."""
    prob, binv, x0, ref, _ = _system(step, robust)
    e, med = np.zeros_like(ref["tb"][0]), []
    for i in range(1, 4):
        e = ref["tb"][i - 1] + SB.apply_ref(prob, binv, e, ref["model"])[2]
        xi = np.abs(ref["x"][i].astype(np.float64))
        med.append(float(np.median(e[xi > 0] / xi[xi > 0])))
    print(f"SERIESBOUND carried bound step={step} {robust} median e_i/|x_i|: " + ", ".join(f"i={i + 1}: {m:.3g}" for i, m in enumerate(med)))
    assert med[0] < 1e-6 and med[2] > 1.0
