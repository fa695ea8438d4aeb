"""Cases and references of the compacted dense system (povar_set_dense_compaction), for the CPU and GPU tests.

In mode 1 the dense matrix of CHOLESKY / RICHOLESKY and of the covariance calls spans the free cameras only, in ascending
camera id: A = S_ff.  The references are the existing ones, restricted:

* dense_case(case, step): the sc_bounds.System of the problem with S, ES, b, Eb indexed by the free coordinates and n, N those
  of the compact matrix -- what sc_bounds.factor_check holds POVAR_BUF_SC_FACTOR to;
* cov_case(case, step, lam): fixed_cameras_reference.CovCase of the problem and the case's fixed set -- the covariance outputs
  do not depend on the layout;
* expected_map(n_cams, dim, F, mode): what povar_dense_layout must return.

The problems are synth.make_problem(n_cams, n_lms, n_obs, seed), listed in PROBLEMS: this module builds them itself.  The
landmark, observation and pair reference classes are keyed by a problem name that they look up in covariance_reference.REGULAR;
p40 is not in that table, so cov_case() lends it the name for the duration of the construction alone (_lent) and keeps the
result in this module's own cache: the existing modules' tables and caches are as they were before and after.
Every case is chosen for an index path (what it hits):

  small   F = (1, 4)                       48 / 44 rows    one 64-block, padding inside it
  p22     F = (2, 3, 5)                    228 / 209       blocks straddle other 64-edges than in mode 0
  p24     F = (0, 23)                      264 / 242       first and last camera fixed; step 1 crosses the 256-row outer block
  p24s    F = (20 .. 23)                   240 / 220       a suffix: the compact matrix is a leading block of mode 0's
  p40     F = (0, 31, 32, 39)              432 / 396       both sides of sc_dense_ordered's 32-camera column tile
  p40w    all but (7, 8, 30, 33, 34)       60 / 55         a window: landmarks without a free camera
"""
import contextlib
import copy

import numpy as np

import covariance_reference as R
import fixed_cameras_reference as FR
import sc_bounds as SB

PROBLEMS = {"small": (6, 40, 150, 3), "p22": (22, 150, 1500, 5), "p24": (24, 200, 1600, 8), "p40": (40, 300, 2600, 13)}
LAM = 1e-4
WINDOW = (7, 8, 30, 33, 34)
# case -> (problem, F, compact rows of step 1, of step 2)
CASES = {
    "small": ("small", (1, 4), 48, 44),
    "p22": ("p22", (2, 3, 5), 228, 209),
    "p24": ("p24", (0, 23), 264, 242),
    "p24s": ("p24", (20, 21, 22, 23), 240, 220),
    "p40": ("p40", (0, 31, 32, 39), 432, 396),
    "p40w": ("p40", tuple(c for c in range(40) if c not in WINDOW), 60, 55),
}


def problem_of(case):
    return CASES[case][0]


def fixed_of(case):
    return list(CASES[case][1])


def rows_of(case, step):
    return CASES[case][2 if step == 1 else 3]


def synth_problem(name):
    from povar_amd import synth
    n_c, n_l, n_o, seed = PROBLEMS[name]
    return synth.make_problem(n_c, n_l, n_o, seed=seed)


def expected_map(n_cams, dim, F, mode):
    """(n, cam_row) of povar_dense_layout."""
    rows = np.full(n_cams, -1, dtype=np.int32)
    inside = np.arange(n_cams) if mode == 0 else np.setdiff1d(np.arange(n_cams), np.asarray(F, dtype=np.int64))
    rows[inside] = dim * np.arange(inside.shape[0])
    return dim * inside.shape[0], rows


_FULL, _DENSE, _PROBLEMS = {}, {}, {}


def full_system(name, step, shards=1):
    """sc_bounds.dense_system of the problem, unrestricted: computed once, shared, never modified."""
    key = (name, step, shards)
    if key not in _FULL:
        s = synth_problem(name)
        case = SB.pose_case(s, "NONE", LAM) if step == 1 else SB.joint_case(s, "NONE", LAM)
        _FULL[key] = SB.dense_system(case, step == 2, shards=shards)
    return _FULL[key]


def restrict(sy, F):
    """A copy of an sc_bounds.System with S, ES, b, Eb on the free coordinates and n, N of the compact matrix."""
    f = FR.free_coords(sy.p.n_cams, sy.dim, F)
    out = copy.copy(sy)
    out.S, out.ES = sy.S[np.ix_(f, f)], sy.ES[np.ix_(f, f)]
    out.b, out.Eb = np.asarray(sy.b)[f], np.asarray(sy.Eb)[f]
    out.n = f.shape[0]
    out.N = SB.padded(out.n)
    out.free = f
    return out


def dense_case(case, step, shards=1):
    key = (case, step, shards)
    if key not in _DENSE:
        _DENSE[key] = restrict(full_system(problem_of(case), step, shards), fixed_of(case))
    return _DENSE[key]


def cov_state_system(name):
    """sc_bounds.dense_system of step 1 at the linearisation point of the covariance tests (landmark_covariance_reference.state:
    the same cameras and landmarks, Jl column scaling left on), so that one context can serve a solve and a covariance call and
    both have their reference.  Computed once, shared, never modified."""
    import landmark_covariance_reference as L
    import operand_bounds as OB
    key = (name, "cov-state")
    if key not in _FULL:
        s = synth_problem(name)
        cams, lms, obs = L.state(s, 1)
        case = OB.Pose(s.n_cams, s.lm_off, s.cam_idx, obs, cams, lms, L.ALPHA, LAM, "NONE", SB.HUBER1, scale_jl=True)
        _FULL[key] = SB.dense_system(case, False)
    return _FULL[key]


@contextlib.contextmanager
def _lent(name):
    """A problem of PROBLEMS that covariance_reference.REGULAR does not hold is in that table while the block runs, and what the
    name-keyed modules cached under the name is dropped with it."""
    import landmark_covariance_reference as L
    import observation_covariance_reference as OC
    if name in R.REGULAR:
        assert R.REGULAR[name] == PROBLEMS[name]
        yield
        return
    R.REGULAR[name] = PROBLEMS[name]
    try:
        yield
    finally:
        del R.REGULAR[name]
        for cache in (L._SYSTEMS, OC._OBS, FR._COV):
            for key in [k for k in cache if k[0] == name]:
                del cache[key]


_COV = {}


def cov_case(case, step, lam):
    """fixed_cameras_reference.CovCase of the case: computed once, shared, never modified."""
    key = (case, step, lam)
    if key not in _COV:
        with _lent(problem_of(case)):
            _COV[key] = FR.CovCase(problem_of(case), step, lam, fixed_of(case))
    return _COV[key]


def conditioning(case, step, lam):
    """(smallest, largest eigenvalue) of S_ff(lam) from the oracle's system (covariance_reference.system_pose / system_joint)."""
    name = problem_of(case)
    if name not in _PROBLEMS:
        _PROBLEMS[name] = synth_problem(name)
    p = _PROBLEMS[name]
    S = (R.system_pose(p, lam) if step == 1 else R.system_joint(p, lam))[0]
    ev = np.linalg.eigvalsh(FR.restricted(np.asarray(S, dtype=np.float64), 12 if step == 1 else 11, fixed_of(case)))
    return float(ev[0]), float(ev[-1])
