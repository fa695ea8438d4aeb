"""NumPy reference of the covariance blocks of parameter pairs (povar_covariance_blocks_pose / _joint), for the CPU and GPU
tests.  Builds on tests/landmark_covariance_reference.py (System, reference, problem; its caches are shared).

In the solver's coordinates, with C the camera covariance (System.camera_covariance: S(lam)^-1, or S0^+ in the free gauge),
hi_l = Hll_l^-1 (System.hll_inv) and F_l = Hpl[:, l] hi_l on the rows of the cameras of landmark l (the W_j of its observations
stacked):
    camera a, camera b        C[a, b]
    camera c, landmark l      -C[c, cams(l)] F_l                                   (DIM x 3; the transpose the other way round)
    landmark l, landmark m    delta_lm hi_l + F_l^T C[cams(l), cams(m)] F_m
Damped these are the blocks of H(lam)^-1; in the free gauge those of the covariance with the gauge fixed on the cameras,
K^-1 - n n^T with K = H0 + Cg Cg^T, Cg = [Q; 0], n = [Q; -F^T Q] (tests/test_pair_covariance_reference.py holds both).
Parameter coordinates: M_a T M_b^T with M_cam = D (step 1) or D N_c (step 2), M_lm = diag(s_l) or D4 N_l.

Bound of the GPU test, per block: |got - want|_F <= m u cond_2(K) |K^-1|_2 f_a f_b (landmark_covariance_reference.Reference.bound),
f = 1 in solver coordinates, f_cam = max sigma and f_lm = max s in parameter coordinates.
"""
import numpy as np

import covariance_reference as R
import landmark_covariance_reference as L

CAMERA, LANDMARK = 0, 1


class PairReference:
    """Long-double blocks of any pair of one case, on demand."""

    def __init__(self, name, step, norm, lam, free_gauge):
        self.ref = L.reference(name, step, norm, lam, free_gauge)  # the bound, and the camera / landmark references
        s = self.sys = self.ref.sys
        self.step, self.dim, self.lam, self.free_gauge = step, s.dim, lam, free_gauge
        self.C = s.camera_covariance(lam, free_gauge)
        self.hi = s.hll_inv(lam)
        self.F = [s.Hpl[s.rows[l], 3 * l:3 * l + 3].astype(np.longdouble) @ self.hi[l] for l in range(s.n_lms)]
        self.bound = self.ref.bound
        if step == 2:
            w, beta = R.householder(s.cams)
            self.Nc = R.reflectors(w, beta)[:, :, 1:]

    def _cam_rows(self, c):
        return np.arange(self.dim * c, self.dim * c + self.dim)

    def block(self, ka, a, kb, b):
        """Solver coordinates, long double."""
        s = self.sys
        if ka == CAMERA and kb == CAMERA:
            return self.C[np.ix_(self._cam_rows(a), self._cam_rows(b))]
        if ka == CAMERA:
            return -self.C[np.ix_(self._cam_rows(a), s.rows[b])] @ self.F[b]
        if kb == CAMERA:
            return self.block(kb, b, ka, a).T
        out = self.F[a].T @ self.C[np.ix_(s.rows[a], s.rows[b])] @ self.F[b]
        return out + self.hi[a] if a == b else out

    def side_map(self, kind, i):
        """M of one side in parameter coordinates: D or D N_c (12 x dim), diag(s_l) or D4 N_l (3 x 3 / 4 x 3)."""
        s = self.sys
        if kind == CAMERA:
            N = np.eye(12) if self.step == 1 else self.Nc[i]
            return (s.sigma[i][:, None] * N).astype(np.longdouble)
        N = np.eye(3) if self.step == 1 else s.Nl[i]
        return (s.s[i][:, None] * N).astype(np.longdouble)

    def want(self, pair, parameter_coords):
        ka, a, kb, b = (int(x) for x in pair)
        if ka == LANDMARK and kb == CAMERA:
            return self.want((kb, b, ka, a), parameter_coords).T
        T = self.block(ka, a, kb, b)
        if not parameter_coords:
            return T
        return self.side_map(ka, a) @ T @ self.side_map(kb, b).T

    def scale(self, pair, parameter_coords):
        """f_a f_b."""
        if not parameter_coords:
            return 1.0
        f = {CAMERA: float(self.sys.sigma.max()), LANDMARK: float(self.sys.s.max())}
        return f[int(pair[0])] * f[int(pair[2])]

    def smallest_diagonal_block(self):
        """min over the cameras' and the landmarks' own blocks of |Sigma_xx|_F, solver coordinates."""
        cams = [np.linalg.norm(self.block(CAMERA, c, CAMERA, c).astype(np.float64)) for c in range(self.sys.n_cams)]
        lms = [np.linalg.norm(self.block(LANDMARK, l, LANDMARK, l).astype(np.float64)) for l in range(self.sys.n_lms)]
        return float(min(min(cams), min(lms)))


# the cases of tests/test_gpu_pair_covariance.py: (step, problem, norm, lam, free gauge)
GPU_CASES = ([(s, "small", norm, 0.0, True) for s in (1, 2) for norm in ("NONE", "HUBER")] +
             [(s, n, "NONE", 0.0, True) for s in (1, 2) for n in ("p22", "tracks")] +
             [(s, n, "NONE", lam, False) for s in (1, 2) for n in ("small", "medium") for lam in (1e-4, 1.0)])

_REFS = {}


def reference(name, step, norm, lam, free_gauge):
    """Computed once per case, shared, never modified."""
    key = (name, step, norm, lam, free_gauge)
    if key not in _REFS:
        _REFS[key] = PairReference(name, step, norm, lam, free_gauge)
    return _REFS[key]


def all_pairs(n_cams, n_lms):
    """Every ordered pair of the three kinds: camera-camera, camera-landmark, landmark-landmark."""
    cc = [(CAMERA, a, CAMERA, b) for a in range(n_cams) for b in range(n_cams)]
    cl = [(CAMERA, c, LANDMARK, l) for c in range(n_cams) for l in range(n_lms)]
    ll = [(LANDMARK, l, LANDMARK, m) for l in range(n_lms) for m in range(n_lms)]
    return cc, cl, ll


def sample_pairs(rng, n_cams, n_lms, count):
    """`count` seeded pairs of each kind; the mixed ones in both orders."""
    cc = [(CAMERA, int(a), CAMERA, int(b)) for a, b in rng.integers(0, n_cams, size=(count, 2))]
    ll = [(LANDMARK, int(a), LANDMARK, int(b)) for a, b in rng.integers(0, n_lms, size=(count, 2))]
    cl = []
    for k, (c, l) in enumerate(zip(rng.integers(0, n_cams, size=count), rng.integers(0, n_lms, size=count))):
        cl.append((CAMERA, int(c), LANDMARK, int(l)) if k % 2 == 0 else (LANDMARK, int(l), CAMERA, int(c)))
    return cc, cl, ll
