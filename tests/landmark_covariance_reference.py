"""NumPy reference of the per-landmark marginal covariance (povar_landmark_covariance_pose / _joint), for the CPU and GPU
tests.  Builds on the dense Jacobians of oracle/povar_numpy.py and on tests/covariance_reference.py (states, gauge bases,
long-double Cholesky inverse).

Everything is in the solver's Jacobi-scaled coordinates (step 2: the tangent coordinates of the reflector bases N_c, N_l):
    H(lam) = [[Hpp + lam I, Hpl], [Hlp, Hll + lam_l I]],   lam_l = 0 (step 1) or lam (step 2),
    S(lam) = Hpp + lam I - Hpl (Hll + lam_l I)^-1 Hlp,
    C      = S(lam)^-1 (damped)  or  S(0)^+ = (S0 + Q Q^T)^-1 - Q Q^T (free gauge),
    Sigma_l = Hll_l^-1 + F_l^T C F_l,   F_l = Hpl[:, l] Hll_l^-1.
Damped, Sigma_l is the (l, l) block of H^-1.  In the free gauge it is the landmark block of the covariance under the
constraint Q^T x_cameras = 0 (gauge fixed on the cameras: minimum norm over the camera parameters): the top-left part of
[[H0, Cg], [Cg^T, 0]]^-1 with Cg = [Q; 0] -- not the block of pinv(H0).

Bound of the GPU test, per block (the camera test's first-order rule carried to the full system):
    |Sigma^_l - Sigma_l|_F <= m u cond_2(K) |K^-1|_2,   K = H0 + Cg Cg^T (free gauge) or H(lam), m its dimension, u = 2^-53,
times max s_l^2 in landmark coordinates.
"""
import numpy as np

import covariance_reference as R
from oracle import povar_numpy as PN

ALPHA, U = R.ALPHA, R.U
HUBER = {1: 30.0, 2: 0.5}  # as tests/test_gpu_camera_covariance.py
EPS = 1e-5
LONG = (66, 300, 3000, 5)  # two landmarks of >= 65 observations, three of 33..64: both chunk loops of both stagings repeat


# `tracks`: 66 cameras, every track length at which obs_cov's loops turn (povar_kernels_cov.hpp:597-648): the generator's
# shortest track (2), the pass of 16 lanes groups (15, 16, 17), step 2's staging chunk of 32 (31, 32, 33), step 1's of 64
# (63, 64, 65; 65 is also three chunks of step 2).  The track of 17 is followed by another landmark (the rows after it
# exist).  The rest: eighty short tracks, so that every camera has the six observations its eleven step-2 parameters need.
TRACK_EDGES = (2, 17, 15, 16, 31, 32, 33, 63, 64, 65)
TRACKS = (66, 7)


def _tracks_problem():
    """A subgraph of the complete 66-camera graph of the generator with the prescribed track lengths (a seeded choice of the
    cameras of every landmark, ascending), so the image points are the generator's own projections."""
    from povar_amd import synth
    n_c, seed = TRACKS
    lengths = np.array(list(TRACK_EDGES) + [3 + i % 8 for i in range(80)])
    full = synth.make_problem(n_c, len(lengths), n_c * len(lengths), seed=seed, popularity="uniform")
    assert np.all(np.diff(full.lm_off) == n_c)
    rng = np.random.default_rng(seed)
    keep = np.concatenate([n_c * l + np.sort(rng.choice(n_c, size=k, replace=False)) for l, k in enumerate(lengths)])
    lm_off = np.zeros(len(lengths) + 1, dtype=np.int32)
    np.cumsum(lengths, out=lm_off[1:])
    # the generator's cameras have the third row (0, 0, 0, 1): y2 = 1 and 1 / y2 would be exact in every precision in step 1
    cams = full.cams.copy()
    cams[:, 8:11] = np.round(0.02 * rng.normal(size=(n_c, 3)), 6)
    cams[:, 11] = np.round(1 + 0.1 * rng.normal(size=n_c), 6)
    return synth.Problem(n_c, len(lengths), lm_off, np.ascontiguousarray(full.cam_idx[keep]), np.ascontiguousarray(full.obs[keep]),
                         cams, full.lms)


def problem(name):
    if name == "tracks":
        return _tracks_problem()
    if name == "long":
        from povar_amd import synth
        n_c, n_l, n_o, seed = LONG
        return synth.make_problem(n_c, n_l, n_o, seed=seed, popularity="uniform", long_track_frac=0.05)
    return R.problem(name)


def state(p, step):
    """(cams [n_cams, 12], landmarks [n_lms, 3 or 4], obs): the linearisation point of the step's tests."""
    if step == 1:
        cams = np.asarray(p.cams, dtype=np.float64).reshape(-1, 12)
        return cams, PN.init_landmarks_pose(ALPHA, p.lm_off, p.cam_idx, p.obs, cams), p.obs
    return R.state2(p)


def reflector_basis(x):
    """N = (I - beta w w^T)[:, 1:] of the vector x, w = x + sign(x0) |x| e0 (house4, orc_kernel_basis)."""
    x = np.asarray(x, dtype=np.float64)
    w = x.copy()
    w[0] += np.linalg.norm(x) if x[0] >= 0 else -np.linalg.norm(x)
    return (np.eye(x.shape[0]) - (2.0 / (w @ w)) * np.outer(w, w))[:, 1:]


def _null_basis(x, basis):
    if basis == "householder":
        return reflector_basis(x)
    import scipy.linalg
    return scipy.linalg.null_space(np.asarray(x)[None, :])


def _inv3_longdouble(A):
    A = A.astype(np.longdouble)
    X = np.linalg.inv(A.astype(np.float64)).astype(np.longdouble)
    I2 = 2 * np.eye(A.shape[0], dtype=np.longdouble)
    for _ in range(3):  # Newton: quadratic from an fp64 start
        X = X @ (I2 - A @ X)
    return X


class System:
    """The full scaled system of one case: Hpp, Hpl, Hll (fp64, undamped), the scales and bases, per-landmark row indices."""

    def __init__(self, p, step, norm="NONE", jl_scaling=None, basis="householder"):
        self.step, self.dim, self.n_cams, self.n_lms = step, 12 if step == 1 else 11, p.n_cams, p.lm_off.shape[0] - 1
        cams, lms, obs = state(p, step)
        self.cams, self.lms = cams, lms
        lm_off, cam_idx = np.asarray(p.lm_off), np.asarray(p.cam_idx)
        if step == 1:
            Jp, Jl = PN.dense_pose(ALPHA, p.n_cams, lm_off, cam_idx, obs, cams, lms, norm, HUBER[1])[:2]
            jl_scaling = True if jl_scaling is None else jl_scaling  # (the library's default; S itself does not depend on it)
        else:
            Jp, Jl = PN.dense_homogeneous(p.n_cams, lm_off, cam_idx, obs, cams, lms, norm, HUBER[2])[:2]
            jl_scaling = True
        self.sigma = (1.0 / (EPS + np.sqrt((Jp * Jp).sum(0)))).reshape(-1, 12)
        w = 3 if step == 1 else 4
        self.s = (1.0 / (EPS + np.sqrt((Jl * Jl).sum(0))) if jl_scaling else np.ones(Jl.shape[1])).reshape(-1, w)
        Jp, Jl = Jp * self.sigma.reshape(-1), Jl * self.s.reshape(-1)
        if step == 2:
            Nc = np.zeros((12 * p.n_cams, 11 * p.n_cams))
            for c in range(p.n_cams):
                Nc[12 * c:12 * c + 12, 11 * c:11 * c + 11] = _null_basis(cams[c], basis)
            self.Nl = np.stack([_null_basis(lms[l], basis) for l in range(self.n_lms)])
            Jp = Jp @ Nc
            Jl = np.concatenate([Jl[:, 4 * l:4 * l + 4] @ self.Nl[l] for l in range(self.n_lms)], axis=1)
        self.n = Jp.shape[1]
        self.Hpp, self.Hpl = Jp.T @ Jp, Jp.T @ Jl
        self.Hll = np.stack([Jl[:, 3 * l:3 * l + 3].T @ Jl[:, 3 * l:3 * l + 3] for l in range(self.n_lms)])
        self.rows = []
        for l in range(self.n_lms):
            cs = np.unique(cam_idx[lm_off[l]:lm_off[l + 1]])
            self.rows.append((self.dim * cs[:, None] + np.arange(self.dim)[None, :]).reshape(-1))
        self.track = np.diff(lm_off)
        self.Q = None
        if basis == "householder":
            V = R.gauge_basis_pose(cams, self.sigma) if step == 1 else R.gauge_basis_joint(cams, self.sigma)
            self.Q = R.orthonormal(V)

    def lam_l(self, lam):
        return 0.0 if self.step == 1 else lam

    def full(self, lam):
        """H(lam), cameras first."""
        m = self.n + 3 * self.n_lms
        H = np.zeros((m, m))
        H[:self.n, :self.n] = self.Hpp + lam * np.eye(self.n)
        H[:self.n, self.n:] = self.Hpl
        H[self.n:, :self.n] = self.Hpl.T
        for l in range(self.n_lms):
            a = self.n + 3 * l
            H[a:a + 3, a:a + 3] = self.Hll[l] + self.lam_l(lam) * np.eye(3)
        return H

    def gauge_border(self):
        """Cg = [Q; 0]."""
        Cg = np.zeros((self.n + 3 * self.n_lms, self.Q.shape[1]))
        Cg[:self.n] = self.Q
        return Cg

    def hll_inv(self, lam):
        return [_inv3_longdouble(self.Hll[l] + self.lam_l(lam) * np.eye(3)) for l in range(self.n_lms)]

    def reduced(self, lam, hi=None):
        """S(lam) in long double, landmark by landmark on the rows of its cameras."""
        hi = self.hll_inv(lam) if hi is None else hi
        S = (self.Hpp + lam * np.eye(self.n)).astype(np.longdouble)
        for l in range(self.n_lms):
            idx = self.rows[l]
            E = self.Hpl[idx, 3 * l:3 * l + 3].astype(np.longdouble)
            S[np.ix_(idx, idx)] -= E @ hi[l] @ E.T
        return S

    def camera_covariance(self, lam, free_gauge):
        """C in long double: S(lam)^-1, or (S0 + Q Q^T)^-1 - Q Q^T; for a basis without the analytic Q: pinv(S0)."""
        S = self.reduced(lam)
        if not free_gauge:
            return R.chol_inverse_longdouble(S)
        if self.Q is None:
            nq = 12 if self.step == 1 else 15
            ev, V = np.linalg.eigh(S.astype(np.float64))
            return ((V[:, nq:] / ev[nq:]) @ V[:, nq:].T).astype(np.longdouble)
        Ql = self.Q.astype(np.longdouble)
        return R.chol_inverse_longdouble(S + Ql @ Ql.T) - Ql @ Ql.T

    def sigma_blocks(self, lam, free_gauge, C=None):
        """[n_lms, 3, 3] in long double by the Schur formula."""
        hi = self.hll_inv(lam)
        C = self.camera_covariance(lam, free_gauge) if C is None else C
        out = np.zeros((self.n_lms, 3, 3), dtype=np.longdouble)
        for l in range(self.n_lms):
            idx = self.rows[l]
            F = self.Hpl[idx, 3 * l:3 * l + 3].astype(np.longdouble) @ hi[l]
            out[l] = hi[l] + F.T @ C[np.ix_(idx, idx)] @ F
        return out

    def to_landmark_coords(self, blocks):
        """Step 1: D Sigma D (3 x 3); step 2: D4 N_l Sigma N_l^T D4 (4 x 4)."""
        s = self.s.astype(blocks.dtype)
        if self.step == 2:
            N = self.Nl.astype(blocks.dtype)
            blocks = N @ blocks @ N.transpose(0, 2, 1)
        return s[:, :, None] * blocks * s[:, None, :]


def landmark_blocks(M, n, n_lms):
    """The 3 x 3 diagonal blocks of the landmark part of a full matrix (cameras first)."""
    return np.stack([M[n + 3 * l:n + 3 * l + 3, n + 3 * l:n + 3 * l + 3] for l in range(n_lms)])


class Reference:
    """Long-double landmark blocks of one case, the camera reference of the same system and the figures of the bound."""

    def __init__(self, sys_, lam, free_gauge):
        self.sys, self.lam, self.free_gauge = sys_, lam, free_gauge
        self.blocks = sys_.sigma_blocks(lam, free_gauge)
        K = sys_.full(lam)
        if free_gauge:
            Cg = sys_.gauge_border()
            K = K + Cg @ Cg.T
        ev = np.linalg.eigvalsh(K)
        self.m = K.shape[0]
        self.cond, self.inv_norm = float(ev[-1] / ev[0]), float(1.0 / ev[0])
        self.unit = U * self.cond * self.inv_norm
        self.bound = self.m * self.unit
        # the camera blocks of the same call: the camera test's reference and bound on the same reduced system
        self.cameras = R.Reference(sys_.reduced(lam).astype(np.float64), sys_.dim, sys_.Q if free_gauge else None)

    def scale(self, landmark_coords):
        return float(self.sys.s.max() ** 2) if landmark_coords else 1.0

    def want(self, landmark_coords):
        return self.sys.to_landmark_coords(self.blocks) if landmark_coords else self.blocks


# the cases of tests/test_gpu_landmark_covariance.py: (step, problem, norm, lam, free gauge)
GPU_CASES = ([(s, n, "NONE", 0.0, True) for s in (1, 2) for n in ("small", "p22", "p24", "long")] +
             [(s, "small", "HUBER", 0.0, True) for s in (1, 2)] +
             [(s, n, "NONE", lam, False) for s in (1, 2) for n in ("small", "medium") for lam in (1e-4, 1.0)])

_SYSTEMS, _REFS = {}, {}


def system(name, step, norm="NONE"):
    key = (name, step, norm)
    if key not in _SYSTEMS:
        _SYSTEMS[key] = System(problem(name), step, norm)
    return _SYSTEMS[key]


def reference(name, step, norm, lam, free_gauge):
    """Computed once per case, shared, never modified."""
    key = (name, step, norm, lam, free_gauge)
    if key not in _REFS:
        _REFS[key] = Reference(system(name, step, norm), lam, free_gauge)
    return _REFS[key]
