"""NumPy reference of the solves and covariances with fixed cameras (povar_set_fixed_cameras), for the CPU and GPU tests.

A set F of whole cameras is held constant: every solve returns the increment of S_ff x_f = -b_f (f: the coordinates of the
free cameras) with zeros on F.  The device gets there without restricting anything: it zeroes the blocks of B^-1 (power
series) or of the Schur-Jacobi inverse (PCG) on F, or replaces the rows and columns of F in the dense matrix by the
identity's (CHOLESKY, covariance).  This module states both sides with the existing oracle binding:

* masked(blocks, F): the per-camera inverse blocks with zero blocks on F -- what Oracle.solve_pose / solve_joint / pcg take;
* restricted(S, dim, F), pad(x_f, ...): S_ff and the zero-padding of a vector or a matrix of the free coordinates;
* dense_e0(apply, n): the dense E0 behind the series, column by column through the oracle's right_mul_e0_*;
* restricted_series(...): the power series of S_ff = B_ff - E0_ff written out on the restricted dense matrices;
* decoupled(S, b, dim, F): the matrix and right-hand side CHOLESKY factors;
* covariance(S, dim, F): [S_ff]^-1 by covariance_reference.chol_inverse_longdouble, zero-padded (long double).

Systems and states are those of covariance_reference (system_pose / system_joint: ALPHA = 0.01, sigma = 1 / (1e-5 +
sqrt(diag2)), the step-2 state of state2).
"""
import numpy as np

import covariance_reference as R

ALPHA = R.ALPHA
# the fixed sets of the tests: two cameras of `small` (6 cameras: 1 in the first, 4 in the tail workgroup of cam_build_binv),
# three of p22 (camera 5 straddles row 64 of the factor in step 1)
SETS = {"small": (1, 4), "p22": (2, 3, 5)}


def free_coords(n_cams, dim, F):
    """Indices of the coordinates of the free cameras, ascending."""
    free = np.setdiff1d(np.arange(n_cams), np.asarray(F, dtype=np.int64))
    return (dim * free[:, None] + np.arange(dim)[None, :]).ravel()


def fixed_coords(n_cams, dim, F):
    F = np.unique(np.asarray(F, dtype=np.int64))
    return (dim * F[:, None] + np.arange(dim)[None, :]).ravel()


def masked(blocks, F):
    """A copy of per-camera blocks [n_cams, ...] with zero blocks on F."""
    out = np.array(blocks, dtype=np.float64, copy=True)
    out[np.asarray(F, dtype=np.int64)] = 0.0
    return out


def restricted(S, dim, F):
    f = free_coords(S.shape[0] // dim, dim, F)
    return S[np.ix_(f, f)]


def pad(x, n_cams, dim, F):
    """A vector (or square matrix) of the free coordinates, zero-padded to all of them."""
    f = free_coords(n_cams, dim, F)
    n = dim * n_cams
    if x.ndim == 1:
        out = np.zeros(n, dtype=x.dtype)
        out[f] = x
    else:
        out = np.zeros((n, n), dtype=x.dtype)
        out[np.ix_(f, f)] = x
    return out


def decoupled(S, b, dim, F):
    """(A, rhs): S and b with the rows and columns of F replaced by the identity's and rhs = 0 there."""
    k = fixed_coords(S.shape[0] // dim, dim, F)
    A, rhs = S.copy(), b.copy()
    A[k, :] = 0.0
    A[:, k] = 0.0
    A[k, k] = 1.0
    rhs[k] = 0.0
    return A, rhs


def dense_e0(apply, n):
    """The matrix of x -> apply(x), column by column."""
    E = np.zeros((n, n))
    for k in range(n):
        e = np.zeros(n)
        e[k] = 1.0
        E[:, k] = apply(e)
    return E


def restricted_series(binv, E0, b, dim, F, m):
    """sum_{i <= m} (B_ff^-1 E0_ff)^i B_ff^-1 (-b_f) on the explicitly restricted matrices, zero-padded: (sum, terms [m + 1, n])."""
    n_cams = binv.shape[0]
    f = free_coords(n_cams, dim, F)
    Bi = np.zeros((dim * n_cams, dim * n_cams))
    for c in range(n_cams):
        Bi[dim * c:dim * c + dim, dim * c:dim * c + dim] = binv[c].reshape(dim, dim)
    Bi_ff, E_ff = Bi[np.ix_(f, f)], E0[np.ix_(f, f)]
    t = Bi_ff @ (-b[f])
    terms = [t]
    for _ in range(m):
        t = Bi_ff @ (E_ff @ t)
        terms.append(t)
    terms = np.array(terms)
    return pad(terms.sum(0), n_cams, dim, F), np.array([pad(t, n_cams, dim, F) for t in terms])


def covariance(S, dim, F):
    """[S_ff]^-1 zero-padded, in long double, and (cond_2, |S_ff^-1|_2) of S_ff."""
    n_cams = S.shape[0] // dim
    Sff = restricted(S, dim, F)
    ev = np.linalg.eigvalsh(Sff)
    return pad(R.chol_inverse_longdouble(Sff), n_cams, dim, F), float(ev[-1] / ev[0]), float(1.0 / ev[0])


# ---- the power-series side of a problem, both steps: what the masked-oracle series and the restricted dense series need
def series_pose(p, lam, lms=None):
    """(orc, st, hll, b, binv [n_cams, 144], sigma, lms): LinearizorPowerVarproj's step-1 system at lam (tests/test_gpu_step1.py);
    landmarks from init_landmarks_pose unless given."""
    from oracle import povar_oracle as O
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    lms = orc.init_landmarks_pose(ALPHA, p.cams) if lms is None else np.asarray(lms, dtype=np.float64)
    st, diag2, jls, sigma, ok = orc.stage1_pose(ALPHA, p.cams, lms)
    orc.scale_jp_cols_pose(st, sigma)
    hll, b, binv = orc.prepare_hb_pose(st, lam, 0.0)
    return orc, st, hll, b, binv, sigma, lms


def series_joint(p, lam, state=None):
    """(orc, st_h, st_n, hll, b, binv [n_cams, 121], sigma, jls, cams, lms_h, obs): step 2's (tests/test_gpu_step2.py) at the
    state (cams, lms_h, obs) -- covariance_reference.state2 unless given."""
    from oracle import povar_oracle as O
    cams, lms_h, obs = R.state2(p) if state is None else state
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, obs)
    st_h, ok = orc.linearize_homogeneous(cams, lms_h)
    diag2 = orc.jp_diag2_homogeneous(st_h)
    jls = orc.scale_jl_cols_homogeneous(st_h)
    sigma = 1.0 / (1e-5 + np.sqrt(diag2))
    orc.scale_jp_cols_joint(st_h, sigma)
    st_n = orc.linearize_nullspace(cams, lms_h, st_h)
    hll, b, binv = orc.prepare_hb_joint(st_h, st_n, lam)
    return orc, st_h, st_n, hll, b, binv, sigma, jls, cams, lms_h, obs


def masked_series(p, step, lam, F, m, want_terms=True, state=None):
    """The oracle's own series with the blocks of B^-1 zeroed on F: (sum, terms, system) -- system as series_pose / series_joint
    (state: step 1 the landmarks, step 2 (cams, lms_h, obs))."""
    if step == 1:
        s = series_pose(p, lam, state)
        orc, st, hll, b, binv = s[:5]
        acc, it, status, terms = orc.solve_pose(st, hll, masked(binv, F), b, m, want_terms=want_terms)
    else:
        s = series_joint(p, lam, state)
        orc, st_h, st_n, hll, b, binv = s[:6]
        acc, it, status, terms = orc.solve_joint(st_n, hll, masked(binv, F), b, m, want_terms=want_terms)
    return acc, terms, s


# ---- covariance with fixed cameras: every output of the five families from one zero-padded C
class _Bound:
    def __init__(self, bound):
        self.bound = bound


class CovCase:
    """One case (problem, step, lambda, F) on the systems of landmark_covariance_reference / observation_covariance_reference:
    C = [S_ff(lam)]^-1 zero-padded (long double), the outputs of every covariance family fed that C through the existing
    reference modules' formulas, and their bounds with the matrices that are actually inverted: A = S_ff for the camera
    blocks (n u cond_2(A) |A^-1|_2, n = dim A: tests/test_gpu_camera_covariance.py), K = H(lam) without the rows and columns of
    the fixed cameras for everything that involves landmarks (m u cond_2(K) |K^-1|_2, m = dim K: the landmark,
    observation, hat and pair tests' rule)."""

    def __init__(self, name, step, lam, F):
        import landmark_covariance_reference as L
        import observation_covariance_reference as OC
        import pair_covariance_reference as PC
        self.name, self.step, self.lam, self.F = name, step, lam, tuple(F)
        self.sys = s = L.system(name, step)
        self.osys = osys = OC.obs_system(name, step)
        self.dim, self.n_cams, self.n_lms = s.dim, s.n_cams, s.n_lms
        S = s.reduced(lam).astype(np.float64)
        self.C, self.cond, self.inv_norm = covariance(S, s.dim, F)
        self.cam_blocks = R.blocks(self.C, s.dim)
        n_f = s.dim * (s.n_cams - len(set(F)))
        self.cam_unit = R.U * self.cond * self.inv_norm
        self.cam_bound = n_f * self.cam_unit
        keep = np.concatenate([free_coords(s.n_cams, s.dim, F), s.n + np.arange(3 * s.n_lms)])
        ev = np.linalg.eigvalsh(s.full(lam)[np.ix_(keep, keep)])
        self.m = keep.shape[0]
        self.full_unit = R.U * float(ev[-1] / ev[0]) * float(1.0 / ev[0])
        self.full_bound = self.m * self.full_unit
        self.rank = n_f + 3 * s.n_lms  # sum of the leverages: every free parameter is determined
        # landmarks
        self.lm_blocks = s.sigma_blocks(lam, False, C=self.C)
        # observations: (h, c_uu, c_uv, c_vv) and the hat blocks, the walk of ObsSystem.schur_rows / hat_reference.schur_blocks
        LD = np.longdouble
        hi = s.hll_inv(lam)
        self.obs_rows = np.zeros((osys.n_obs, 4), dtype=LD)
        self.hat_blocks = np.zeros((osys.n_obs, osys.d, osys.d), dtype=LD)
        for l in range(s.n_lms):
            idx = s.rows[l]
            Fl = s.Hpl[idx, 3 * l:3 * l + 3].astype(LD) @ hi[l]
            Cpp = self.C[np.ix_(idx, idx)]
            Cpl = -Cpp @ Fl
            Sl = hi[l] - Fl.T @ Cpl
            cams_of = idx[::osys.dim] // osys.dim
            for i in range(osys.lm_off[l], osys.lm_off[l + 1]):
                k = int(np.flatnonzero(cams_of == osys.cam_idx[i])[0]) * osys.dim
                r = slice(k, k + osys.dim)
                cov = np.block([[Cpp[r, r], Cpl[r]], [Cpl[r].T, Sl]])
                self.obs_rows[i] = osys._row(i, cov)
                Jw = osys.rows(i).astype(LD)
                self.hat_blocks[i] = Jw @ cov @ Jw.T
        self.obs_bound = osys.bound(_Bound(self.full_bound))
        nb = np.stack([np.linalg.norm(osys.rows(i), axis=1) for i in range(osys.n_obs)])
        self.hat_bound = self.full_bound * nb[:, :, None] * nb[:, None, :]
        # pairs: PairReference's formulas on this C (built without its constructor, which inverts the unrestricted system)
        pr = object.__new__(PC.PairReference)
        pr.sys, pr.step, pr.dim, pr.lam, pr.free_gauge = s, step, s.dim, lam, False
        pr.C, pr.hi = self.C, hi
        pr.F = [s.Hpl[s.rows[l], 3 * l:3 * l + 3].astype(LD) @ hi[l] for l in range(s.n_lms)]
        pr.bound = self.full_bound
        if step == 2:
            w, beta = R.householder(s.cams)
            pr.Nc = R.reflectors(w, beta)[:, :, 1:]
        self.pairs = pr


_COV = {}


def cov_case(name, step, lam, F):
    """Computed once per case, shared, never modified."""
    key = (name, step, lam, tuple(F))
    if key not in _COV:
        _COV[key] = CovCase(name, step, lam, F)
    return _COV[key]
