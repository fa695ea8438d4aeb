"""NumPy reference of the per-observation leverage and predicted-point covariance (povar_observation_covariance_pose /
_joint), for the CPU and GPU tests.  Builds on tests/landmark_covariance_reference.py (System: the scaled full system, its
bases and gauge basis; Reference: the figures of the bound) and on the dense rows of oracle/povar_numpy.py.

Everything is in the solver's scaled coordinates (step 2: the tangent coordinates of N_c, N_l).  For observation i of landmark
l in camera c, with y = P_c X_l the projected homogeneous point (h = [X; 1] in step 1):
    dy   = U_i^T dp_c + L_i dl        U_i^T: 3 x DIM,  L_i: 3 x 3
    J_i  = A_i [U_i^T | L_i]          the d weighted residual rows (d = 4 in step 1, 2 in step 2),  M_i = A_i^T A_i
    Ju_i = Jpi_i [U_i^T | L_i]        Jpi = d(y0 / y2, y1 / y2) / dy: the two unweighted rows of the predicted image point
and the row of the call is (h, c_uu, c_uv, c_vv) = (tr(J_i Cov J_i^T), Ju_i Cov Ju_i^T) with Cov the covariance of the
parameters.  Three routes to Cov, all gauge-invariant on these rows:
    A  free gauge: the gauge fixed on the cameras, [[C, -C F], [-F^T C, Sigma]] by the Schur formulas in long double
       (C = (S0 + Q Q^T)^-1 - Q Q^T; landmark_covariance_reference.System);
    B  free gauge: J pinv(J^T J) J^T through the SVD of the dense J (fp64);
    D  damped: the long-double inverse of System.full(lam).  It is evaluated by block elimination of the 3 x 3 landmark
       blocks (exact algebra, every operation in long double: schur_rows); dense_inverse_rows inverts the assembled matrix
       as one block instead (the CPU test holds the two against each other on `small`).

Bound of the GPU test, per entry: the project's first-order rule carried through the rows whose quadratic form the entry is,
    |err| <= m u cond_2(K) |K^-1|_2 |b_p| |b_q|,    K, m, u as in landmark_covariance_reference.Reference,
summed over the d weighted rows J_i for h (p = q), with the two unweighted rows of Ju_i for c_uu, c_uv, c_vv.
"""
import numpy as np

import covariance_reference as R
import landmark_covariance_reference as L
from oracle import povar_numpy as PN

ALPHA, U = L.ALPHA, L.U
CHUNK = {1: 64, 2: 32}  # SCD_CHUNK, SCDH_CHUNK: the staging chunks of the kernel


def _jpi(y):
    return np.array([[1 / y[2], 0, -y[0] / y[2] ** 2], [0, 1 / y[2], -y[1] / y[2] ** 2]])


class ObsSystem:
    """Per-observation factors of one case on top of its landmark_covariance_reference.System."""

    def __init__(self, name, step, norm="NONE"):
        p = L.problem(name)
        self.sys = s = L.system(name, step, norm)
        self.step, self.d, self.dim = step, 4 if step == 1 else 2, s.dim
        cams, lms, obs = L.state(p, step)
        self.lm_off, self.cam_idx = np.asarray(p.lm_off), np.asarray(p.cam_idx)
        n_o, n_l = self.cam_idx.shape[0], s.n_lms
        self.n_obs = n_o
        self.lm_of = np.repeat(np.arange(n_l), np.diff(self.lm_off))
        if step == 1:
            self.w = PN.dense_pose(ALPHA, p.n_cams, self.lm_off, self.cam_idx, obs, cams, lms, norm, L.HUBER[1])[4]
        else:
            self.w = PN.dense_homogeneous(p.n_cams, self.lm_off, self.cam_idx, obs, cams, lms, norm, L.HUBER[2])[4]
        self.Nc = [L.reflector_basis(cams[c]) for c in range(p.n_cams)] if step == 2 else None
        self.Ut, self.Lm, self.A, self.Jpi = [], [], [], []
        for i in range(n_o):
            c, l = self.cam_idx[i], self.lm_of[i]
            P = cams[c].reshape(3, 4)
            sw = np.sqrt(self.w[i])
            if step == 1:
                h = np.append(lms[l], 1.0)
                Ut = np.kron(np.eye(3), h[None, :]) * s.sigma[c][None, :]
                Lm = P[:, :3] * s.s[l][None, :]
                A = sw * PN._A(ALPHA, *obs[i])
            else:
                h = lms[l]
                Ut = (np.kron(np.eye(3), h[None, :]) * s.sigma[c][None, :]) @ self.Nc[c]
                Lm = (P * s.s[l][None, :]) @ s.Nl[l]
                A = sw * _jpi(P @ h)
            self.Ut.append(Ut), self.Lm.append(Lm), self.A.append(A), self.Jpi.append(_jpi(P @ h))
        self.m = s.n + 3 * n_l

    def cols(self, i):
        c, l = self.cam_idx[i], self.lm_of[i]
        return np.concatenate([self.dim * c + np.arange(self.dim), self.sys.n + 3 * l + np.arange(3)])

    def rows(self, i, weighted=True):
        """J_i (d x (DIM + 3)) or Ju_i (2 x (DIM + 3)) on cols(i)."""
        return (self.A[i] if weighted else self.Jpi[i]) @ np.concatenate([self.Ut[i], self.Lm[i]], axis=1)

    def dense(self, weighted=True):
        d = self.d if weighted else 2
        J = np.zeros((d * self.n_obs, self.m))
        for i in range(self.n_obs):
            J[d * i:d * i + d, self.cols(i)] = self.rows(i, weighted)
        return J

    def _row(self, i, cov):
        """(h, c_uu, c_uv, c_vv) of observation i from the covariance `cov` of its DIM + 3 parameters."""
        Jw, Ju = self.rows(i).astype(cov.dtype), self.rows(i, False).astype(cov.dtype)
        Cu = Ju @ cov @ Ju.T
        return [np.trace(Jw @ cov @ Jw.T), Cu[0, 0], Cu[0, 1], Cu[1, 1]]

    def schur_rows(self, lam, free_gauge):
        """Routes A and D: [n_obs, 4] in long double from C, Sigma_l and the cross blocks -C F_l."""
        s = self.sys
        hi = s.hll_inv(lam)
        C = s.camera_covariance(lam, free_gauge)
        out = np.zeros((self.n_obs, 4), dtype=np.longdouble)
        for l in range(s.n_lms):
            idx = s.rows[l]
            F = s.Hpl[idx, 3 * l:3 * l + 3].astype(np.longdouble) @ hi[l]
            Cpp = C[np.ix_(idx, idx)]
            Cpl = -Cpp @ F
            Sl = hi[l] - F.T @ Cpl
            cams_of = idx[::self.dim] // self.dim
            for i in range(self.lm_off[l], self.lm_off[l + 1]):
                k = int(np.flatnonzero(cams_of == self.cam_idx[i])[0]) * self.dim
                r = slice(k, k + self.dim)
                cov = np.block([[Cpp[r, r], Cpl[r]], [Cpl[r].T, Sl]])
                out[i] = self._row(i, cov)
        return out

    def dense_inverse_rows(self, lam):
        """Route D as one block: the long-double Cholesky inverse of the assembled System.full(lam)."""
        Kinv = R.chol_inverse_longdouble(self.sys.full(lam))
        out = np.zeros((self.n_obs, 4), dtype=np.longdouble)
        for i in range(self.n_obs):
            cc = self.cols(i)
            out[i] = self._row(i, Kinv[np.ix_(cc, cc)])
        return out

    def pinv_rows(self):
        """Route B: J pinv(J^T J) J^T, pinv through the SVD of J with the rank m - nq; (rows [n_obs, 4] fp64, rank)."""
        J = self.dense()
        _, sv, Vt = np.linalg.svd(J, full_matrices=False)
        rank = self.m - self.sys.Q.shape[1]
        assert sv[rank - 1] > 1e-6 * sv[0] and (rank == sv.shape[0] or sv[rank] < 1e-10 * sv[0]), "rank J"
        Z = Vt[:rank].T / sv[:rank]  # pinv(H) = Z Z^T
        out = np.zeros((self.n_obs, 4))
        for i in range(self.n_obs):
            cc = self.cols(i)
            a, b = self.rows(i) @ Z[cc], self.rows(i, False) @ Z[cc]
            Cu = b @ b.T
            out[i] = [np.sum(a * a), Cu[0, 0], Cu[0, 1], Cu[1, 1]]
        return out, rank

    def bound(self, ref):
        """[n_obs, 4]: m u cond_2(K) |K^-1|_2 |b_p| |b_q| summed over the rows of each entry (ref: the landmark Reference)."""
        out = np.zeros((self.n_obs, 4))
        for i in range(self.n_obs):
            nw = np.linalg.norm(self.rows(i), axis=1)
            nu = np.linalg.norm(self.rows(i, False), axis=1)
            out[i] = [np.sum(nw * nw), nu[0] * nu[0], nu[0] * nu[1], nu[1] * nu[1]]
        return ref.bound * out

    # ------------------------------------------------------------------ the kernel's formula in fp64
    def emulate(self, C, hi, mutation=None):
        """obs_cov as the device evaluates it, in fp64: C [n, n] the camera covariance without the gauge correction, hi the
        Hll^-1 of the call; the pair walk over every j in chunks, Sigma_l with nq = 0.  `mutation` breaks one thing:
          "no_cross"      the cross term - R_i L_i^T - L_i R_i^T dropped
          "transposed"    K_ij used transposed for i > j
          "second_chunk"  the second chunk of j skipped in R_i
          "corrected"     Sigma_l taken with the - T_l^T T_l correction while R_i has none
          "weighted"      the weighted rows used for c_*"""
        s, dim = self.sys, self.dim
        chunk = CHUNK[self.step]
        out = np.zeros((self.n_obs, 4))
        for l in range(s.n_lms):
            tr = list(range(self.lm_off[l], self.lm_off[l + 1]))
            Hi = np.asarray(hi[l], dtype=np.float64)
            Us = [self.Ut[i].T for i in tr]
            Ms = [self.A[i].T @ self.A[i] for i in tr]
            Gs = [Ms[a] @ self.Lm[i] @ Hi for a, i in enumerate(tr)]
            blk = [slice(dim * self.cam_idx[i], dim * self.cam_idx[i] + dim) for i in tr]
            k = len(tr)
            K = [[Us[a].T @ C[blk[a], blk[b]] @ Us[b] for b in range(k)] for a in range(k)]
            Sl = Hi.copy()
            for a in range(k):
                for b in range(k):
                    Sl += Gs[a].T @ K[a][b] @ Gs[b]
            if mutation == "corrected":
                T = sum(s.Q[blk[a]].T @ Us[a] @ Gs[a] for a in range(k))
                Sl -= T.T @ T
            for a, i in enumerate(tr):
                Ri = np.zeros((3, 3))
                for jc in range(0, k, chunk):
                    if mutation == "second_chunk" and jc == chunk:
                        continue
                    for b in range(jc, min(k, jc + chunk)):
                        Kab = K[b][a] if (mutation == "transposed" and a > b) else K[a][b]
                        Ri += Kab @ Gs[b]
                Lm = self.Lm[i]
                Syy = K[a][a] + Lm @ Sl @ Lm.T
                if mutation != "no_cross":
                    Syy = Syy - Ri @ Lm.T - Lm @ Ri.T
                Jpi = self.Jpi[i] * (np.sqrt(self.w[i]) if mutation == "weighted" else 1.0)
                Cu = Jpi @ Syy @ Jpi.T
                out[i] = [np.sum(Ms[a] * Syy), Cu[0, 0], Cu[0, 1], Cu[1, 1]]
        return out

    def emulation_operands(self, lam, free_gauge):
        """(C, Hll^-1) in fp64 as the device holds them: (S0 + Q Q^T)^-1 without the correction, or S(lam)^-1."""
        s = self.sys
        hi = s.hll_inv(lam)
        S = s.reduced(lam, hi)
        if free_gauge:
            Ql = s.Q.astype(np.longdouble)
            S = S + Ql @ Ql.T
        return R.chol_inverse_longdouble(S).astype(np.float64), [h.astype(np.float64) for h in hi]


class Reference:
    """Long-double rows of one case and their bound."""

    def __init__(self, osys, lm_ref, lam, free_gauge):
        self.osys, self.lm_ref, self.lam, self.free_gauge = osys, lm_ref, lam, free_gauge
        self.rows = osys.schur_rows(lam, free_gauge)
        self.bound = osys.bound(lm_ref)
        self.rank = osys.m - (osys.sys.Q.shape[1] if free_gauge else 0)


# the cases of tests/test_gpu_observation_covariance.py: (step, problem, norm, lam, free gauge)
GPU_CASES = ([(s, n, "NONE", 0.0, True) for s in (1, 2) for n in ("small", "p22", "long")] +
             [(s, "small", "HUBER", 0.0, True) for s in (1, 2)] +
             [(s, n, "NONE", lam, False) for s in (1, 2) for n in ("small", "medium") for lam in (1e-4, 1.0)])

_OBS, _REFS = {}, {}


def obs_system(name, step, norm="NONE"):
    key = (name, step, norm)
    if key not in _OBS:
        _OBS[key] = ObsSystem(name, step, norm)
    return _OBS[key]


def reference(name, step, norm, lam, free_gauge):
    """Computed once per case, shared, never modified."""
    key = (name, step, norm, lam, free_gauge)
    if key not in _REFS:
        _REFS[key] = Reference(obs_system(name, step, norm), L.reference(name, step, norm, lam, free_gauge), lam, free_gauge)
    return _REFS[key]
