"""NumPy reference of the per-observation residuals, hat blocks and deletion statistics (povar_observation_hat_pose / _joint,
capi.deletion_statistics), for the CPU and GPU tests.  Builds on tests/observation_covariance_reference.py (ObsSystem: U_i, L_i,
A_i of every observation in the solver's scaled coordinates) and tests/landmark_covariance_reference.py (System, Reference: the
figures of the bound) and on the dense rows of oracle/povar_numpy.py.

For observation i of landmark l in camera c, J_i = A_i [U_i^T | L_i] (d x (DIM + 3); d = 4 in step 1, 2 in step 2) and
    P_ii = J_i Cov J_i^T,   r_i = the weighted residual of dense_pose / dense_homogeneous,
with Cov the covariance of the DIM + 3 parameters by the Schur route of ObsSystem.schur_rows in long double (C, Sigma_l and the
cross blocks -C F_l).  Gauge-invariant: [Q; -Hll^-1 Hlp Q] lies in the null space of J.

Bound of the GPU test, per entry (p, q) of P_ii: the project's first-order rule carried through the rows whose bilinear form
the entry is,
    |err| <= m u cond_2(K) |K^-1|_2 |b_p| |b_q|,    K, m, u as in landmark_covariance_reference.Reference,
with b_p, b_q the weighted rows of J_i.

The deletion statistic t_i = r_i^T (I - P_ii)^+ r_i and its rank come from the eigenpairs of the reference's I - P_ii (TOL_NULL
below: an eigenvalue under it is a null direction).  propagate() carries entry bounds of r and P through the statistic to first
order: with M = I - P_ii, z = M^+ r and N the projector on the null directions,
    dt = 2 z^T dr + z^T dP z + 2 (M^+ z)^T dP (N r),     so  |dt| <= 2 |z|^T Er + |z|^T EP |z| + 2 |M^+ z|^T EP |N r|,
(the last term is there for completeness: N r is rounding noise) where the host's own eigen-solver counts as one more
perturbation of M of 8 d u per entry (a backward-stable symmetric eigen-solver on a matrix of norm <= 1).
"""
import numpy as np

import landmark_covariance_reference as L
import observation_covariance_reference as O
from oracle import povar_numpy as PN

ALPHA, U = L.ALPHA, L.U
LD = np.longdouble
TOL_NULL, GAP = 1e-9, 1e-4  # every reference eigenvalue of I - P_ii is below the first or above the second (asserted by the tests)


def residuals(osys, name, norm):
    """[n_obs, d] weighted residuals at the linearisation point of the case, from the oracle's dense rows (fp64)."""
    p = L.problem(name)
    cams, lms, obs = L.state(p, osys.step)
    if osys.step == 1:
        r = PN.dense_pose(ALPHA, p.n_cams, osys.lm_off, osys.cam_idx, obs, cams, lms, norm, L.HUBER[1])[2]
    else:
        r = PN.dense_homogeneous(p.n_cams, osys.lm_off, osys.cam_idx, obs, cams, lms, norm, L.HUBER[2])[2]
    return np.asarray(r).reshape(osys.n_obs, osys.d)


def schur_blocks(osys, lam, free_gauge):
    """[n_obs, d, d] in long double: J_i Cov J_i^T with Cov = [[C_cc, -C F], [-F^T C, Sigma_l]] as ObsSystem.schur_rows forms it."""
    s = osys.sys
    hi = s.hll_inv(lam)
    C = s.camera_covariance(lam, free_gauge)
    out = np.zeros((osys.n_obs, osys.d, osys.d), dtype=LD)
    for l in range(s.n_lms):
        idx = s.rows[l]
        F = s.Hpl[idx, 3 * l:3 * l + 3].astype(LD) @ hi[l]
        Cpp = C[np.ix_(idx, idx)]
        Cpl = -Cpp @ F
        Sl = hi[l] - F.T @ Cpl
        cams_of = idx[::osys.dim] // osys.dim
        for i in range(osys.lm_off[l], osys.lm_off[l + 1]):
            k = int(np.flatnonzero(cams_of == osys.cam_idx[i])[0]) * osys.dim
            r = slice(k, k + osys.dim)
            cov = np.block([[Cpp[r, r], Cpl[r]], [Cpl[r].T, Sl]])
            Jw = osys.rows(i).astype(LD)
            out[i] = Jw @ cov @ Jw.T
    return out


def statistics(r, P, tol=TOL_NULL):
    """(t [n], rank [n], mu [n, d], V [n, d, d]) of the reference: the eigenpairs of I - P_ii in fp64 of the long-double blocks."""
    d = r.shape[1]
    M = np.eye(d)[None] - np.asarray(P, dtype=np.float64)
    mu, V = np.linalg.eigh(0.5 * (M + M.transpose(0, 2, 1)))
    keep = mu > tol
    proj = np.einsum("nkj,nk->nj", V, r)
    t = np.where(keep, proj ** 2 / np.where(keep, mu, 1.0), 0.0).sum(1)
    return t, keep.sum(1), mu, V


def propagate(r, mu, V, Er, EP, tol=TOL_NULL):
    """[n]: the first-order bound on |dt| of the module docstring from entry bounds Er [n, d] and EP [n, d, d]."""
    d = r.shape[1]
    keep = mu > tol
    proj = np.einsum("nkj,nk->nj", V, r)
    inv = np.where(keep, 1.0 / np.where(keep, mu, 1.0), 0.0)
    z = np.einsum("nkj,nj->nk", V, proj * inv)
    mz = np.einsum("nkj,nj->nk", V, proj * inv * inv)
    nr = np.einsum("nkj,nj->nk", V, np.where(keep, 0.0, proj))
    EP = EP + 8 * d * U
    za, mza, nra = np.abs(z), np.abs(mz), np.abs(nr)
    return (2 * (za * Er).sum(1) + np.einsum("np,npq,nq->n", za, EP, za) + 2 * np.einsum("np,npq,nq->n", mza, EP, nra)) * (1 + 1e-6)


class Reference:
    """Long-double blocks of one case, the oracle's residuals, the entry bound and the reference's statistic."""

    def __init__(self, name, step, norm, lam, free_gauge):
        self.osys = osys = O.obs_system(name, step, norm)
        self.lm_ref = lm_ref = L.reference(name, step, norm, lam, free_gauge)
        self.d = osys.d
        self.P = schur_blocks(osys, lam, free_gauge)
        self.r = residuals(osys, name, norm)
        nb = np.stack([np.linalg.norm(osys.rows(i), axis=1) for i in range(osys.n_obs)])
        self.bound = lm_ref.bound * nb[:, :, None] * nb[:, None, :]
        self.rank = osys.m - (osys.sys.Q.shape[1] if free_gauge else 0)
        self.t, self.rank_i, self.mu, self.V = statistics(self.r, self.P)
        self.two_view = np.repeat(np.diff(osys.lm_off) == 2, np.diff(osys.lm_off))


_REFS = {}


def reference(name, step, norm, lam, free_gauge):
    """Computed once per case, shared, never modified."""
    key = (name, step, norm, lam, free_gauge)
    if key not in _REFS:
        _REFS[key] = Reference(name, step, norm, lam, free_gauge)
    return _REFS[key]


# ------------------------------------------------------------------ the new row policy in fp64
def emulate(osys, r_unweighted, C, hi, uv, mutation=None):
    """obs_hat's row as the device evaluates it, in fp64, on top of ObsSystem.emulate's route to Syy_i: C [n, n] the camera
    covariance without the gauge correction, hi the Hll^-1 of the call.  r_unweighted [n, d] the residual without sqrt(w), uv the
    image points.  Returns (r [n, d], P [n, d, d]).  `mutation` breaks one thing:
      "no_offdiag"     the off-diagonal entries of P_ii dropped
      "unweighted_a"   A_i without sqrt(w)
      "unweighted_r"   the residual without sqrt(w)
      "uv_kept"        step 2's residual with uv not subtracted
      "half_factor"    A_i Syy_i returned without the right factor A_i^T (its leading d x d part)"""
    s, dim, d = osys.sys, osys.dim, osys.d
    n = osys.n_obs
    r_out, P_out = np.zeros((n, d)), np.zeros((n, d, d))
    for l in range(s.n_lms):
        tr = list(range(osys.lm_off[l], osys.lm_off[l + 1]))
        Hi = np.asarray(hi[l], dtype=np.float64)
        Us = [osys.Ut[i].T for i in tr]
        Ms = [osys.A[i].T @ osys.A[i] for i in tr]
        Gs = [Ms[a] @ osys.Lm[i] @ Hi for a, i in enumerate(tr)]
        blk = [slice(dim * osys.cam_idx[i], dim * osys.cam_idx[i] + dim) for i in tr]
        k = len(tr)
        K = [[Us[a].T @ C[blk[a], blk[b]] @ Us[b] for b in range(k)] for a in range(k)]
        Sl = Hi.copy()
        for a in range(k):
            for b in range(k):
                Sl += Gs[a].T @ K[a][b] @ Gs[b]
        for a, i in enumerate(tr):
            Ri = sum(K[a][b] @ Gs[b] for b in range(k))
            Lm = osys.Lm[i]
            Syy = K[a][a] + Lm @ Sl @ Lm.T - Ri @ Lm.T - Lm @ Ri.T
            Syy = np.triu(Syy) + np.triu(Syy, 1).T
            sw = np.sqrt(osys.w[i])
            A = osys.A[i] / sw if mutation == "unweighted_a" else osys.A[i]
            T = A @ Syy
            P = T @ A.T
            P = np.triu(P) + np.triu(P, 1).T
            if mutation == "no_offdiag":
                P = np.diag(np.diag(P))
            if mutation == "half_factor":
                P = T[:, :d] if d <= 3 else np.concatenate([T, np.zeros((d, d - 3))], 1)
            ru = r_unweighted[i]
            if mutation == "uv_kept" and osys.step == 2:
                ru = ru + uv[i]
            r_out[i] = ru if mutation == "unweighted_r" else sw * ru
            P_out[i] = P
    return r_out, P_out
