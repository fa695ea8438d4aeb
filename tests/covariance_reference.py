"""NumPy reference of the per-camera marginal covariance (povar_camera_covariance_pose / _joint), for the CPU and GPU tests.

Everything is in the solver's Jacobi-scaled coordinates: S comes from the oracle's get_hb_pose / get_hb_joint, set up as
tests/test_gpu_sc_solvers.py does (ALPHA = 0.01, sigma = 1 / (1e-5 + sqrt(diag2)), step-2 state from _state2).

* gauge_basis_pose / gauge_basis_joint: the analytic null space of the undamped system S0,
    step 1: the affine gauge X -> A X that keeps the last homogeneous coordinate 1: for the 12 generators G = e_i e_j^T with
            i < 3, v_c = vec_rowmajor(-P_c G) / sigma_c;
    step 2: the projective gauge with the per-camera scale absorbed: for the 15 generators (i, j) != (3, 3),
            g = vec(-P_c G), h0 = first column of the reflector H = I - beta w w^T (N_c = H[:, 1:]),
            a = -(h0 . (g / sigma_c)) / (h0 . (P_c / sigma_c)), x_c = N_c^T ((g + a P_c) / sigma_c).
* the identity S0^+ = (S0 + Q Q^T)^-1 - Q Q^T with Q an orthonormal basis of that null space;
* chol_inverse_longdouble: the inverse through a Cholesky factor in long double (LAPACK through NumPy takes none);
* to_camera_coords: the map the device applies to a block: D T D (step 1), D N_c T N_c^T D (step 2).
"""
import numpy as np

ALPHA = 0.01
U = 2.0 ** -53

REGULAR = {"small": (6, 40, 150, 3), "p22": (22, 150, 1500, 5), "p24": (24, 200, 1600, 8)}
DEGENERATE = {"medium": (49, 300, 1230, 49)}


def problem(name):
    from povar_amd import synth
    n_c, n_l, n_o, seed = {**REGULAR, **DEGENERATE}[name]
    return synth.make_problem(n_c, n_l, n_o, seed=seed)


def state2(p, seed=11):
    """The step-2 state of tests/test_gpu_sc_solvers.py::_state2."""
    rng = np.random.default_rng(seed)
    cams = rng.normal(size=(p.n_cams, 12))
    cams[:, 8:11] *= 0.1
    cams[:, 11] = 5 + rng.random(p.n_cams)
    cams /= np.linalg.norm(cams, axis=1, keepdims=True)
    lms_h = np.concatenate([rng.normal(size=(p.n_lms, 3)), np.ones((p.n_lms, 1))], 1)
    return cams, lms_h, p.obs / 500.0


def householder(cams):
    """(w, beta) per camera, as the oracle's orc_kernel_basis: w = P + sign(P[0]) |P| e0, beta = 2 / w.w."""
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 12)
    w = cams.copy()
    nv = np.linalg.norm(cams, axis=1)
    w[:, 0] += np.where(cams[:, 0] >= 0, nv, -nv)
    return w, 2.0 / np.einsum("ci,ci->c", w, w)


def reflectors(w, beta):
    return np.eye(12)[None] - beta[:, None, None] * w[:, :, None] * w[:, None, :]


def system_pose(p, lam, norm="NONE", huber=30.0):
    """(S, sigma [n_cams, 12], cams, lms, b): step 1's reduced system at lam, no landmark damping."""
    from oracle import povar_oracle as O
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=norm, huber=huber)
    lms = orc.init_landmarks_pose(ALPHA, p.cams)
    st, ok = orc.linearize_pose(ALPHA, p.cams, lms)
    sigma = 1.0 / (1e-5 + np.sqrt(orc.jp_diag2_pose(st)))
    orc.scale_jp_cols_pose(st, sigma)
    S, b = orc.get_hb_pose(st, lam)
    return S, sigma.reshape(-1, 12), np.asarray(p.cams, dtype=np.float64).reshape(-1, 12), lms, b


def system_joint(p, lam, norm="NONE", huber=0.5):
    """(S, sigma, cams, lms_h, obs, b): step 2's tangent system at lam for cameras and landmarks."""
    from oracle import povar_oracle as O
    cams, lms_h, obs = state2(p)
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, obs, robust_norm=norm, huber=huber)
    st_h, ok = orc.linearize_homogeneous(cams, lms_h)
    diag2 = orc.jp_diag2_homogeneous(st_h)
    orc.scale_jl_cols_homogeneous(st_h)
    sigma = 1.0 / (1e-5 + np.sqrt(diag2))
    orc.scale_jp_cols_joint(st_h, sigma)
    st_n = orc.linearize_nullspace(cams, lms_h, st_h)
    S, b = orc.get_hb_joint(st_h, st_n, lam)
    return S, sigma.reshape(-1, 12), cams, lms_h, obs, b


def _generators(last_row):
    out = []
    for i in range(4 if last_row else 3):
        for j in range(4):
            if (i, j) != (3, 3):
                G = np.zeros((4, 4))
                G[i, j] = 1.0
                out.append(G)
    return out


def gauge_basis_pose(cams, sigma, generators=None):
    """n x 12 (not orthonormal): v = vec_rowmajor(-P_c G) / sigma_c stacked over the cameras, G = e_i e_j^T, i < 3."""
    P = np.asarray(cams, dtype=np.float64).reshape(-1, 3, 4)
    gens = _generators(False) if generators is None else generators
    return np.stack([(-(P @ G)).reshape(-1, 12) / sigma for G in gens], axis=-1).reshape(-1, len(gens))


def gauge_basis_joint(cams, sigma):
    """n x 15 (not orthonormal), n = 11 n_cams, in the tangent coordinates of the reflectors' N_c."""
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 12)
    P = cams.reshape(-1, 3, 4)
    w, beta = householder(cams)
    H = reflectors(w, beta)
    h0, N = H[:, :, 0], H[:, :, 1:]
    cols = []
    for G in _generators(True):
        g = (-(P @ G)).reshape(-1, 12)
        a = -np.einsum("ci,ci->c", h0, g / sigma) / np.einsum("ci,ci->c", h0, cams / sigma)
        cols.append(np.einsum("cij,ci->cj", N, (g + a[:, None] * cams) / sigma))
    return np.stack(cols, axis=-1).reshape(-1, 15)


def orthonormal(V):
    return np.linalg.qr(V)[0]


def null_dimension(S0):
    """Eigenvalues under 1e-10 of the largest (the gauge ones are rounding noise, the next one is >= 1e-2)."""
    ev = np.linalg.eigvalsh(S0)
    return int(np.sum(ev < 1e-10 * ev[-1])), ev


def chol_inverse_longdouble(A):
    """A^-1 of a symmetric positive definite matrix through A = R^T R, W = R^-1, A^-1 = W W^T, in long double;
    hand-written, vectorised by rows."""
    A = np.asarray(A, dtype=np.longdouble)
    n = A.shape[0]
    R = np.zeros_like(A)
    for k in range(n):
        d = A[k, k] - R[:k, k] @ R[:k, k]
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        R[k, k] = np.sqrt(d)
        R[k, k + 1:] = (A[k, k + 1:] - R[:k, k] @ R[:k, k + 1:]) / R[k, k]
    W = np.zeros_like(A)
    for k in range(n - 1, -1, -1):  # row k of W from R W = I
        e = np.zeros(n, dtype=np.longdouble)
        e[k] = 1
        W[k] = (e - R[k, k + 1:] @ W[k + 1:]) / R[k, k]
    return W @ W.T


def blocks(C, dim):
    n_c = C.shape[0] // dim
    return np.stack([C[dim * c:dim * c + dim, dim * c:dim * c + dim] for c in range(n_c)])


def to_camera_coords(T, sigma, step, cams=None):
    """Blocks [n_cams, dim, dim] -> [n_cams, 12, 12]: D T D (step 1), D N_c T N_c^T D (step 2)."""
    if step == 2:
        w, beta = householder(cams)
        N = reflectors(w, beta)[:, :, 1:].astype(T.dtype)
        T = N @ T @ N.transpose(0, 2, 1)
    s = sigma.astype(T.dtype)
    return s[:, :, None] * T * s[:, None, :]


class Reference:
    """Long-double reference blocks of one case and the figures the tolerance is made of."""

    def __init__(self, S, dim, Q=None):
        self.n = S.shape[0]
        A = S if Q is None else S + Q @ Q.T
        C = chol_inverse_longdouble(A)
        if Q is not None:
            Ql = Q.astype(np.longdouble)
            C = C - Ql @ Ql.T
        ev = np.linalg.eigvalsh(A)
        self.cond, self.inv_norm = float(ev[-1] / ev[0]), float(1.0 / ev[0])
        self.blocks = blocks(C, dim)
        # per block: |C^_cc - C_cc|_F <= n u cond_2(A) |A^-1|_2, first order, with the classical factor n
        self.bound = self.n * U * self.cond * self.inv_norm
        self.unit = U * self.cond * self.inv_norm  # the error ratios of DESIGN.md are stated in this unit
