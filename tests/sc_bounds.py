"""Componentwise bounds for the explicit-Schur-complement path (povar_sc.hip, povar_kernels_sc.hpp, povar_kernels_chol.hpp):
the dense reduced camera matrix S of CHOLESKY / RICHOLESKY entry by entry, the block diagonal B_c and the Schur-Jacobi
preconditioner S_cc^-1 of PCG / RIPCG, and the factor R with its two triangular solves (helper module of
tests/test_sc_bounds.py and tests/test_gpu_sc_bounds.py; not a test module).  Conventions of operand_bounds.py: LD, g(k)
rounded up, first order, a final factor 1 + 1e-6; inputs are only what the caller set (an operand_bounds.Pose / Joint).  The
operands the kernels read -- weights and rho, sigma, the Jl scale s, Hll^-1, the camera reflectors, b, the Hpp moments -- come
from operand_bounds.pose_operands / joint_operands together with their bounds, which enter here as operand perturbations.

One form for both steps.  Per observation i of camera c and landmark l the kernels stage a 3 x 3 matrix F_i, G_i = F_i Hll^-1
and three dim-vectors u_a (a = 0..2); the contribution of the pair (i, j) of one landmark to the block (c_i, c_j) is
    -sum_ab u_a(i) T_ab u_b(j)^T,  T = G_i F_j^T            i.e.  -W_i Z_j^T  with  W_i = U_i^T G_i,  Z_j = U_j^T F_j  (dim x 3).
With magnitudes Fm, Gm = Fm |Hll^-1|, Um and operand errors EF, EG = EF |Hi| + Fm E(Hi) + g3 Gm, EU:
    Mag = Wm Zm^T,   E(pair) = EW Zm^T + Wm EZ^T + g(k_v + 3) Mag,   EW = EU^T Gm + Um^T EG,   EZ = EU^T Fm + Um^T EF
(T's three-term dot: 3; k_v: what the pair loop does with T and the vectors).
  step 1  scd_stage (povar_kernels_sc.hpp:529-549): F = w (C P3) diag(s).  sb sb: g4 + 1 (operand_bounds: dsb); cu = sb2 u: 6;
          cuv = sb2 (u u + v v): 8; the three-term dot C P3: 3; w = sw sw: 1 and 2 rho; the product with w: 1; with s: 1 and
          E(s) / s:  EF = Fm (g14 + 2 rho + E(s_j) / s_j).  G (:547): three-term dot, g3.  sc_dense_offdiag (:576-583):
          v = -t h h sigma_i sigma_j: k_v = 4; u_a = sigma_c o (e_a (x) h) is exact given sigma: EU = E(sigma) |h|.
  step 2  scdh_stage (:624-664): F rows 0, 1 = sw D00 jl3 (2 products), row 2 = sw (D02 jl3_0 + D12 jl3_1) (4), with D's and
          jl3's errors of operand_bounds.joint_operands (E00, E02, E12, ejl3) and rho of sw.  u_a = N_c^T (sigma o (e_a (x) X))
          (:649-662): the product (1), the four-term dot (4), two products and the difference (3): g8 and the device's
          reflector dNc on |N_c|^T |v|, plus |N_c|^T (E(sigma) |X|).  sc_dense_offdiag_h (:692-703): T (3), then
          a_r (T0 v0 + T1 v1 + T2 v2) summed over three rows: 3 + 1 + 2: k_v = 6.
The atomics sum in any order: per entry g over (the number of landmarks that contribute + 1 for sc_dense_diag + 1 per extra
shard) on the sum of the magnitudes, B_c's included; E(S) adds E(B_c).  An entry no landmark touches is exactly 0; the block
of a camera nobody observes is exactly lambda I (0 + lambda) and its right-hand side exactly 0.  The rhs column is -b with
b = POVAR_BUF_B / B_JOINT bit for bit (sc_dense_diag :599): E(b) is operand_bounds' bound.

BLOCKDIAG  cam_build_sc<HOM> with dm = null (:164-215): operand_bounds' B of B_INV / B_INV_JOINT with the REFERENCE's sigma:
          E(B) = sigma sigma (E(moments) + g(n_c + 9 | n_c + 4) |moments|) + (E(sigma_i) / sigma_i + E(sigma_k) / sigma_k) |.|
          (+ the two reflector products of step 2, 2 (g16 + dNc) on |N_c|^T (sigma |A| sigma) |N_c|, :199-208: a twelve-term
          dot, two products, the difference) + u |B_jj| for lambda.
PRECOND   S_cc = B_c - (E0 diagonal) from the sixty cm_gram_sc moments (:50-137), cam_sum_parts60 (:141-156), cam_build_sc with
          dm (:192).  The summand K_i (x) h h^T has the magnitude of the i == j pair above (w^2 |C| |P3 s| |Hi| |P3 s|^T |C| =
          Fm |Hi| Fm^T; step 2: w |Dm|^T |jl3| |Hi| |jl3|^T |Dm|).  Roundings per summand, step 1: M = P3 s twice (2), MH and A
          (6), C twice (16), CA, K's dot and w2 (7), w and w2 (2, 4 rho), hh and K hh (2), v - dm and two sigmas (3): 38
          against the pair form's 14 + 14 + 3 + 3 + 4 = 38: two more are charged.  Step 2: V, W (6), K (7), w (1), hh, K hh (2),
          v - dm, two sigmas (3): 19 against 18, and the two reflector products at g15 + dNc against the vectors' g8 + dNc:
          sixteen more are charged.  The sum over the camera: g(n_c + 1) (any order; lambda).
          E(S_cc) = E(B_c) + sum_i (E(pair i i) + g(2 | 16) Mag_ii) + g(n_c + 1) sum_i Mag_ii.
          The check is operand_bounds.binv_check's right residual with S_cc,ref: cam_build_sc's Cholesky solves per column
          (:216-243), Higham 2nd ed. Thm 10.3 / 10.4: |S_cc,ref X_dev - I|_ij <= sum_k (g(3 dim + 1) sqrt(S_ii S_kk) + E(S_cc)_ik)
          |X_dev|_kj, and |X - X^T| <= |X| R + (|X| R)^T.

FACTOR    chol_factor (povar_sc.hip) is right-looking with panels of 64 inside blocks of 256.  Entry (i, j), i <= j, of
          the augmented matrix (j = N: the rhs) receives, in this order: one `*cp -= acc` of chol_syrk_outer per finished
          block (povar_kernels_chol.hpp:196-204; acc: 256 products in any order, MFMA accumulation included), one of chol_syrk
          per earlier panel of its own block (:127-135; 64 products), i mod 64 steps `a -= r r` of chol_diag (:56) or chol_trsm
          (:82), then the division by r_ii (:53, :79) or the root (:52).  A product r_ki r_kj passes at most K (its accumulation
          group: 256 once a block is finished, else 64, else 0) + the later subtractions; S_ij passes every subtraction and
          the division.  Normalised so that S_ij stays unperturbed (Higham Lemma 8.4):
              k_f(i) = K + 2 (i div 256 + (i mod 256) div 64) + 3 (i mod 64) + 2
              |S_ref - R^T R|_ij <= g(k_f(i)) (|R^T| |R|)_ij + E(S)_ij            (Thm 10.3)
              |b_ref + R^T y|_i  <= g(k_f(i)) (|R^T| |y|)_i + E(b)_i              (the rhs column)
          Back substitution (:213-243): row i takes one `x[row] -= s` per later panel (s: 64 products through wave_sum), then
          chol_back_solve's wave_sum, difference and division:  k_b(i) = 64 + 2 (N / 64 - 1 - i div 64) + 4,
              |R x - y|_i <= g(k_b(i)) (|R| |x|)_i                               (Thm 8.5)
          with the device's own R, y, x: no condition number.  The padding is exact: rows and columns [n, N) of R are the
          identity, y and x are 0 there.  R^T R is formed without rounding (exact_gram: four 19-bit slices per column, every
          slice product exact in fp64 for N <= 2048); what the slices leave out is bounded entrywise and added to the bound,
          as is the long-double rounding of the matrix-vector products.

Emulations (fp64 NumPy, the kernels' operation order, two summation orders) and the mutation list: at the end.
"""
import numpy as np

import operand_bounds as OB
import rounding_bounds as RB
from operand_bounds import F, LD, _ab, _f, g
from rounding_bounds import U64, ULD

CH_NB, CH_OB, CH_T = 64, 256, 128
ONE = 1 + 1e-6


def padded(n):
    return (n + CH_NB - 1) // CH_NB * CH_NB


# ======== per-observation pieces
class Pieces:
    """F, G, U (long double) with their magnitudes and operand errors, [n_obs, 3, 3] and [n_obs, 3, dim]."""


def _finish_pieces(q, Hi, EHi, u):
    q.G = np.einsum("nik,nkj->nij", q.F, Hi)
    q.Gm = np.einsum("nik,nkj->nij", q.Fm, _ab(Hi))
    q.EG = np.einsum("nik,nkj->nij", q.EF, _ab(Hi)) + np.einsum("nik,nkj->nij", q.Fm, EHi) + g(3, u) * q.Gm
    q.W, q.Z = np.einsum("nap,nam->npm", q.U, q.G), np.einsum("nap,nam->npm", q.U, q.F)
    q.Wm, q.Zm = np.einsum("nap,nam->npm", q.Um, q.Gm), np.einsum("nap,nam->npm", q.Um, q.Fm)
    q.EW = np.einsum("nap,nam->npm", q.EU, q.Gm) + np.einsum("nap,nam->npm", q.Um, q.EG)
    q.EZ = np.einsum("nap,nam->npm", q.EU, q.Fm) + np.einsum("nap,nam->npm", q.Um, q.EF)
    return q


def _hi_of(p, R, mutate):
    ch = R.aux["chain"]
    Hi, EHi = ch["Hi"], ch["EHi"]
    if "hll_undamped" in mutate:  # one landmark's Hll^-1 without lambda on its diagonal
        l = mutate["hll_undamped"]
        H = R.aux["H"][l:l + 1] - LD(p.lam_lm) * np.eye(3, dtype=LD)[None]
        Hi = Hi.copy()
        Hi[l] = OB.inv3_bound(H, np.zeros((1, 3, 3)))[0][0]
    return Hi[p.lm], EHi[p.lm]


def _sigma_obs(p, R, mutate):
    ch = R.aux["chain"]
    sig, Esig = ch["sig"][p.cam_idx].copy(), ch["Esig"][p.cam_idx]
    if "sigma_row" in mutate:  # one row of one observation's vectors scaled by another camera's sigma
        o, r, c2 = mutate["sigma_row"]
        sig[o, r] = ch["sig"][c2, r]
    return sig, Esig


def pieces_pose(p, R, u=U64, mutate=None):
    mutate = mutate or {}
    ch = R.aux["chain"]
    c, lm = p.cam_idx, p.lm
    n = len(c)
    q = Pieces()
    q.dim, q.kv, q.extra = 12, 4, 2
    w, rho, sb2 = ch["w"], ch["rho"], ch["sb2"]
    uv = p.obs.astype(LD)
    Uc, Vc = uv[:, 0], uv[:, 1]
    C = np.zeros((n, 3, 3), dtype=LD)
    C[:, 0, 0] = C[:, 1, 1] = 1
    C[:, 0, 2] = C[:, 2, 0] = -sb2 * Uc
    C[:, 1, 2] = C[:, 2, 1] = -sb2 * Vc
    C[:, 2, 2] = sb2 * (Uc * Uc + Vc * Vc)
    P3 = p.cams[c].reshape(n, 3, 4)[:, :, :3]
    s, ds = ch["s"][lm], (ch["Es"] / _f(ch["s"]))[lm]
    q.F = w[:, None, None] * np.einsum("nik,nkj->nij", C, P3.astype(LD)) * s[:, None, :]
    q.Fm = _f(w)[:, None, None] * np.einsum("nik,nkj->nij", _ab(C), np.abs(P3)) * _f(s)[:, None, :]
    q.EF = q.Fm * ((g(14, u) + 2 * rho)[:, None, None] + ds[:, None, :])
    h = np.concatenate([p.lms[lm].astype(LD), np.ones((n, 1), dtype=LD)], 1)
    sig, Esig = _sigma_obs(p, R, mutate)
    q.U, q.EU = np.zeros((n, 3, 12), dtype=LD), np.zeros((n, 3, 12))
    for a in range(3):
        q.U[:, a, 4 * a:4 * a + 4] = sig[:, 4 * a:4 * a + 4] * h
        q.EU[:, a, 4 * a:4 * a + 4] = Esig[:, 4 * a:4 * a + 4] * _ab(h)
    q.Um = _ab(q.U)
    q.h = h
    return _finish_pieces(q, *_hi_of(p, R, mutate), u)


def pieces_joint(p, R, u=U64, mutate=None):
    mutate = mutate or {}
    ch = R.aux["chain"]
    c, lm = p.cam_idx, p.lm
    n = len(c)
    q = Pieces()
    q.dim, q.kv, q.extra = 11, 6, 16
    sw, rho, D, A, E = ch["sw"], ch["rho"], ch["D"], ch["A"], ch["E"]
    jl3, jl3a, ejl3 = ch["jl3"], ch["jl3a"], ch["ejl3"]
    swa = _f(sw)
    q.F, q.Fm, q.EF = np.zeros((n, 3, 3), dtype=LD), np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    for k in range(2):
        q.F[:, k] = (sw * D[0])[:, None] * jl3[k]
        q.Fm[:, k] = (swa * A[0])[:, None] * jl3a[k]
        q.EF[:, k] = swa[:, None] * (A[0][:, None] * ejl3[k] + E[0][:, None] * jl3a[k]) + (g(2, u) + rho)[:, None] * q.Fm[:, k]
    q.F[:, 2] = sw[:, None] * (D[1][:, None] * jl3[0] + D[2][:, None] * jl3[1])
    q.Fm[:, 2] = swa[:, None] * (A[1][:, None] * jl3a[0] + A[2][:, None] * jl3a[1])
    q.EF[:, 2] = swa[:, None] * (A[1][:, None] * ejl3[0] + A[2][:, None] * ejl3[1] + E[1][:, None] * jl3a[0] + E[2][:, None] * jl3a[1]) \
        + (g(4, u) + rho)[:, None] * q.Fm[:, 2]
    X = p.lms[lm].astype(LD)
    sig, Esig = _sigma_obs(p, R, mutate)
    cw, cb = ch["cw"][c], ch["cb"][c]
    cwa, cba = _ab(cw), _f(cb)
    dnc = R.aux["dnc"]
    q.U, q.Um, q.EU = np.zeros((n, 3, 11), dtype=LD), np.zeros((n, 3, 11)), np.zeros((n, 3, 11))
    for a in range(3):
        v, Ev = np.zeros((n, 12), dtype=LD), np.zeros((n, 12))
        v[:, 4 * a:4 * a + 4] = sig[:, 4 * a:4 * a + 4] * X
        Ev[:, 4 * a:4 * a + 4] = Esig[:, 4 * a:4 * a + 4] * _ab(X)
        q.U[:, a] = OB._nt12(cw, cb, v)
        q.Um[:, a] = OB._nt12(cwa, cba, _ab(v), +1)
        q.EU[:, a] = OB._nt12(cwa, cba, Ev, +1) + (g(8, u) + dnc) * q.Um[:, a]
    q.h = X
    return _finish_pieces(q, *_hi_of(p, R, mutate), u)


# ======== the block diagonal B_c with the reference's sigma
def _hpp_joint(Gx):
    nC = Gx.shape[0]
    Hh = np.zeros((nC, 3, 4, 3, 4), dtype=Gx.dtype)
    Hh[:, 0, :, 0, :] = Gx[:, 0]
    Hh[:, 1, :, 1, :] = Gx[:, 0]
    Hh[:, 2, :, 2, :] = Gx[:, 3]
    for k in range(2):
        Hh[:, k, :, 2, :] = Gx[:, k + 1]
        Hh[:, 2, :, k, :] = Gx[:, k + 1]
    return Hh.reshape(nC, 12, 12)


def blockdiag(p, R, joint, u=U64):
    """(B_c [n_cams, dim, dim] long double, E(B_c), the ambient sigma Hpp sigma) -- module docstring: BLOCKDIAG."""
    ch = R.aux["chain"]
    sig, rs = ch["sig"], ch["Esig"] / _f(ch["sig"])
    ss = _f(sig)[:, :, None] * _f(sig)[:, None, :]
    rr = rs[:, :, None] + rs[:, None, :]
    seen = (p.n_c > 0)[:, None, None]
    if not joint:
        sb2 = ch["sb2"]
        Hpp, Hm, EH = OB._hpp_pose(ch["G"], sb2), np.abs(OB._hpp_pose(ch["Gm"], float(sb2))), np.abs(OB._hpp_pose(ch["EG"], float(sb2)))
        SAS = sig[:, :, None] * Hpp * sig[:, None, :]
        B = SAS + LD(p.lam) * np.eye(12, dtype=LD)[None]
        EB = ss * (EH + g(p.n_c + 9, u)[:, None, None] * Hm) + ss * Hm * rr + u * _ab(B) * np.eye(12)[None]
        return B, np.where(seen, EB, 0.0) * ONE, SAS
    cw, cb = ch["cw"], ch["cb"]
    cwa, cba = _ab(cw), _f(cb)
    SAS = sig[:, :, None] * _hpp_joint(ch["G"]) * sig[:, None, :]
    SASm = ss * _hpp_joint(ch["Gm"])
    ESAS = ss * (_hpp_joint(ch["EG"]) + g(p.n_c + 4, u)[:, None, None] * _hpp_joint(ch["Gm"])) + SASm * rr
    B = OB._ntan(cw, cb, SAS) + LD(p.lam) * np.eye(11, dtype=LD)[None]
    EB = OB._ntan(cwa, cba, ESAS, +1) + 2 * (g(16, u) + R.aux["dnc"]) * OB._ntan(cwa, cba, SASm, +1) + u * _ab(B) * np.eye(11)[None]
    return B, np.where(seen, EB, 0.0) * ONE, SAS


SYM6 = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
SYM10 = np.array([[0, 1, 2, 3], [1, 4, 5, 6], [2, 5, 7, 8], [3, 6, 8, 9]])


def e0_diagonal(p, R, q, joint, u=U64, mutate=None):
    """(E0's diagonal blocks [n_cams, dim, dim] long double through the sixty moments, their error E) -- PRECOND."""
    mutate = mutate or {}
    ch = R.aux["chain"]
    n = len(p.cam_idx)
    K = np.einsum("nam,nbm->nab", q.G, q.F)
    hh = q.h[:, :, None] * q.h[:, None, :]
    summand = (K[:, :, None, :, None] * hh[:, None, :, None, :]).reshape(n, 12, 12)
    amb = OB.csum(p, summand)
    if "moment_last" in mutate:  # one cm_gram_sc moment of one camera without its last summand
        cam, k6, j10 = mutate["moment_last"]
        last = int(np.flatnonzero(p.cam_idx == cam)[-1])
        m6 = np.kron(SYM6 == k6, np.ones((4, 4), dtype=bool))
        m10 = np.kron(np.ones((3, 3), dtype=bool), SYM10 == j10)
        amb = amb.copy()
        amb[cam] = amb[cam] - np.where(m6 & m10, summand[last], LD(0))
    sig = ch["sig"]
    D0 = sig[:, :, None] * amb * sig[:, None, :]
    if joint:
        D0 = OB._ntan(ch["cw"], ch["cb"], D0)
    mag = np.einsum("npm,nqm->npq", q.Wm, q.Zm)
    e = np.einsum("npm,nqm->npq", q.EW, q.Zm) + np.einsum("npm,nqm->npq", q.Wm, q.EZ) + g(q.kv + 3 + q.extra, u) * mag
    return D0, (OB.csum(p, e) + g(p.n_c + 1, u)[:, None, None] * OB.csum(p, mag)) * ONE


# ======== the dense system
class System:
    pass


def _lm_index(p, l, dim):
    a, b = int(p.lm_off[l]), int(p.lm_off[l + 1])
    cams = p.cam_idx[a:b]
    assert (np.diff(cams) > 0).all(), "cameras ascend inside a landmark (sc_dense_offdiag keeps camera_i <= camera_j)"
    rows = (dim * cams[:, None] + np.arange(dim)[None, :]).ravel()
    return a, b, rows, np.kron(np.triu(np.ones((b - a, b - a))), np.ones((dim, dim)))


def _upper_sym(A):
    return np.triu(A) + np.triu(A, 1).T


def dense_system(p, joint, shards=1, u=U64, mutate=None, R=None):
    """References and bounds of one prepared system (module docstring).  mutate: reference-side defects (mutations())."""
    mutate = mutate or {}
    if R is None:
        R = (OB.joint_operands if joint else OB.pose_operands)(p, u=u)
    q = (pieces_joint if joint else pieces_pose)(p, R, u, mutate)
    dim = q.dim
    n = dim * p.n_cams
    sy = System()
    sy.p, sy.R, sy.q, sy.joint, sy.dim, sy.n, sy.N, sy.u, sy.shards = p, R, q, joint, dim, n, padded(n), u, shards
    S, Sm, ES, cnt = np.zeros((n, n), dtype=LD), np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    gk = g(q.kv + 3, u)
    for l in range(p.n_lms):
        a, b, rows, mask = _lm_index(p, l, dim)
        k = b - a
        blk = -(q.W[a:b].reshape(k * dim, 3) @ q.Z[a:b].reshape(k * dim, 3).T)
        if mutate.get("pair_dropped", (None,))[0] == l:
            _, i, j = mutate["pair_dropped"]
            blk.reshape(k, dim, k, dim)[i, :, j, :] = 0
        if mutate.get("pair_transposed", (None,))[0] == l:
            _, i, j = mutate["pair_transposed"]
            b4 = blk.reshape(k, dim, k, dim)
            b4[i, :, j, :] = b4[i, :, j, :].T.copy()
        Wm, Zm = q.Wm[a:b].reshape(k * dim, 3), q.Zm[a:b].reshape(k * dim, 3)
        mag = Wm @ Zm.T
        e = q.EW[a:b].reshape(k * dim, 3) @ Zm.T + Wm @ q.EZ[a:b].reshape(k * dim, 3).T + gk * mag
        ix = np.ix_(rows, rows)
        S[ix] += blk * mask.astype(LD)
        Sm[ix] += mag * mask
        ES[ix] += e * mask
        cnt[ix] += mask
    B, EB, _ = blockdiag(p, R, joint, u)
    for c in range(p.n_cams):
        sl = slice(dim * c, dim * c + dim)
        S[sl, sl] += B[c]
        Sm[sl, sl] += _ab(B[c])
        ES[sl, sl] += EB[c]
    ksum = np.where(cnt > 0, cnt + shards, 0.0)
    sy.S, sy.Sm, sy.cnt = _upper_sym(S), _upper_sym(Sm), _upper_sym(cnt)
    sy.ES = _upper_sym(ES + g(ksum, u) * Sm) * ONE
    bn = "B_JOINT" if joint else "B"
    sy.b, sy.Eb = R.ref[bn], R.bound[bn]
    sy.B, sy.EB = B, EB
    sy.E0d, EE0 = e0_diagonal(p, R, q, joint, u, mutate)
    sy.Scc, sy.EScc = B - sy.E0d, EB + EE0
    return sy


def diag_blocks(A, dim):
    return np.stack([A[dim * c:dim * c + dim, dim * c:dim * c + dim] for c in range(A.shape[0] // dim)])


def precond_check(sy, X_dev):
    """(residual, its bound, |X - X^T|, its bound), [n_cams, dim, dim] each -- module docstring: PRECOND."""
    R = OB.Ref()
    R.aux["P"] = dict(B=sy.Scc, EB=sy.EScc, n=sy.dim, u=sy.u)
    return OB.binv_check(R, "P", sy.p, X_dev)


# ======== the factor
def exact_gram(R):
    """(R^T R in long double, an entrywise bound on what is missing from it): every column of R is cut into four slices of
    19 bits below the column's largest exponent; a product of two slices is a multiple of its unit below 2^40, and a sum
    of N <= 2048 of them stays below 2^51: every fp64 slice product is exact.  The sixteen products are added in long double
    (sixteen roundings); the remainders of the slicing enter the bound."""
    R = np.asarray(R, dtype=F)
    N = R.shape[0]
    assert N <= 2048 and np.all(np.isfinite(R))
    cmax = np.abs(R).max(0)
    e = np.where(cmax > 0, np.ceil(np.log2(np.where(cmax > 0, cmax, 1.0))) + 1, 0.0)  # |R_kj| < 2^e_j
    rem, sl = R.copy(), []
    for s in range(4):
        unit = np.exp2(e - 19 * (s + 1))[None, :]
        t = np.rint(rem / unit) * unit
        sl.append(t)
        rem = rem - t
    out = np.zeros((N, N), dtype=LD)
    for a in sl:
        for b in sl:
            out += (a.T @ b).astype(LD)
    Ra, ra = np.abs(R), np.abs(rem)
    miss = (Ra.T @ ra + ra.T @ Ra + ra.T @ ra) * ONE
    return out, miss + 16 * ULD * (Ra.T @ Ra) * ONE


def k_factor(N):
    i = np.arange(N)
    K = np.where(i >= CH_OB, CH_OB, np.where(i >= CH_NB, CH_NB, 0))
    return K + 2 * (i // CH_OB + (i % CH_OB) // CH_NB) + 3 * (i % CH_NB) + 2


def k_back(N):
    i = np.arange(N)
    return CH_NB + 2 * (N // CH_NB - 1 - i // CH_NB) + 4


def factor_check(sy, buf, bd_dev=None):
    """The checks of module docstring: FACTOR on the device's [N, N + 2] buffer.  Returns {name: (err, bound)} with
    'factor' [n, n] (upper triangle; the strict lower is 0 / 0), 'forward' [n], 'back' [N], and 'padding': a list of
    messages about the exact facts that do not hold (empty: all hold).  With the device's BLOCKDIAG also 'chains'
    [n_cams, dim, dim]: |diag block of R^T R - (BLOCKDIAG_dev - E0 diagonal_ref)|, i.e. the dense assembly's diagonal blocks
    (sc_dense_diag + the i == j terms of sc_dense_offdiag[_h], as the factor reproduces them) against the block diagonal
    cam_build_sc wrote, inside the sum of their two bounds."""
    n, N, u = sy.n, sy.N, sy.u
    buf = np.asarray(buf, dtype=F)
    assert buf.shape == (N, N + 2)
    R, y, x = np.triu(buf[:, :N]), buf[:, N], buf[:, N + 1]
    out, pad = {}, []
    if not np.all(np.isfinite(R)) or not np.all(np.isfinite(y)) or not np.all(np.isfinite(x)):
        pad.append("non-finite entries in R, y or x")
        R, y, x = np.nan_to_num(R), np.nan_to_num(y), np.nan_to_num(x)
    RtR, miss = exact_gram(R)
    Ra = np.abs(R)
    A = Ra.T @ Ra
    kf, kb = k_factor(N), k_back(N)
    gf = np.triu(np.broadcast_to(g(kf, u)[:, None], (N, N)))[:n, :n]
    up = np.triu(np.ones((n, n), dtype=bool))
    err = _ab(sy.S - RtR[:n, :n])
    out["factor"] = (np.where(up, err, 0.0), np.where(up, (gf * A[:n, :n] + sy.ES + miss[:n, :n]) * ONE, 0.0))
    Rl, yl, xl = R.astype(LD), y.astype(LD), x.astype(LD)
    fwd = _ab(sy.b + (Rl.T @ yl)[:n])
    out["forward"] = (fwd, ((g(kf[:n], u) + N * ULD) * (Ra.T @ np.abs(y))[:n] + sy.Eb) * ONE)
    out["back"] = (_ab(Rl @ xl - yl), (g(kb, u) + N * ULD) * (Ra @ np.abs(x)) * ONE)
    for i in range(n, N):
        if R[i, i] != 1.0 or np.any(R[i, i + 1:] != 0.0) or np.any(R[:i, i] != 0.0):
            pad.append(f"padding row / column {i} of R is not the identity's")
        if y[i] != 0.0 or x[i] != 0.0:
            pad.append(f"padding entry {i}: y = {y[i]}, x = {x[i]}")
    out["padding"] = pad
    if bd_dev is not None:
        gv = g(kf, u)
        G2 = np.minimum(gv[:, None], gv[None, :])  # (entries (i, j) and (j, i) are one number: its row is min(i, j))
        bound = diag_blocks((G2 * A + miss)[:n, :n] + sy.ES, sy.dim) + sy.EB
        bd = np.asarray(bd_dev, dtype=F).reshape(-1, sy.dim, sy.dim).astype(LD)
        out["chains"] = (_ab(diag_blocks(RtR[:n, :n], sy.dim) - (bd - sy.E0d)), bound * ONE)
    return out


def worst(err, bound):
    """(largest err / bound over the entries with a positive bound or error, flat index, number of entries over)."""
    err, bound = np.asarray(err, dtype=F).reshape(-1), np.asarray(bound, dtype=F).reshape(-1)
    over = ~(err <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / bound, 0.0)
    r = np.where(np.isnan(r), np.inf, r)
    i = int(np.argmax(r)) if r.size else 0
    return (float(r[i]) if r.size else 0.0), i, int(over.sum())


def flagged(err, bound):
    """The flat indices over their bound."""
    err, bound = np.asarray(err, dtype=F).reshape(-1), np.asarray(bound, dtype=F).reshape(-1)
    return set(np.flatnonzero(~(err <= bound)).tolist())


# ======== fp64 emulations in the kernels' operation order
def _emu_pieces_pose(p):
    """scd_stage / cm_gram_sc<false> operands in fp64 from operand_bounds.emulate_pose's sigma, s, Hll^-1."""
    em = OB.emulate_pose(p, "obs")
    c, lm = p.cam_idx, p.lm
    n = len(c)
    sa, sb = np.sqrt(p.alpha), np.sqrt(1.0 - p.alpha)
    P, X, U, V = p.cams[c], p.lms[lm], p.obs[:, 0], p.obs[:, 1]
    h = np.concatenate([X, np.ones((n, 1))], 1)
    Pr = [P[:, 4 * k:4 * k + 4] for k in range(3)]
    if p.robust == "HUBER":
        m0, m1 = sb * (Pr[0] - Pr[2] * U[:, None]), sb * (Pr[1] - Pr[2] * V[:, None])
        res = [RB._dot(m0, h), RB._dot(m1, h), RB._dot(sa * Pr[0], h) - sa * U, RB._dot(sa * Pr[1], h) - sa * V]
        r2 = res[0] * res[0] + res[1] * res[1] + res[2] * res[2] + res[3] * res[3]
        sw = np.sqrt(np.where(r2 < p.huber * p.huber, 1.0, p.huber / np.sqrt(r2)))
    else:
        sw = np.ones(n)
    w = sw * sw
    sb2 = sb * sb
    cu, cv, cuv = sb2 * U, sb2 * V, sb2 * (U * U + V * V)
    C = np.zeros((n, 3, 3))
    C[:, 0, 0] = C[:, 1, 1] = 1
    C[:, 0, 2] = C[:, 2, 0] = -cu
    C[:, 1, 2] = C[:, 2, 1] = -cv
    C[:, 2, 2] = cuv
    P3 = P.reshape(n, 3, 4)[:, :, :3]
    s = em["JL_COL_SCALE"].reshape(-1, 3)[lm]
    Hi = em["HLL_INV"].reshape(-1, 3, 3)[lm]
    q = Pieces()
    q.dim = 12
    CP = C[:, :, 0, None] * P3[:, None, 0, :] + C[:, :, 1, None] * P3[:, None, 1, :] + C[:, :, 2, None] * P3[:, None, 2, :]
    q.F = w[:, None, None] * CP * s[:, None, :]
    q.G = q.F[:, :, 0, None] * Hi[:, None, 0, :] + q.F[:, :, 1, None] * Hi[:, None, 1, :] + q.F[:, :, 2, None] * Hi[:, None, 2, :]
    sig = em["SIGMA"].reshape(-1, 12)
    q.U = np.zeros((n, 3, 12))
    for a in range(3):
        q.U[:, a, 4 * a:4 * a + 4] = sig[c][:, 4 * a:4 * a + 4] * h
    m = np.stack([w, w * U, w * V, w * (U * U + V * V)], 1)
    Gm = OB._add_at(p.n_cams, c, m[:, :, None, None] * (h[:, :, None] * h[:, None, :])[:, None])
    q.h, q.em, q.sig, q.hpp = h, em, sig, OB._hpp_pose(Gm, sb2)
    q.sw, q.sb = sw, sb  # (what obs_cov's lane 0 reads again: cov_bounds.emulate_observations)
    return q


def _emu_pieces_joint(p):
    """scdh_stage / cm_gram_sc<true> operands in fp64 from operand_bounds.emulate_joint's sigma, s, Hll^-1, reflectors."""
    em = OB.emulate_joint(p)
    c, lm = p.cam_idx, p.lm
    n = len(c)
    P, X = p.cams[c], p.lms[lm]
    Pr = [P[:, 4 * k:4 * k + 4] for k in range(3)]
    px, py, pz = (RB._dot(Pr[k], X) for k in range(3))
    r0, r1 = px / pz - p.obs[:, 0], py / pz - p.obs[:, 1]
    D00, D02, D12 = 1 / pz, -px / (pz * pz), -py / (pz * pz)
    r2 = r0 * r0 + r1 * r1
    w = np.where(r2 < p.huber * p.huber, 1.0, p.huber / np.sqrt(np.maximum(r2, 1e-300))) if p.robust == "HUBER" else np.ones(n)
    sw = np.sqrt(w)
    s = em["JL_COL_SCALE_H"].reshape(-1, 4)[lm]
    jl4 = [sw[:, None] * (D00[:, None] * Pr[0] + D02[:, None] * Pr[2]) * s, sw[:, None] * (D00[:, None] * Pr[1] + D12[:, None] * Pr[2]) * s]
    lw, lb = RB.house4(p.lms)
    wl, bl = lw[lm], lb[lm]
    jl3 = [j[:, 1:] - (bl * RB._dot(j, wl))[:, None] * wl[:, 1:] for j in jl4]
    Hi = em["HLL_INV"].reshape(-1, 3, 3)[lm]
    q = Pieces()
    q.dim = 11
    q.F = np.stack([(sw * D00)[:, None] * jl3[0], (sw * D00)[:, None] * jl3[1], sw[:, None] * (D02[:, None] * jl3[0] + D12[:, None] * jl3[1])], 1)
    q.G = q.F[:, :, 0, None] * Hi[:, None, 0, :] + q.F[:, :, 1, None] * Hi[:, None, 1, :] + q.F[:, :, 2, None] * Hi[:, None, 2, :]
    sig = em["SIGMA"].reshape(-1, 12)
    ncw = em["NC_HOUSEHOLDER"].reshape(-1, 13)
    cw, cb = ncw[c, :12], ncw[c, 12]
    q.U = np.zeros((n, 3, 11))
    for a in range(3):
        v = np.zeros((n, 12))
        v[:, 4 * a:4 * a + 4] = sig[c][:, 4 * a:4 * a + 4] * X
        wv = RB._dot(cw[:, 4 * a:4 * a + 4], v[:, 4 * a:4 * a + 4])
        q.U[:, a] = v[:, 1:] - (cb[:, None] * cw[:, 1:]) * wv[:, None]
    ww = sw * sw
    m = np.stack([ww * D00 * D00, ww * D00 * D02, ww * D00 * D12, ww * (D02 * D02 + D12 * D12)], 1)
    q.h, q.em, q.sig, q.ncw = X, em, sig, ncw
    q.sw, q.D = sw, (D00, D02, D12)  # (what obs_cov's lane 0 reads again: cov_bounds.emulate_observations)
    q.hpp = _hpp_joint(OB._add_at(p.n_cams, c, m[:, :, None, None] * (X[:, :, None] * X[:, None, :])[:, None]))
    return q


def emulate_assembly(p, joint, order):
    """The augmented matrix [N, N + 1] (upper block triangle, the identity on the padding, -b in column N) and the
    [n_cams, dim, dim] B_c in fp64.  order 0: B_c first, then the landmarks ascending; order 1: the landmarks descending
    (and the pairs of a landmark from the last to the first: the transposed product), B_c last."""
    q = (_emu_pieces_joint if joint else _emu_pieces_pose)(p)
    dim = q.dim
    n = dim * p.n_cams
    N = padded(n)
    M = np.zeros((N, N + 1))
    Bc = q.em["_B"]

    def add_b():
        for c in range(p.n_cams):
            M[dim * c:dim * c + dim, dim * c:dim * c + dim] += Bc[c]
    if order == 0:
        add_b()
    W, Z = np.einsum("nap,nam->npm", q.U, q.G), np.einsum("nap,nam->npm", q.U, q.F)
    for l in (range(p.n_lms) if order == 0 else range(p.n_lms - 1, -1, -1)):
        a, b, rows, mask = _lm_index(p, l, dim)
        k = b - a
        Wl, Zl = W[a:b].reshape(k * dim, 3), Z[a:b].reshape(k * dim, 3)
        blk = -(Wl @ Zl.T) if order == 0 else -((Zl[:, ::-1] @ Wl[:, ::-1].T).T)
        M[np.ix_(rows, rows)] += blk * mask
    if order == 1:
        add_b()
    M[:n, N] = -q.em["B_JOINT" if joint else "B"]
    M[np.arange(n, N), np.arange(n, N)] = 1.0
    return M, Bc, q


def emulate_precond(p, joint, q):
    """(S_cc^-1 [n_cams, dim, dim], S_cc) through the sixty moments in fp64: cm_gram_sc's K_i (x) h h^T summed per camera in
    row order, cam_build_sc's subtraction, scaling, projection, lambda and Cholesky inverse."""
    n = len(p.cam_idx)
    K = np.einsum("nam,nbm->nab", q.G, q.F)
    hh = q.h[:, :, None] * q.h[:, None, :]
    dm = OB._add_at(p.n_cams, p.cam_idx, (K[:, :, None, :, None] * hh[:, None, :, None, :]).reshape(n, 12, 12))
    sig = q.sig
    A = (q.hpp - dm) * sig[:, :, None] * sig[:, None, :]
    if joint:
        A = OB._ntan(q.ncw[:, :12], q.ncw[:, 12], A)
    A[:, np.arange(q.dim), np.arange(q.dim)] += p.lam
    return OB.chol_inverse(A), A


def emulate_factor(M, mutate=None):
    """chol_factor + run_cholesky's back substitution on the augmented [N, N + 1] matrix in fp64: right-looking, panels of 64
    inside blocks of 256, the trailing updates as fp64 matrix products (any order).  Returns (the [N, N + 2] buffer of
    POVAR_BUF_SC_FACTOR, info).  mutate: defects of the factorisation (mutations())."""
    mutate = mutate or {}
    M = np.array(M, dtype=F)
    N = M.shape[0]
    if "pad_zero" in mutate:
        M[mutate["pad_zero"], mutate["pad_zero"]] = 0.0
    info = 0
    skip = mutate.get("subtile_skipped")  # (first row, first column) of a 16 x 16 tile of a trailing update
    with np.errstate(invalid="ignore", divide="ignore"):
        for K0 in range(0, N, CH_OB):
            kd = min(CH_OB, N - K0)
            R0 = K0 + kd
            for k0 in range(K0, R0, CH_NB):
                k1 = k0 + CH_NB
                A = M[k0:k1, k0:k1]
                for j in range(CH_NB):
                    piv = A[j, j]
                    if not piv > 0:
                        info |= 1
                    d = np.sqrt(piv)
                    row = A[j, :] / d
                    row[:j] = 0.0
                    row[j] = d
                    A[j, :] = row
                    A[j + 1:, j + 1:] -= np.outer(row[j + 1:], row[j + 1:])
                A[np.tril_indices(CH_NB, -1)] = 0.0
                B = M[k0:k1, k1:N + 1]
                for pp in range(CH_NB):
                    B[pp, :] = B[pp, :] / A[pp, pp]
                    B[pp + 1:, :] -= np.outer(A[pp, pp + 1:], B[pp, :])
                Pn = M[k0:k1, :]
                for i0 in range(k1, R0, CH_NB):
                    for j0 in range(i0, N + 1, CH_NB):
                        j1 = min(j0 + CH_NB, N + 1)
                        if j0 == N and mutate.get("rhs_skipped") == (k0, i0):
                            continue
                        upd = Pn[:, i0:i0 + CH_NB].T @ Pn[:, j0:j1]
                        if skip and i0 <= skip[0] < i0 + CH_NB and j0 <= skip[1] < j1 and skip[2] == k0:
                            upd[skip[0] - i0:skip[0] - i0 + 16, skip[1] - j0:skip[1] - j0 + 16] = 0.0
                        M[i0:i0 + CH_NB, j0:j1] -= upd
            if R0 < N:
                Pn = M[K0:R0, :]
                for i0 in range(R0, N, CH_T):
                    i1 = min(i0 + CH_T, N)
                    for j0 in range(i0, N + 1, CH_T):
                        j1 = min(j0 + CH_T, N + 1)
                        upd = Pn[:, i0:i1].T @ Pn[:, j0:j1]
                        if mutate.get("rhs_skipped") == (K0, i0) and j0 <= N < j1:
                            upd[:, N - j0] = 0.0
                        if skip and i0 <= skip[0] < i1 and j0 <= skip[1] < j1 and skip[2] == K0:
                            upd[skip[0] - i0:skip[0] - i0 + 16, skip[1] - j0:skip[1] - j0 + 16] = 0.0
                        M[i0:i1, j0:j1] -= upd
        x = M[:, N].copy()
        for k0 in range(N - CH_NB, -1, -CH_NB):
            A = M[k0:k0 + CH_NB, k0:k0 + CH_NB]
            for i in range(CH_NB - 1, -1, -1):
                x[k0 + i] = (x[k0 + i] - A[i, i + 1:] @ x[k0 + i + 1:k0 + CH_NB]) / A[i, i]
            if k0 > 0:
                upd = M[:k0, k0:k0 + CH_NB] @ x[k0:k0 + CH_NB]
                if mutate.get("back_row_skipped", (None, None))[0] == k0:
                    upd[mutate["back_row_skipped"][1]] = 0.0
                x[:k0] -= upd
    return np.concatenate([M[:, :N], M[:, N:N + 1], x[:, None]], 1), info


# ======== mutations: [(name, side, mutate dict, check, expected flat indices)]
def mutations(sy):
    """The defects a relative 2-norm over all cameras lets through.  side "reference": the dict goes to dense_system and the
    clean emulation must be reported against the mutated reference on exactly the entries named; side "factor": the dict
    goes to emulate_factor and the mutated factor must be reported against the clean reference.  check: "S" (entries of the
    upper triangle of the dense matrix, flat index i n + j), "precond" (cameras), "factor" / "forward" / "back" (flat indices
    of factor_check's arrays), "padding" (any message).  subtile_skipped leaves an indefinite trailing matrix at lambda = 1e-4
    (info = 1, as chol_diag would report): it is looked at on the system at lambda = 1, where the factorisation goes
    through."""
    p, dim, n, N = sy.p, sy.dim, sy.n, sy.N
    l2 = int(np.flatnonzero(p.n_l == 2)[0])
    a = int(p.lm_off[l2])
    ci, cj = int(p.cam_idx[a]), int(p.cam_idx[a + 1])
    blk = lambda r, c: {(dim * r + i) * n + dim * c + j for i in range(dim) for j in range(dim)}
    up = lambda s: {e for e in s if e // n <= e % n}
    out = [("pair_dropped", "reference", {"pair_dropped": (l2, 0, 1)}, "S", blk(ci, cj)),
           ("pair_transposed", "reference", {"pair_transposed": (l2, 0, 1)}, "S", None)]
    # sigma of the wrong camera on one row of one observation: row r of the blocks (c_o, c_j >= c_o), column r of (c_i < c_o, c_o)
    lk = int(np.flatnonzero(p.n_l >= 3)[0])
    o = int(p.lm_off[lk]) + 1
    co = int(p.cam_idx[o])
    r = 5
    exp = set()
    for t in range(int(p.lm_off[lk]), int(p.lm_off[lk + 1])):
        ct = int(p.cam_idx[t])
        if t >= o:
            exp |= {(dim * co + r) * n + dim * ct + j for j in range(dim)}
        if t <= o:
            exp |= {(dim * ct + i) * n + dim * co + r for i in range(dim)}
    other = int(np.flatnonzero((p.n_c > 0) & (np.arange(p.n_cams) != co))[0])
    out.append(("sigma_wrong_camera", "reference", {"sigma_row": (o, r, other)}, "S", None if sy.joint else up(exp)))
    if sy.joint:
        lm_blocks = set()
        for t in range(a, a + 2):
            for v in range(t, a + 2):
                lm_blocks |= blk(int(p.cam_idx[t]), int(p.cam_idx[v]))
        out.append(("hll_undamped", "reference", {"hll_undamped": l2}, "S", up(lm_blocks)))
    few = int(np.flatnonzero(p.n_c > 0)[np.argmin(p.n_c[p.n_c > 0])])
    out.append(("moment_last_summand", "reference", {"moment_last": (few, 1, 5)}, "precond", {few}))
    # the factorisation
    k_first = CH_NB if N > CH_NB else None
    if N > CH_NB:
        if N > CH_OB:  # the rhs column left out of the outer update's first row tile
            i1 = min(CH_OB + CH_T, N, n)
            out.append(("rhs_skipped", "factor", {"rhs_skipped": (0, CH_OB)}, "forward", set(range(CH_OB, i1))))
            if n >= CH_OB + 48:
                out.append(("subtile_skipped", "factor", {"subtile_skipped": (CH_OB + 16, CH_OB + 32, 0)}, "factor",
                            {i * n + j for i in range(CH_OB + 16, CH_OB + 32) for j in range(CH_OB + 32, CH_OB + 48)}))
        else:
            i1 = min(2 * CH_NB, n)
            out.append(("rhs_skipped", "factor", {"rhs_skipped": (0, CH_NB)}, "forward", set(range(CH_NB, i1))))
            if n >= CH_NB + 48:
                out.append(("subtile_skipped", "factor", {"subtile_skipped": (CH_NB + 16, CH_NB + 32, 0)}, "factor",
                            {i * n + j for i in range(CH_NB + 16, CH_NB + 32) for j in range(CH_NB + 32, CH_NB + 48)}))
    if k_first:
        # (row 63 and row 64 belong to one camera in both steps: the skipped product is not zero)
        out.append(("back_row_skipped", "factor", {"back_row_skipped": (CH_NB, CH_NB - 1)}, "back", {CH_NB - 1}))
    if N > n:
        out.append(("pad_zero", "factor", {"pad_zero": N - 1}, "padding", None))
    return out


# ======== the shapes of tests/test_sc_bounds.py and tests/test_gpu_sc_bounds.py
ALPHA, LAM = 0.01, 1e-4
HUBER1, HUBER2 = 30.0, 0.5  # the thresholds of tests/test_gpu_sc_solvers.py


def pose_case(s, robust="NONE", lam=LAM):
    """A synth problem as CHOLESKY's tests set it: landmarks from init_landmarks_pose, no Jl column scaling."""
    from oracle import povar_oracle as O
    lms = O.Oracle(s.n_cams, s.lm_off, s.cam_idx, s.obs).init_landmarks_pose(ALPHA, s.cams)
    return OB.Pose(s.n_cams, s.lm_off, s.cam_idx, s.obs, s.cams, lms, ALPHA, lam, robust, HUBER1, scale_jl=False)


def joint_case(s, robust="NONE", lam=LAM, seed=11):
    """The step-2 state of tests/test_gpu_sc_solvers.py::_state2 on a synth problem's graph."""
    rng = np.random.default_rng(seed)
    cams = rng.normal(size=(s.n_cams, 12))
    cams[:, 8:11] *= 0.1
    cams[:, 11] = 5 + rng.random(s.n_cams)
    cams /= np.linalg.norm(cams, axis=1, keepdims=True)
    lms_h = np.concatenate([rng.normal(size=(s.n_lms, 3)), np.ones((s.n_lms, 1))], 1)
    return OB.Joint(s.n_cams, s.lm_off, s.cam_idx, s.obs / 500.0, cams, lms_h, lam, robust, HUBER2)


def edge_graph():
    """The graph of test_edge_cases_long_landmarks_and_unobserved_cameras (landmarks of 140, 97, 65 and 64 observations,
    120 two-view landmarks, cameras 3, 77 and 149 unobserved) plus one landmark of 33 observations at the end: both staging
    chunk sizes (64 in sc_dense_offdiag, 32 in sc_dense_offdiag_h) are exceeded by one."""
    rng = np.random.default_rng(17)
    n_c = 150
    used = np.setdiff1d(np.arange(n_c), [3, 77, 149])
    degs = [140, 97, 65, 64] + [2] * 120 + list(rng.integers(3, 9, size=150)) + [33]
    cam_idx = np.concatenate([np.sort(rng.choice(used, k, replace=False)) for k in degs]).astype(np.int32)
    lm_off = np.concatenate([[0], np.cumsum(degs)]).astype(np.int32)
    return n_c, degs, cam_idx, lm_off, rng


def edge_pose(robust="NONE", lam=LAM):
    from oracle import povar_oracle as O
    n_c, degs, cam_idx, lm_off, rng = edge_graph()
    n_l = len(degs)
    cams = np.zeros((n_c, 12))
    cams[:, :8] = rng.normal(size=(n_c, 8))
    cams[:, 11] = 1.0
    X = rng.normal(size=(n_l, 3))
    P = cams[cam_idx].reshape(-1, 3, 4)
    proj = np.einsum("nij,nj->ni", P[:, :2, :3], X[np.repeat(np.arange(n_l), degs)]) + P[:, :2, 3]
    obs = proj + rng.normal(scale=0.05, size=proj.shape)
    lms = O.Oracle(n_c, lm_off, cam_idx, obs).init_landmarks_pose(ALPHA, cams)
    return OB.Pose(n_c, lm_off, cam_idx, obs, cams, lms, ALPHA, lam, robust, 0.1, scale_jl=False)


def edge_joint(robust="NONE", lam=LAM):
    n_c, degs, cam_idx, lm_off, rng0 = edge_graph()
    n_l = len(degs)
    rng = np.random.default_rng(11)
    cams = rng.normal(size=(n_c, 12))
    cams[:, 8:11] *= 0.1
    cams[:, 11] = 5 + rng.random(n_c)
    cams /= np.linalg.norm(cams, axis=1, keepdims=True)
    lms_h = np.concatenate([rng.normal(size=(n_l, 3)), np.ones((n_l, 1))], 1)
    pc = np.einsum("nij,nj->ni", cams[cam_idx].reshape(-1, 3, 4), lms_h[np.repeat(np.arange(n_l), degs)])
    obs = pc[:, :2] / pc[:, 2:3] + rng.normal(scale=0.05, size=(len(cam_idx), 2))
    return OB.Joint(n_c, lm_off, cam_idx, obs, cams, lms_h, lam, robust, 0.05)
