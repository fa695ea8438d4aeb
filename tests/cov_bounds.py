"""Componentwise, condition-free bounds for the covariance path (povar_cov.hip: cov_inverse, cov_camera_blocks,
landmark_covariance, observation_covariance; povar_kernels_cov.hpp), stage by stage on the device's own intermediates (helper module of
tests/test_cov_bounds.py and tests/test_gpu_cov_bounds.py; not a test module).  The last stage of the path, the covariance
blocks of parameter pairs (covariance_blocks: pair_cc, pair_cl, pair_ll), is held in the same way on the same C and Q by
tests/pair_bounds.py (tests/test_pair_bounds.py, tests/test_gpu_pair_bounds.py).  Conventions of sc_bounds.py: LD, g(k) rounded
up, first order, a final factor 1 + 1e-6, `worst` / `flagged` for reporting.  The device's buffers: R = POVAR_BUF_COV_FACTOR
(upper triangle), W = the upper triangle of POVAR_BUF_COV_INVERSE, C = its strictly lower 64 x 64 blocks and POVAR_BUF_COV_PANEL
read as cov_at does (povar_kernels_cov.hpp:280-284), Q = POVAR_BUF_COV_GAUGE.  Products of device matrices are formed
without rounding (sc_bounds.exact_gram for W W^T and R^T R, exact_matmul below for W R and Q^T Q: the same slicing); what the
slicing leaves out is added to every bound.  An MFMA accumulation counts as "K products in any order": g(K).  Line numbers
are those of povar_kernels_cov.hpp unless a file is named.

ASSEMBLY  chol_factor (povar_sc.hip) with Q: the FACTOR identity of sc_bounds.py on the kept R,
              |S_ref(lambda) + Q_dev Q_dev^T - R^T R|_ij <= g(k_f(i)) (|R^T| |R|)_ij + E(S)_ij + E(QQ)_ij       (i <= j < n)
          with S_ref, E(S) from sc_bounds.dense_system at the call's lambda (0 in the free gauge) and, for cov_add_qqt (:29-41),
          the nq-term dot `s += qi[k] * qj[k]` (:38: g(nq)) and `M += s` (:39): one more summand of the entry's atomic sum, i.e.
          g(cnt + shards + 1) on |Q| |Q|^T and one more rounding u on the other summands:
              E(QQ) = (g(nq) + g(cnt + shards + 1)) |Q| |Q|^T + u Sm.
          Damped calls have no Q term.  cov_add_qqt runs on rank 0 only (povar_sc.hip: chol_factor): with two shards the term enters
          once.  Rows and columns [n, N) of R are the identity's, bit for bit (chol_pad).
GAUGE     gauge_basis (cov_plan.hpp): twice-applied modified Gram-Schmidt.  Diagonal: the n-term dot of positive terms
          (g(n)), the root (1) squared (2), every division (1) squared (2):  |q_k . q_k - 1| <= g(n + 4).  Off the diagonal, j < k:
          in the second pass t = q_j . v carries g(n) |q_j| . |v|; the update of step j and of every later step of that pass
          rounds v twice per entry (product, difference): 2 (k - j) u |q_j| . |v|; the later steps' own corrections t' q_j'
          move q_j . v by t' (q_j . q_j'), a product of two quantities of the order u kappa(V): second order, dropped as
          everywhere here (the call itself refuses a column that loses more than 1e-8 of its norm, cov_plan.hpp: gauge_basis); the
          norm and the division (n + 4 halves, 1):  |q_j . q_k| <= g(n + 2 nq + 4) |q_j| . |q_k|.  Columns on disjoint supports
          (step 1: generators of different gj) are orthogonal exactly: the bound is 0 there.
          Span (gauge_span): every long-double generator v built from the caller's cameras and the reference's sigma and
          reflectors is reproduced by Q Q^T:  |v - Q (Q^T v)|_2 <= (kappa_2(V_ref) (g(n + 2 nq + 4) nq + 2 E_rel(V)) + g(2 nq) nq) |v|_2
          with kappa_2(V_ref) the condition number of the 12- or 15-column generator matrix -- a reference quantity computed
          from the reference, not the system's -- and E_rel(V) the largest relative operand error of a generator entry
          (E(sigma) / sigma; step 2: + the reflector's dNc and the g(40) of the a / N_c^T arithmetic).
INVERSE   cov_inverse's loop (povar_cov.hip: cov_inverse).  Diagonal block (cov_diag_inv :64-84): lane c forms row c from W R = I
          left to right, `s += w[p] * R[p][j]` over p < j (:75; the terms p < c are exact zeros) and `-s / d` (:77): a product
          passes its own rounding and at most j - c - 1 additions, the division rounds once:
              |W_jj R_jj - I|_cj <= g(max(j - c, 1)) (|W_jj| |R_jj|)_cj =: D0_cj  (j >= c; below: W = 0 and the residual is 0).
          Block column j, block row i < j (cov_trmm :97-154): T^ = fl(R_0j W_jj) with k_first = 0, k_end = 1 (:123-125,
          the loop's first cov_trmm): 64 products, alpha = 1 exact; W^_ij = -fl(sum_{kb = i .. j-1} W_i,kb T^_kb) with k_first = i, k_end = j
          (its second cov_trmm): 64 (j - i) products, alpha = -1 exact.  Left residual of the block:
              |(W R)_ij| <= A_i D0_j + (g(64) + g(64 (j - i))) (|W_lead| (|R_0j| |W_jj|))_i |R_jj|,  A_i = (|W_lead| |R_0j|)_i
          (|T^| <= (1 + g(64)) |R_0j| |W_jj|: first order).  Everything from the device's own R and W: no condition number.
          Exact: the strictly lower part of every diagonal block of W is zero (cov_diag_inv stores its zeros, :77-83: the
          remark on cov_gram that leftovers of the assembly sit below the diagonal holds for the strictly lower 64 x 64 BLOCKS
          only, which a camera block that straddles a 64-edge reaches); padding rows / columns are the identity's; +-0 is 0.
GRAM      cov_gram (:164-192): thread t sums `acc += v[a] * v[b]` (:180) over its ceil((n - DIM c - t) / 256) <= trips_c =
          ceil((n - DIM c) / 256) columns, entries left of the diagonal masked to 0 (:175) as W has them; block_sum
          (povar_kernels.hpp:428-443): six additions of the wavefront stage and three of the four partial sums: 9:
              |T_c - (W W^T)_cc| <= g(trips_c + 9) (|W| |W|^T)_cc.
FINISH    cov_finish (:202-248), solver coordinates: `s += qa[k] * qb[k]` (:214: g(nq)) and `o - s` (:215: one more on both):
              |out_c - ((W W^T)_cc - Q_J Q_J^T)| <= g(trips_c + 10) (|W| |W|^T)_cc + g(nq + 1) |Q_J| |Q_J|^T   (nq = 0: g(trips_c + 9)).
          Camera coordinates: DIM = 12: `sg[i] * v * sg[j]` (:245): two roundings and the two sigma operands; DIM = 11: N_c's
          entries `delta - beta w w` (:223: 3), the two eleven-term dots (:238-242: 11 + 11), then :245:
              E = D |N| E(T) |N|^T D + (g(2) | g(30) + 2 dNc) D |N| |T| |N|^T D + (E(sigma_i) / sigma_i + E(sigma_j) / sigma_j) |.|
          with the reference's sigma, reflectors and their operand bounds (operand_bounds: Esig, dnc).  Every block is
          symmetric bit for bit.
LAUUM     cov_lauum (:261-328): block (I, J), I >= J: `for kb = I .. nb - 1` (:299), 64 products a step, stored as it is (:327):
              |C_dev - W W^T|_rc <= g(64 (nb - I)) (|W| |W|^T)_rc,   I = r div 64,
          on every entry of the strictly lower blocks (POVAR_BUF_COV_INVERSE) and of the full diagonal blocks (the panel).
LANDMARK  lm_cov (:372-539) with C_dev through cov_at, Q_dev and the staged operands of sc_bounds.pieces_pose / pieces_joint
          (W_i = U_i^T G_i = E_i Hll^-1, dim x 3, magnitudes Wm, operand errors EW; Hll^-1 with EHi), solver coordinates:
              Sigma_l = Hll^-1 + sum_ij W_i^T C[c_i, c_j] W_j - T_l^T T_l,     T_l = sum_i Q[c_i]^T W_i  (nq x 3).
          K (:447-462): per lane ceil(DIM^2 / 16) terms `K += u * cv * v` (2 products, the additions) and the four shuffle
          additions: k_K = ceil(DIM^2 / 16) + 6; K G_j (:470) and G_i^T (.) (:474): 3 + 3; P + P^T (:479): 1; `acc +=` (:479): at
          most trips_l = sum over the chunk pairs of ceil(ni nj / 16) (:439) additions; block_sum: 9; `Hi + acc - tt` (:502): 2:
              E(pairs) = sum_ij (EW_i^T |C_ij| Wm_j + Wm_i^T |C_ij| EW_j) + g(k_K + 7 + trips_l + 11) sum_ij Wm_i^T |C_ij| Wm_j.
          T_l (:421-437, :496-501): `ta += qv * u` over DIM rows (DIM), the three-term product with G (3), `tacc +=` over
          tt_l = sum over the chunks of ceil(ni / 4) observations, the four-way sum (3): k_t = DIM + 6 + tt_l per factor;
          `tt += tx * ty` (nq) and the subtraction (1):
              E(T) = ET^T Tm + Tm^T ET + g(2 k_t + nq + 1) Tm^T Tm,   Tm = sum_i |Q[c_i]|^T Wm_i,  ET = sum_i |Q[c_i]|^T EW_i.
          Hll^-1 passes the two additions of :502:  E(Hi) + 2 u |Hi|.  The three magnitudes stay apart, so the cancellation
          of the free gauge is charged.  Landmark coordinates: DIM = 12 (:517): two roundings and the two s operands; DIM = 11
          (:522-534): first N_l Sigma N_l^T with the long-double house4 of the caller's X_l, its entries to g(25) (operand_bounds:
          dn) on |N_l|, the two three-term products (3 + 3), then the same scaling with the four s of the landmark.
          Given C this is condition-free.  Every block is symmetric bit for bit.
OBSERVATION  obs_cov (:559-715) with C_dev through cov_at, the staged U_i, G_j of pieces_pose / pieces_joint (U, Um, EU; G, Gm, EG)
          and Sigma_l = lm_cov's output with nq = 0 in solver coordinates: its long-double value from the same C and its bound
          E(Sigma_l) are LANDMARK's (landmark_reference with Q = None).  Row of observation i of landmark l (k observations):
              Syy_i = K_ii - R_i L_i^T - L_i R_i^T + L_i Sigma_l L_i^T,  K_ij = U_i C[c_i, c_j] U_j^T,  R_i = sum_j K_ij G_j,
              h_i = sum_e (M_i)_e (Syy_i)_e,    [[c_uu, c_uv], [c_uv, c_vv]] = J Syy_i J^T,  J = [[iz, 0, j0], [0, iz, j1]].
          K_ij (:619-630): lane gl sums its t_K = ceil(DIM^2 / 16) terms `K += u * cv * v`: two products and t_K additions, and for
          DIM = 12 the products sigma h of lm_cov_u (:362) on either side (2): k_K = t_K + 2 (+ 2).  R_i (:634): the three-term dot
          with G_j (3), `R +=` once per observation of the track, in every chunk (k), the four butterfly additions (:642-647: 4);
          K_ii is copied (:635-638) and passes the butterfly only:
              E(K_ii) = EU_i |C_ii| Um_i^T + Um_i |C_ii| EU_i^T + g(k_K + 4) Um_i |C_ii| Um_i^T,
              E(R_i)  = sum_j ((EU_i |C_ij| Um_j^T + Um_i |C_ij| EU_j^T) Gm_j + Km_ij EG_j) + g(k_K + 7 + k) sum_j Km_ij Gm_j,
          Km_ij = Um_i |C_ij| Um_j^T.  Lane 0's operands (:649-683), from the caller's cameras, points and image points and the
          reference chain of operand_bounds, as sc_bounds' pieces take theirs:
            y    four-term dots (:660): E(y) = g(4) |P| |h|.
            L_i  DIM = 12 (:663): P3 diag(s): one product and E(s) / s.  DIM = 11 (:665-668): q4 = p4 s4 (1 and E(s) / s), the
                 four-term `aw` (4), two products and the difference (3), house4 of the device against the long-double one to
                 g(25) (operand_bounds: dn) on |N_l|^T |q4|:  EL = |N_l|^T (|q4| (u + E(s) / s)) + (g(8) + g(25)) |N_l|^T |q4|.
            M_i  DIM = 12 (:672-676): sb sb (g(4) + 1, operand_bounds: dsb), cuv = sb2 (u u + v v) (+ 3: the longest entry), w = sw sw
                 (1 and 2 rho), the product (1): EM = (g(10) + 2 rho) |M|.  DIM = 11 (:678-682): hom_project's D00, D02, D12 with the
                 chain's magnitudes A and errors E (as pieces_joint), D02 D02 + D12 D12 (3), w = sw sw (1, 2 rho), the product (1):
                 EM = w E(m9) + (g(5) + 2 rho) Mm,  E(m9) by the product rule on A, E.
            J    iz = 1 / y2 (:704): r_z = E(y2) / |y2| + u;  j = -y iz iz (:705): E(j) = |j| (2 r_z + 2 u) + E(y) iz^2.
          The final expression (:689-697): `SL` and `lsl` three-term dots (3 + 3), `rl`, `lr` (3 each), the three additions of `v`:
              E(Syy) = E(K_ii) + (E(R) |L|^T + |R| EL^T + g(3) |R| |L|^T) + (.)^T
                       + EL |Sigma| |L|^T + |L| |Sigma| EL^T + |L| E(Sigma) |L|^T + g(6) |L| |Sigma| |L|^T + g(3) Smag,
              Smag   = |K_ii| + |R| |L|^T + |L| |R|^T + |L| |Sigma| |L|^T:
          the four magnitudes stay apart, so what cancels between them in the free gauge is charged.  With Sa = |Syy| + E(Syy):
              E(h)   = sum_e (Mm E(Syy) + EM Sa)_e + g(9) sum_e (Mm Sa)_e                                  (:703: nine terms)
              E(A)   = |J| E(Syy) + EJ Sa + g(2) |J| Sa,    A = J Syy                                          (:706-707)
              E(c)   = E(A) |J|^T + (|J| Sa) EJ^T + g(2) |J| Sa |J|^T                                          (:710-712).
          Given C this is condition-free: the inputs are the caller's data, the chain's operand bounds and the device's C.
          Exact: every entry is finite; a landmark requested twice returns the same bits.  Step 2's h and w (c_uu + c_vv) are
          different expressions (M_i has D02^2 + D12^2 in one entry; c_* goes through J twice): nothing is asserted between them.

Emulations (fp64 NumPy, the kernels' operation order, two summation orders) and the mutation list: at the end.
"""
import numpy as np

import operand_bounds as OB
import sc_bounds as SB
from operand_bounds import F, LD, _ab, _f, g
from rounding_bounds import U64, ULD
from sc_bounds import CH_NB, ONE, flagged, padded, worst  # noqa: F401  (worst / flagged: re-exported for the tests)

NB = CH_NB


def exact_matmul(A, B):
    """(A B in long double, an entrywise bound on what is missing from it): sc_bounds.exact_gram's slicing with the rows of A
    and the columns of B cut into four slices of 19 bits below their largest exponent; inner dimension <= 2048."""
    A, B = np.asarray(A, dtype=F), np.asarray(B, dtype=F)
    assert A.shape[1] == B.shape[0] <= 2048 and np.all(np.isfinite(A)) and np.all(np.isfinite(B))

    def slices(X, axis):
        m = np.abs(X).max(axis, keepdims=True)
        e = np.where(m > 0, np.ceil(np.log2(np.where(m > 0, m, 1.0))) + 1, 0.0)
        rem, sl = X.copy(), []
        for s in range(4):
            unit = np.exp2(e - 19 * (s + 1))
            t = np.rint(rem / unit) * unit
            sl.append(t)
            rem = rem - t
        return sl, np.abs(rem)
    sa, ra = slices(A, 1)
    sb, rb = slices(B, 0)
    out = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for a in sa:
        for b in sb:
            out += (a @ b).astype(LD)
    Aa, Ba = np.abs(A), np.abs(B)
    return out, (Aa @ rb + ra @ Ba + ra @ rb + 16 * ULD * (Aa @ Ba)) * ONE


# ======== the layout
def upper(inv):
    """W: the upper triangle of POVAR_BUF_COV_INVERSE."""
    return np.triu(np.asarray(inv, dtype=F))


def c_lower(inv, panel):
    """C as cov_lauum leaves it, [N, N]: the strictly lower 64 x 64 blocks from `inv`, the full diagonal blocks from the panel,
    zeros above."""
    inv, panel = np.asarray(inv, dtype=F), np.asarray(panel, dtype=F)
    N = inv.shape[0]
    C = np.zeros((N, N))
    for I in range(N // NB):
        r = slice(NB * I, NB * I + NB)
        C[r, :NB * I] = inv[r, :NB * I]
        C[r, r] = panel[r, :]
    return C


def cov_at(inv, panel, r, c):
    """Entry (r, c) of C as the device's cov_at reads it (:280-284); r, c: integer arrays."""
    r, c = np.maximum(r, c), np.minimum(r, c)
    same = (r >> 6) == (c >> 6)
    return np.where(same, np.asarray(panel)[r, c & 63], np.asarray(inv)[r, c])


def c_symmetric(inv, panel):
    """The symmetric [N, N] matrix every cov_at read comes from."""
    N = np.asarray(inv).shape[0]
    i = np.arange(N)
    return cov_at(inv, panel, i[:, None], i[None, :])


def _identity_padding(M, n, what, pad):
    N = M.shape[0]
    for i in range(n, N):
        if M[i, i] != 1.0 or np.any(M[i, i + 1:] != 0.0) or np.any(M[:i, i] != 0.0):
            pad.append(f"padding row / column {i} of {what} is not the identity's")


# ======== ASSEMBLY
def assembly_check(sy, Rk, Q=None):
    """{'assembly': (err, bound) [n, n] on the upper triangle, 'exact': messages}; sy: sc_bounds.dense_system at the call's
    lambda (its `shards`), Rk: POVAR_BUF_COV_FACTOR, Q: POVAR_BUF_COV_GAUGE or None (damped)."""
    n, N, u = sy.n, sy.N, sy.u
    R = np.triu(np.asarray(Rk, dtype=F))
    assert R.shape == (N, N)
    pad = []
    if not np.all(np.isfinite(R)):
        pad.append("non-finite entries in R")
        R = np.nan_to_num(R)
    RtR, miss = SB.exact_gram(R)
    Ra = np.abs(R)
    A = Ra.T @ Ra
    gf = np.broadcast_to(g(SB.k_factor(N), u)[:, None], (N, N))[:n, :n]
    ref, bound = sy.S, gf * A[:n, :n] + sy.ES + miss[:n, :n]
    if Q is not None:
        Q = np.asarray(Q, dtype=F)
        nq = Q.shape[1]
        QQ, mq = exact_matmul(Q, Q.T)
        QQm = np.abs(Q) @ np.abs(Q).T
        ref = ref + QQ
        bound = bound + (g(nq, u) + g(sy.cnt + sy.shards + 1, u)) * QQm + u * sy.Sm + mq
    up = np.triu(np.ones((n, n), dtype=bool))
    _identity_padding(R, n, "R", pad)
    return {"assembly": (np.where(up, _ab(ref - RtR[:n, :n]), 0.0), np.where(up, bound * ONE, 0.0)), "exact": pad}


# ======== GAUGE
def gauge_check(Q):
    """(|Q^T Q - I|, its bound), [nq, nq]."""
    Q = np.asarray(Q, dtype=F)
    n, nq = Q.shape
    QtQ, miss = exact_matmul(Q.T, Q)
    Qa = np.abs(Q)
    M = Qa.T @ Qa
    k = np.where(np.eye(nq, dtype=bool), n + 4, n + 2 * nq + 4)
    return _ab(QtQ - np.eye(nq, dtype=LD)), (g(k) * M + miss) * ONE


def gauge_generators(sy):
    """(V [n, nq] long double: the generators of gauge_basis from the caller's cameras and the reference's sigma and reflectors,
    E_rel: the bound on a generator entry's relative operand error on the device)."""
    ch, p = sy.R.aux["chain"], sy.p
    sig, rs = ch["sig"], float((ch["Esig"] / _f(ch["sig"])).max())
    P = p.cams.astype(LD)
    nq = 12 if sy.dim == 12 else 15
    cols = []
    for col in range(nq):
        gi, gj = divmod(col, 4)
        G = np.zeros_like(P)
        for r in range(3):
            G[:, 4 * r + gj] = -P[:, 4 * r + gi]
        if sy.dim == 12:
            cols.append((G / sig).reshape(-1))
            continue
        cw, cb = ch["cw"], ch["cb"]
        h0 = -cb[:, None] * cw * cw[:, :1]
        h0[:, 0] += 1
        a = -((h0 * (G / sig)).sum(1)) / ((h0 * (P / sig)).sum(1))
        cols.append(OB._nt12(cw, cb, (G + a[:, None] * P) / sig).reshape(-1))
    V = np.stack(cols, 1)
    return V, (rs if sy.dim == 12 else 3 * rs + 2 * sy.R.aux["dnc"] + g(40))


def gauge_span(sy, Q):
    """(|v - Q Q^T v|_2 per generator, its bound) -- module docstring: GAUGE."""
    V, erel = gauge_generators(sy)
    Ql = np.asarray(Q, dtype=F).astype(LD)
    n, nq = Ql.shape
    res = V - Ql @ (Ql.T @ V)
    sv = np.linalg.svd(V.astype(F), compute_uv=False)
    kappa = float(sv[0] / sv[-1])
    norm = np.sqrt((V * V).sum(0)).astype(F)
    bound = (kappa * (g(n + 2 * nq + 4) * nq + 2 * erel) + g(2 * nq) * nq) * norm * ONE
    return np.sqrt((res * res).sum(0)).astype(F), bound, kappa


# ======== INVERSE
def _d0_gamma():
    c, j = np.arange(NB)[:, None], np.arange(NB)[None, :]
    return np.where(j >= c, g(np.maximum(j - c, 1)), 0.0)


def inverse_check(Rk, inv, n):
    """{'inverse': (|W R - I|, bound) [N, N], 'exact': messages} from POVAR_BUF_COV_FACTOR and POVAR_BUF_COV_INVERSE."""
    R, Wf = np.triu(np.asarray(Rk, dtype=F)), np.asarray(inv, dtype=F)
    N = R.shape[0]
    nb = N // NB
    bad = []
    for I in range(nb):
        blk = Wf[NB * I:NB * I + NB, NB * I:NB * I + NB]
        if np.any(np.tril(blk, -1) != 0.0):
            bad.append(f"diagonal block {I} of W is not zero below its diagonal")
    W = np.triu(Wf)
    if not (np.all(np.isfinite(W)) and np.all(np.isfinite(R))):
        bad.append("non-finite entries in R or W")
        W, R = np.nan_to_num(W), np.nan_to_num(R)
    _identity_padding(W, n, "W", bad)
    P, miss = exact_matmul(W, R)
    err = _ab(P - np.eye(N, dtype=LD))
    Wa, Ra = np.abs(W), np.abs(R)
    bound = np.zeros((N, N))
    gd = _d0_gamma()
    for j in range(nb):
        cj = slice(NB * j, NB * j + NB)
        D0 = gd * (Wa[cj, cj] @ Ra[cj, cj])
        bound[cj, cj] = D0
        if j == 0:
            continue
        lead = slice(0, NB * j)
        A = Wa[lead, lead] @ Ra[lead, cj]
        X = (Wa[lead, lead] @ (Ra[lead, cj] @ Wa[cj, cj])) @ Ra[cj, cj]
        gi = g(NB) + g(NB * (j - np.arange(NB * j) // NB))
        bound[lead, cj] = A @ D0 + gi[:, None] * X
    return {"inverse": (err, (bound + miss) * ONE), "exact": bad}


# ======== GRAM / FINISH
def _trips(n, dim, n_cams):
    return -(-(n - dim * np.arange(n_cams)) // 256)


def _camera_maps(sy):
    """Per camera: (L [n_cams, 12, dim] long double with block -> L block L^T, |L| magnitudes, relative error of the map)."""
    ch, u = sy.R.aux["chain"], sy.u
    sig, rs = ch["sig"], ch["Esig"] / _f(ch["sig"])
    if sy.dim == 12:
        eye = np.eye(12, dtype=LD)[None]
        return sig[:, :, None] * eye, _f(sig)[:, :, None] * np.eye(12)[None], rs, g(2, u)
    cw, cb = ch["cw"], ch["cb"]
    Nc = (np.eye(12, dtype=LD)[None] - cb[:, None, None] * cw[:, :, None] * cw[:, None, :])[:, :, 1:]
    Nm = (np.eye(12)[None] + _f(cb)[:, None, None] * _ab(cw)[:, :, None] * _ab(cw)[:, None, :])[:, :, 1:]
    return sig[:, :, None] * Nc, _f(sig)[:, :, None] * Nm, rs, g(30, u) + 2 * sy.R.aux["dnc"]


def camera_check(inv, Q, blocks, n, dim, coords=1, sy=None):
    """{'camera': (err, bound) [n_cams, d, d], 'exact': messages}: the camera blocks of a call against (W W^T)_cc - Q_J Q_J^T
    from the same call's W and Q (Q None: damped); coords = 0 needs sy (the reference's sigma and reflectors)."""
    W = upper(inv)
    n_cams = n // dim
    WWt, miss = SB.exact_gram(W.T)
    Wa = np.abs(W)
    A = Wa @ Wa.T
    nq = 0 if Q is None else np.asarray(Q).shape[1]
    kc = _trips(n, dim, n_cams) + 9 + (1 if nq else 0)
    T = SB.diag_blocks(WWt[:n, :n], dim)
    Tm = SB.diag_blocks(A[:n, :n], dim)
    ET = g(kc)[:, None, None] * Tm + SB.diag_blocks(miss[:n, :n], dim)
    if nq:
        Ql, Qa = np.asarray(Q, dtype=F).astype(LD).reshape(n_cams, dim, nq), np.abs(np.asarray(Q, dtype=F)).reshape(n_cams, dim, nq)
        QQm = np.einsum("cak,cbk->cab", Qa, Qa)
        T = T - np.einsum("cak,cbk->cab", Ql, Ql)
        Tm = Tm + QQm
        ET = ET + (g(nq + 1) + (nq + 1) * ULD) * QQm
    blocks = np.asarray(blocks, dtype=F)
    bad = [] if np.array_equal(blocks, blocks.transpose(0, 2, 1)) else ["a camera block is not symmetric bit for bit"]
    if coords == 0:
        L, Lm, rs, gmap = _camera_maps(sy)
        T = L @ T @ L.transpose(0, 2, 1)
        mag = Lm @ Tm @ Lm.transpose(0, 2, 1)
        ET = Lm @ ET @ Lm.transpose(0, 2, 1) + (gmap + rs[:, :, None] + rs[:, None, :] + 300 * ULD) * mag
    return {"camera": (_ab(blocks.astype(LD) - T), ET * ONE), "exact": bad}


# ======== LAUUM
def lauum_check(inv, panel):
    """{'lauum': (err, bound) [N, N] on the strictly lower 64 x 64 blocks and the full diagonal blocks}."""
    W = upper(inv)
    N = W.shape[0]
    C = c_lower(inv, panel)
    WWt, miss = SB.exact_gram(W.T)
    Wa = np.abs(W)
    blk = np.arange(N) // NB
    low = blk[:, None] >= blk[None, :]
    gk = g(NB * (N // NB - blk))[:, None]
    err = np.where(low, _ab(C.astype(LD) - WWt), 0.0)
    if not np.all(np.isfinite(C)):
        err = np.where(np.isfinite(err), err, np.inf)
    return {"lauum": (err, np.where(low, (gk * (Wa @ Wa.T) + miss) * ONE, 0.0))}


# ======== LANDMARK
def _chunk_trips(k, chunk):
    sizes = [min(chunk, k - a) for a in range(0, k, chunk)]
    pairs = sum(-(-sizes[i] * sizes[j] // 16) for i in range(len(sizes)) for j in range(i, len(sizes)))
    return pairs, sum(-(-s // 4) for s in sizes)


def landmark_reference(sy, Cs, Q, ids=None, mutate=None):
    """(Sigma_l [len(ids), 3, 3] long double in solver coordinates, its bound) -- module docstring: LANDMARK.  Cs: the
    symmetric [N, N] C of cov_at's reads (c_symmetric); Q: the device's gauge basis or None."""
    p, q, dim, u = sy.p, sy.q, sy.dim, sy.u
    ch = sy.R.aux["chain"]
    ids = np.arange(p.n_lms) if ids is None else np.asarray(ids)
    chunk = 64 if dim == 12 else 32  # SCD_CHUNK / SCDH_CHUNK (povar_kernels_sc.hpp)
    kK = -(-dim * dim // 16) + 6
    Cl, Ca = np.asarray(Cs, dtype=F).astype(LD), np.abs(np.asarray(Cs, dtype=F))
    nq = 0 if Q is None else np.asarray(Q).shape[1]
    if nq:
        Ql, Qa = np.asarray(Q, dtype=F).astype(LD), np.abs(np.asarray(Q, dtype=F))
    out, bound = np.zeros((len(ids), 3, 3), dtype=LD), np.zeros((len(ids), 3, 3))
    for t, l in enumerate(ids):
        a, b, rows, _ = SB._lm_index(p, int(l), dim)
        k = b - a
        Wl, Wm, EW = q.W[a:b].reshape(k * dim, 3), q.Wm[a:b].reshape(k * dim, 3), q.EW[a:b].reshape(k * dim, 3)
        ix = np.ix_(rows, rows)
        Hi, EHi = ch["Hi"][l], ch["EHi"][l]
        pairs, tt = _chunk_trips(k, chunk)
        CW = Ca[ix] @ Wm
        mag = Wm.T @ CW
        e = EW.T @ CW + CW.T @ EW + g(kK + 7 + pairs + 11, u) * mag
        val = Hi + Wl.T @ Cl[ix] @ Wl
        e = e + EHi + 2 * u * _ab(Hi)
        if nq:
            Tl, Tm, ETl = Ql[rows].T @ Wl, Qa[rows].T @ Wm, Qa[rows].T @ EW
            kt = dim + 6 + tt
            val = val - Tl.T @ Tl
            e = e + ETl.T @ Tm + Tm.T @ ETl + g(2 * kt + nq + 1, u) * (Tm.T @ Tm)
        # the long-double reference's own rounding: k dim-term dots on the same magnitudes
        e = e + (k * dim + nq + 8) * ULD * (mag + _ab(Hi) + ((Tm.T @ Tm) if nq else 0.0))
        out[t], bound[t] = val, e * ONE
    return out, bound


def landmark_check(sy, Cs, Q, blocks, ids=None, coords=1):
    """{'landmark': (err, bound), 'exact': messages} for the returned landmark blocks in solver (1) or landmark (0) coordinates."""
    ref, e = landmark_reference(sy, Cs, Q, ids)
    blocks = np.asarray(blocks, dtype=F)
    bad = [] if np.array_equal(blocks, blocks.transpose(0, 2, 1)) else ["a landmark block is not symmetric bit for bit"]
    if coords == 0:
        ch, u = sy.R.aux["chain"], sy.u
        ids_ = np.arange(sy.p.n_lms) if ids is None else np.asarray(ids)
        nm, w = ("JL_COL_SCALE", 3) if sy.dim == 12 else ("JL_COL_SCALE_H", 4)
        s, Es = sy.R.ref[nm].reshape(-1, w)[ids_], sy.R.bound[nm].reshape(-1, w)[ids_]
        rs = Es / _f(s)
        gmap = g(2, u)
        if sy.dim == 11:  # N_l Sigma N_l^T first (:522-533): N_l's entries with house4's g(25) (operand_bounds: dn), 3 + 3 terms
            import rounding_bounds as RB
            lw, lb = RB.house4(sy.p.lms.astype(LD)[ids_])
            Nl = (np.eye(4, dtype=LD)[None] - lb[:, None, None] * lw[:, :, None] * lw[:, None, :])[:, :, 1:]
            Nm = (np.eye(4)[None] + _f(lb)[:, None, None] * _ab(lw)[:, :, None] * _ab(lw)[:, None, :])[:, :, 1:]
            mag0 = Nm @ (_ab(ref) + e) @ Nm.transpose(0, 2, 1)
            e = Nm @ e @ Nm.transpose(0, 2, 1) + (g(6, u) + 2 * g(25, u)) * mag0
            ref = Nl @ ref @ Nl.transpose(0, 2, 1)
        ss = _f(s)[:, :, None] * _f(s)[:, None, :]
        mag = ss * (_ab(ref) + e)
        e = ss * e + (gmap + rs[:, :, None] + rs[:, None, :] + 40 * ULD) * mag
        ref = s[:, :, None] * ref * s[:, None, :]
    return {"landmark": (_ab(blocks.astype(LD) - ref), e * ONE), "exact": bad}


# ======== OBSERVATION
class ObsOperands:
    """Per observation, long double with magnitudes and operand errors: y [n, 3], L, M [n, 3, 3], J [n, 2, 3]."""


def observation_operands(sy):
    """What lane 0 of obs_cov forms at :649-683 and :704-705, from the caller's inputs and the reference chain -- module
    docstring: OBSERVATION.  Computed once per system."""
    if hasattr(sy, "_obs_operands"):
        return sy._obs_operands
    import rounding_bounds as RB
    p, u, ch = sy.p, sy.u, sy.R.aux["chain"]
    c, lm = p.cam_idx, p.lm
    n = len(c)
    o = ObsOperands()
    P = p.cams[c].reshape(n, 3, 4)
    Pl, Pa = P.astype(LD), np.abs(P)
    h, ha = sy.q.h, _ab(sy.q.h)
    o.y = np.einsum("nxk,nk->nx", Pl, h)
    o.Ey = g(4, u) * np.einsum("nxk,nk->nx", Pa, ha)
    rho = ch["rho"]
    if sy.dim == 12:
        s, ds = ch["s"][lm], (ch["Es"] / _f(ch["s"]))[lm]
        o.L = Pl[:, :, :3] * s[:, None, :]
        o.La = _ab(o.L)
        o.EL = o.La * (u + ds[:, None, :])
        w, sb2 = ch["w"], ch["sb2"]
        uv = p.obs.astype(LD)
        C9 = np.zeros((n, 3, 3), dtype=LD)
        C9[:, 0, 0] = C9[:, 1, 1] = 1
        C9[:, 0, 2] = C9[:, 2, 0] = -sb2 * uv[:, 0]
        C9[:, 1, 2] = C9[:, 2, 1] = -sb2 * uv[:, 1]
        C9[:, 2, 2] = sb2 * (uv[:, 0] * uv[:, 0] + uv[:, 1] * uv[:, 1])
        o.M = w[:, None, None] * C9
        o.Mm = _ab(o.M)
        o.EM = o.Mm * (g(10, u) + 2 * rho)[:, None, None]
    else:
        s = sy.R.ref["JL_COL_SCALE_H"].reshape(-1, 4)[lm]
        ds = (sy.R.bound["JL_COL_SCALE_H"].reshape(-1, 4) / _f(sy.R.ref["JL_COL_SCALE_H"].reshape(-1, 4)))[lm]
        q4 = Pl * s[:, None, :]
        q4a = _ab(q4)
        Eq4 = q4a * (u + ds[:, None, :])
        lw, lb = RB.house4(p.lms.astype(LD))
        lwo, lbo, lwa, lba = lw[lm], lb[lm], _ab(lw)[lm], _f(lb)[lm]
        o.L = np.stack([RB._nt(lwo, lbo, q4[:, x]) for x in range(3)], 1)
        o.La = _ab(o.L)
        Lm = np.stack([RB._nt(lwa, lba, q4a[:, x], +1) for x in range(3)], 1)
        o.EL = np.stack([RB._nt(lwa, lba, Eq4[:, x], +1) for x in range(3)], 1) + (g(8, u) + g(25, u)) * Lm
        sw, D, A, E = ch["sw"], ch["D"], ch["A"], ch["E"]
        w, wa = sw * sw, _f(sw) * _f(sw)
        m9, mm, em = np.zeros((n, 3, 3), dtype=LD), np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
        m9[:, 0, 0] = m9[:, 1, 1] = D[0] * D[0]
        mm[:, 0, 0] = mm[:, 1, 1] = A[0] * A[0]
        em[:, 0, 0] = em[:, 1, 1] = 2 * A[0] * E[0]
        for k in range(2):
            m9[:, k, 2] = m9[:, 2, k] = D[0] * D[k + 1]
            mm[:, k, 2] = mm[:, 2, k] = A[0] * A[k + 1]
            em[:, k, 2] = em[:, 2, k] = A[0] * E[k + 1] + A[k + 1] * E[0]
        m9[:, 2, 2] = D[1] * D[1] + D[2] * D[2]
        mm[:, 2, 2] = A[1] * A[1] + A[2] * A[2]
        em[:, 2, 2] = 2 * (A[1] * E[1] + A[2] * E[2])
        o.M = w[:, None, None] * m9
        o.Mm = wa[:, None, None] * mm
        o.EM = wa[:, None, None] * em + (g(5, u) + 2 * rho)[:, None, None] * o.Mm
    iz = 1 / o.y[:, 2]
    iza = _ab(iz)
    rz = o.Ey[:, 2] * iza + u
    o.J, o.Ja, o.EJ = np.zeros((n, 2, 3), dtype=LD), np.zeros((n, 2, 3)), np.zeros((n, 2, 3))
    for k in range(2):
        jk = -o.y[:, k] * iz * iz
        o.J[:, k, k], o.J[:, k, 2] = iz, jk
        o.EJ[:, k, k], o.EJ[:, k, 2] = iza * rz, _ab(jk) * (2 * rz + 2 * u) + o.Ey[:, k] * iza * iza
    o.Ja = _ab(o.J)
    sy._obs_operands = o
    return o


def observation_reference(sy, Cs, ids=None, mutate=None):
    """(rows [sum of the tracks of ids, 4] long double: h, c_uu, c_uv, c_vv per observation in the order of the call, their
    bound) -- module docstring: OBSERVATION.  Cs: the symmetric [n, n] C of cov_at's reads (c_symmetric).  mutate:
    reference-side defects: {"Q": the gauge basis} takes Sigma_l with the gauge correction, {"no_cross": True} drops R_i."""
    mutate = mutate or {}
    p, q, dim, u = sy.p, sy.q, sy.dim, sy.u
    ids = np.arange(p.n_lms) if ids is None else np.asarray(ids)
    o = observation_operands(sy)
    Sig, ESig = landmark_reference(sy, Cs, mutate.get("Q"), ids)
    tK = -(-dim * dim // 16)
    kK = tK + 2 + (2 if dim == 12 else 0)
    Cl, Ca = np.asarray(Cs, dtype=F).astype(LD), np.abs(np.asarray(Cs, dtype=F))
    n_rows = int(p.n_l[ids].sum())
    out, bound = np.zeros((n_rows, 4), dtype=LD), np.zeros((n_rows, 4))
    r0 = 0
    T = lambda A: A.transpose(0, 2, 1)
    mm = lambda A, B: np.einsum("ixz,izy->ixy", A, B)
    for t, l in enumerate(ids):
        a, b, rows, _ = SB._lm_index(p, int(l), dim)
        k = b - a
        ix = np.ix_(rows, rows)
        X, Xa = Cl[ix].reshape(k, dim, k * dim), Ca[ix].reshape(k, dim, k * dim)
        U, Um, EU = q.U[a:b], q.Um[a:b], q.EU[a:b]
        G, Gm, EG = q.G[a:b], q.Gm[a:b], q.EG[a:b]
        # K[i, j] = U_i C_ij U_j^T and its magnitude / operand error, [k, k, 3, 3]
        right = lambda Y, V: np.einsum("iajc,jbc->ijab", Y.reshape(k, 3, k, dim), V)
        K = right(U @ X, U)
        UmX = Um @ Xa
        Km = right(UmX, Um)
        EK = right(EU @ Xa, Um) + right(UmX, EU)
        R = np.einsum("ijab,jbm->iam", K, G)
        Rm = np.einsum("ijab,jbm->iam", Km, Gm)
        ER = np.einsum("ijab,jbm->iam", EK, Gm) + np.einsum("ijab,jbm->iam", Km, EG) + g(kK + 7 + k, u) * Rm
        if mutate.get("no_cross"):
            R = np.zeros_like(R)
        d = np.arange(k)
        Kii, Kiim = K[d, d], Km[d, d]
        EKii = EK[d, d] + g(kK + 4, u) * Kiim
        L, La, EL = o.L[a:b], o.La[a:b], o.EL[a:b]
        S, Sa_, ES = Sig[t][None], _ab(Sig[t])[None], ESig[t][None]
        Ra = _ab(R)
        RL, RLa = mm(R, T(L)), mm(Ra, T(La))
        ERL = mm(ER, T(La)) + mm(Ra, T(EL)) + g(3, u) * RLa
        LSL, LSLa = mm(mm(L, S), T(L)), mm(mm(La, Sa_), T(La))
        ELSL = mm(mm(EL, Sa_), T(La)) + mm(mm(La, Sa_), T(EL)) + mm(mm(La, ES), T(La)) + g(6, u) * LSLa
        Syy = Kii - RL - T(RL) + LSL
        Smag = _ab(Kii) + RLa + T(RLa) + LSLa
        ESyy = EKii + ERL + T(ERL) + ELSL + g(3, u) * Smag
        # the long-double reference's own rounding: k dim-term dots on the same magnitudes
        RmL = mm(Rm, T(La))
        ESyy = ESyy + (k * (dim + 3) + 20) * ULD * (Kiim + RmL + T(RmL) + LSLa)
        Sa = _ab(Syy) + ESyy
        M, Mm, EM = o.M[a:b], o.Mm[a:b], o.EM[a:b]
        lev = (M * Syy).sum((1, 2))
        Elev = (Mm * ESyy + EM * Sa).sum((1, 2)) + (g(9, u) + 20 * ULD) * (Mm * Sa).sum((1, 2))
        J, Ja, EJ = o.J[a:b], o.Ja[a:b], o.EJ[a:b]
        A = mm(J, Syy)
        Am = mm(Ja, Sa)
        EA = mm(Ja, ESyy) + mm(EJ, Sa) + g(2, u) * Am
        O = mm(A, T(J))
        Om = mm(Am, T(Ja))
        EO = mm(EA, T(Ja)) + mm(Am, T(EJ)) + (g(2, u) + 20 * ULD) * Om
        out[r0:r0 + k] = np.stack([lev, O[:, 0, 0], O[:, 0, 1], O[:, 1, 1]], 1)
        bound[r0:r0 + k] = np.stack([Elev, EO[:, 0, 0], EO[:, 0, 1], EO[:, 1, 1]], 1) * ONE
        r0 += k
    return out, bound


def observation_check(sy, Cs, rows, ids=None, ref=None):
    """{'observation_h': (err, bound) [rows], 'observation_c': (err, bound) [rows, 3], 'exact': messages} for the rows of one
    call; ref: observation_reference's result for the same Cs and ids, when it is at hand."""
    want, e = observation_reference(sy, Cs, ids) if ref is None else ref
    rows = np.asarray(rows, dtype=F)
    assert rows.shape == want.shape, (rows.shape, want.shape)
    bad = []
    if not np.all(np.isfinite(rows)):
        bad.append("non-finite entries in the observation rows")
    ids_ = np.arange(sy.p.n_lms) if ids is None else np.asarray(ids)
    start = np.r_[0, np.cumsum(sy.p.n_l[ids_])]
    first = {}
    for t, l in enumerate(ids_.tolist()):
        if l in first and not np.array_equal(rows[start[t]:start[t + 1]], rows[start[first[l]]:start[first[l] + 1]]):
            bad.append(f"landmark {l} requested twice returns different bits")
        first.setdefault(l, t)
    err = _ab(rows.astype(LD) - want)
    err = np.where(np.isfinite(rows), err, np.inf)
    return {"observation_h": (err[:, 0], e[:, 0]), "observation_c": (err[:, 1:], e[:, 1:]), "exact": bad}


# ======== fp64 emulations in the kernels' operation order (order 0: ascending sums, order 1: descending)
def _dot(A, B, order):
    """A B with the inner index summed ascending (0) or descending (1)."""
    return A @ B if order == 0 else A[:, ::-1] @ B[::-1, :]


def _tree(x, order):
    """Pairwise sum over the last axis (a power of two): halves (order 0) or even / odd neighbours (order 1)."""
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:] if order == 0 else x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _strided_sum(terms, lanes, order):
    """Sum over the last axis as `lanes` threads do: thread t adds the terms t, t + lanes, ... in turn (order 1: from the last
    one), then a pairwise tree over the threads."""
    m = terms.shape[-1]
    trips = -(-m // lanes)
    x = np.zeros(terms.shape[:-1] + (trips * lanes,))
    x[..., :m] = terms
    x = x.reshape(terms.shape[:-1] + (trips, lanes))
    acc = np.zeros(terms.shape[:-1] + (lanes,))
    for t in (range(trips) if order == 0 else range(trips - 1, -1, -1)):
        acc = acc + x[..., t, :]
    return _tree(acc, order)


def emulate_gauge(cams, sig, ncw, dim):
    """gauge_basis (cov_plan.hpp) in fp64: (Q [n, nq], ok)."""
    nq = 12 if dim == 12 else 15
    P, s = np.asarray(cams, dtype=F).reshape(-1, 12), np.asarray(sig, dtype=F).reshape(-1, 12)
    V = []
    for col in range(nq):
        gi, gj = divmod(col, 4)
        G = np.zeros_like(P)
        for r in range(3):
            G[:, 4 * r + gj] = -P[:, 4 * r + gi]
        if dim == 12:
            V.append((G / s).reshape(-1))
            continue
        w, beta = ncw[:, :12], ncw[:, 12]
        h0 = -beta[:, None] * w * w[:, :1]
        h0[:, 0] += 1.0
        a = -(h0 * (G / s)).sum(1) / (h0 * (P / s)).sum(1)
        y = (G + a[:, None] * P) / s
        V.append((y[:, 1:] - (beta * (w * y).sum(1))[:, None] * w[:, 1:]).reshape(-1))
    for k in range(nq):
        norm0 = np.sqrt(V[k] @ V[k])
        for _ in range(2):
            for j in range(k):
                V[k] = V[k] - (V[j] @ V[k]) * V[j]
        norm = np.sqrt(V[k] @ V[k])
        if not norm > 1e-8 * norm0:
            return None, False
        V[k] = V[k] / norm
    return np.stack(V, 1), True


def emulate_inverse(R, order, mutate=None):
    """cov_diag_inv and the two cov_trmm products per block column, in place on a copy of the upper triangular R."""
    mutate = mutate or {}
    M = np.triu(np.asarray(R, dtype=F))
    N = M.shape[0]
    for j in range(N // NB):
        cj = slice(NB * j, NB * j + NB)
        Rb = M[cj, cj].copy()
        Wb = np.zeros((NB, NB))
        for c in range(NB):
            Wb[c, c] = 1.0 / Rb[c, c]
        for jj in range(1, NB):
            s = _dot(Wb[:, :jj], Rb[:jj, jj:jj + 1], order)[:, 0]
            rows = np.arange(NB) < jj
            Wb[rows, jj] = (-s / Rb[jj, jj])[rows]
        M[cj, cj] = Wb
        if j == 0:
            continue
        T = np.concatenate([_dot(M[NB * i:NB * i + NB, cj], Wb, order) for i in range(j)], 0)
        for i in range(j):
            ri = slice(NB * i, NB * i + NB)
            k_first, alpha = i, -1.0
            if mutate.get("trmm_k_first") == (i, j):
                k_first = i + 1
            if mutate.get("trmm_alpha") == (i, j):
                alpha = 1.0
            M[ri, cj] = alpha * _dot(M[ri, NB * k_first:NB * j], T[NB * k_first:NB * j], order)
    if "w_tile" in mutate:
        i, j = mutate["w_tile"]
        M[NB * i:NB * i + 16, NB * j:NB * j + 2] *= 1 + 1e-10
    return M


def emulate_camera(W, Q, n, dim, order, mutate=None):
    """cov_gram and cov_finish in solver coordinates: [n_cams, dim, dim]."""
    mutate = mutate or {}
    W = np.asarray(W, dtype=F)
    n_cams = n // dim
    out = np.zeros((n_cams, dim, dim))
    for c in range(n_cams):
        r0 = dim * c
        V = W[r0:r0 + dim, :n].copy()
        k = np.arange(n)[None, :]
        row = r0 + np.arange(dim)[:, None]
        V[(k <= row) if mutate.get("gram_mask") == c else (k < row)] = 0.0
        T = _strided_sum(V[:, None, r0:] * V[None, :, r0:], 256, order)  # (thread t starts at column r0 + t)
        if Q is not None:
            Qc = Q[r0:r0 + dim]
            s = _dot(Qc, Qc.T, order)
            times = {"qqt_twice": 2.0, "qqt_none": 0.0}.get(mutate.get("qqt", (None, None))[0] if mutate.get("qqt", (None, -1))[1] == c else None, 1.0)
            T = T - times * s
        out[c] = np.triu(T) + np.triu(T, 1).T
    return out


def emulate_camera_coords(T, sig, ncw, dim, mutate=None):
    """cov_finish's map to camera coordinates on solver-coordinate blocks, [n_cams, 12, 12]."""
    mutate = mutate or {}
    T = np.asarray(T, dtype=F)
    sig = np.asarray(sig, dtype=F).reshape(-1, 12)
    if dim == 11:
        w, beta = ncw[:, :12], ncw[:, 12]
        Nm = (np.eye(12)[None] - beta[:, None, None] * w[:, :, None] * w[:, None, :])[:, :, 1:]
        T = Nm @ (T @ Nm.transpose(0, 2, 1))
    left = sig.copy()
    out = left[:, :, None] * T * sig[:, None, :]
    if "sigma_j_for_i" in mutate:
        c = mutate["sigma_j_for_i"]
        out[c] = sig[c][None, :] * T[c] * sig[c][None, :]
    return np.triu(out) + np.triu(out, 1).transpose(0, 2, 1)


def emulate_landmark_coords(S, q, p, ids=None):
    """lm_cov's map to landmark coordinates (:512-537): s_x Sigma_xy s_y (step 1), s_i (N_l Sigma N_l^T)_ij s_j (step 2), mirrored."""
    ids = np.arange(p.n_lms) if ids is None else np.asarray(ids)
    S = np.asarray(S, dtype=F)
    if q.dim == 12:
        s = q.em["JL_COL_SCALE"].reshape(-1, 3)[ids]
    else:
        import rounding_bounds as RB
        s = q.em["JL_COL_SCALE_H"].reshape(-1, 4)[ids]
        lw, lb = RB.house4(p.lms[ids])
        Nl = (np.eye(4)[None] - lb[:, None, None] * lw[:, :, None] * lw[:, None, :])[:, :, 1:]
        S = Nl @ (S @ Nl.transpose(0, 2, 1))
    out = s[:, :, None] * S * s[:, None, :]
    return np.triu(out) + np.triu(out, 1).transpose(0, 2, 1)


def emulate_lauum(W, order, mutate=None):
    """cov_lauum on the upper triangular W: (the dense matrix with C in its strictly lower blocks, the panel)."""
    mutate = mutate or {}
    W = np.triu(np.asarray(W, dtype=F))
    N = W.shape[0]
    nb = N // NB
    M, panel = W.copy(), np.zeros((N, NB))
    for I in range(nb):
        for J in range(I + 1):
            k0, k1 = I, nb
            if mutate.get("lauum_k_start") == (I, J):
                k0 = I + 1
            if mutate.get("lauum_k_end") == (I, J):
                k1 = nb - 1
            A, B = W[NB * I:NB * I + NB, NB * k0:NB * k1], W[NB * J:NB * J + NB, NB * k0:NB * k1]
            Cb = _dot(A, B.T, order) if k1 > k0 else np.zeros((NB, NB))
            if mutate.get("c_tile") == (I, J):
                Cb[0:2, 32:48] *= 1 + 1e-10
            if I == J:
                panel[NB * I:NB * I + NB] = Cb
            else:
                M[NB * I:NB * I + NB, NB * J:NB * J + NB] = Cb
    return M, panel


def emulate_landmarks(p, q, inv, panel, Q, dim, order, ids=None, mutate=None):
    """lm_cov's contraction in solver coordinates from the fp64 staged operands q (sc_bounds._emu_pieces_*): [len(ids), 3, 3]."""
    mutate = mutate or {}
    ids = np.arange(p.n_lms) if ids is None else np.asarray(ids)
    Hi_all = q.em["HLL_INV"].reshape(-1, 3, 3)
    out = np.zeros((len(ids), 3, 3))
    for t, l in enumerate(ids):
        a, b = int(p.lm_off[l]), int(p.lm_off[l + 1])
        k = b - a
        cams = p.cam_idx[a:b]
        acc = np.zeros((16, 3, 3))
        pairs = [(i, j) for i in range(k) for j in range(i, k)]
        for i, j in (pairs if order == 0 else pairs[::-1]):
            r = dim * cams[i] + np.arange(dim)
            c = dim * cams[j] + np.arange(dim)
            rr, cc = r[:, None], c[None, :]
            if mutate.get("cov_at") == "transposed" and (cams[i] * dim) // NB != (cams[i] * dim + dim - 1) // NB and i == j:
                # a diagonal-tile entry read transposed across the 64-edge: the (upper) panel entry instead of the lower block
                Cb = np.where((rr >> 6) != (cc >> 6), np.asarray(panel)[np.minimum(rr, cc), np.maximum(rr, cc) & 63], cov_at(inv, panel, rr, cc))
            elif mutate.get("cov_at") == "wrong_buffer":
                Cb = np.asarray(inv)[np.maximum(rr, cc), np.minimum(rr, cc)]
            else:
                Cb = cov_at(inv, panel, rr, cc)
            terms = (q.U[a + i][:, None, :, None] * Cb[None, None, :, :]) * q.U[a + j][None, :, None, :]
            K = _strided_sum(terms.reshape(3, 3, dim * dim), 16, order)
            P = _dot(q.G[a + i].T, _dot(K, q.G[a + j], order), order)
            slot = (i * k + j) % 16  # (the 16-lane group of the pair: its own accumulator)
            acc[slot] += P if (i == j or mutate.get("no_transpose") == int(l)) else P + P.T
        acc = _tree(np.moveaxis(acc, 0, -1), order)
        tt = np.zeros((3, 3))
        if Q is not None:
            Tg = np.zeros((4, Q.shape[1], 3))
            for i in (range(k) if order == 0 else range(k - 1, -1, -1)):
                if mutate.get("t_group") == int(l) and i % 4 == 1:
                    continue
                ta = _dot(Q[dim * cams[i]:dim * cams[i] + dim].T, q.U[a + i].T, order)
                Tg[i % 4] += _dot(ta, q.G[a + i], order)
            Tl = ((Tg[0] + Tg[1]) + Tg[2]) + Tg[3]
            tt = _dot(Tl.T, Tl, order)
        S = Hi_all[l] + acc - tt
        out[t] = np.triu(S) + np.triu(S, 1).T
    return out


def _dot3(A, B, order):
    """A B for 3 x 3 operands (leading axes broadcast) as the kernel's three-term dots: a0 b0 + a1 b1 + a2 b2 (order 1: from
    the last term)."""
    t = [A[..., :, z, None] * B[..., None, z, :] for z in (range(3) if order == 0 else range(2, -1, -1))]
    return (t[0] + t[1]) + t[2]


def emulate_observations(p, q, inv, panel, sig, dim, order, ids=None, mutate=None):
    """obs_cov (:559-715) in fp64 from the staged operands q and `sig` = emulate_landmarks(.., Q=None) of the same ids: lane gl's
    share e = gl, gl + 16, ... of every K_ij, the j walk over all chunks, the butterfly as a tree, lane 0's expressions.
    Returns the rows [sum of the tracks, 4].  mutate -- one defect each (mutations_obs):
      c_tile: (I, J)      the reads of that 64 x 64 tile of C scaled by 1 + 1e-10
      sw_f32, iz_f32, r_f32: True   that quantity rounded to single precision
      kii_any_chunk: l    K_ii copied at j == i of every chunk (the last one stays)
      skip_last_j: l      the last j of a full chunk left out
      unmasked: l         the groups with i >= ni of the last pass of 16 write the rows behind the track
      stale_oj: l         oj not staged again at jc = 0 when ic advances"""
    mutate = mutate or {}
    ids = np.arange(p.n_lms) if ids is None else np.asarray(ids)
    chunk = 64 if dim == 12 else 32
    dd = dim * dim
    trips = -(-dd // 16)
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(F)
    P = p.cams.reshape(-1, 3, 4)
    sw = f32(q.sw) if mutate.get("sw_f32") else q.sw
    if dim == 12:
        s_all = q.em["JL_COL_SCALE"].reshape(-1, 3)
        sb2 = q.sb * q.sb
    else:
        import rounding_bounds as RB
        s_all = q.em["JL_COL_SCALE_H"].reshape(-1, 4)
        lw, lb = RB.house4(p.lms)
    inv_, panel_ = np.asarray(inv), np.asarray(panel)
    n_rows = int(p.n_l[ids].sum())
    out = np.zeros((n_rows, 4))
    stray = []  # (row, values) written by an unmasked group: after everything else
    seq = (lambda n: range(n)) if order == 0 else (lambda n: range(n - 1, -1, -1))
    row0 = 0
    for t, l in enumerate(ids.tolist()):
        a, b = int(p.lm_off[l]), int(p.lm_off[l + 1])
        k = b - a
        cams = p.cam_idx[a:b]
        oj = np.zeros(chunk, dtype=np.int64)  # the observation each entry of oj holds
        staged = -1
        for ic in range(0, k, chunk):
            ni = min(chunk, k - ic)
            for i0 in range(0, ni, 16):
                last_pass = i0 + 16 >= ni
                groups = range(i0, i0 + 16) if (mutate.get("unmasked") == l and last_pass and ic + chunk >= k) else range(i0, min(i0 + 16, ni))
                partial = {}
                for jc in range(0, k, chunk):
                    nj = min(chunk, k - jc)
                    if staged != jc:
                        if not (mutate.get("stale_oj") == l and ic > 0 and jc == 0 and i0 == 0):
                            oj[:nj] = jc + np.arange(nj)
                        staged = jc
                    nj_walk = nj - 1 if (mutate.get("skip_last_j") == l and nj == chunk) else nj
                    js = oj[:nj_walk]
                    for i in groups:
                        oi = ic + (i if i < ni else i % ni)  # (an unmasked group reads what the entry held: modelled as i mod ni)
                        r = dim * cams[oi] + np.arange(dim)
                        cc = (dim * cams[js][:, None] + np.arange(dim)[None, :])  # [nj, dim]
                        Cb = cov_at(inv_, panel_, r[None, :, None], cc[:, None, :])  # [nj, dim, dim]
                        if "c_tile" in mutate:
                            I, J = mutate["c_tile"]
                            rr, c2 = np.maximum(r[None, :, None], cc[:, None, :]), np.minimum(r[None, :, None], cc[:, None, :])
                            Cb = np.where(((rr >> 6) == I) & ((c2 >> 6) == J), Cb * (1 + 1e-10), Cb)
                        Ui, Uj = q.U[a + oi], q.U[a + js]  # [3, dim], [nj, 3, dim]
                        terms = (Ui[None, :, None, :, None] * Cb[:, None, None, :, :]) * Uj[:, None, :, None, :]  # [nj, x, y, r, c]
                        x = np.zeros((len(js), 3, 3, trips * 16))
                        x[..., :dd] = terms.reshape(len(js), 3, 3, dd)
                        x = x.reshape(len(js), 3, 3, trips, 16)
                        Kl = np.zeros((len(js), 3, 3, 16))
                        for tr in seq(trips):
                            Kl = Kl + x[:, :, :, tr, :]
                        Kl = np.moveaxis(Kl, -1, 1)  # [nj, lane, 3, 3]
                        KG = _dot3(Kl, q.G[a + js][:, None], order)
                        Rl, Kii = partial.get(i, (np.zeros((16, 3, 3)), np.zeros((16, 3, 3))))
                        for jj in seq(len(js)):
                            Rl = Rl + KG[jj]
                            if jj == (i if i < ni else -1) and (jc == ic or mutate.get("kii_any_chunk") == l):
                                Kii = Kl[jj]
                        partial[i] = (Rl, Kii)
                for i in groups:
                    Rl, Kii = partial[i]
                    R = _tree(np.moveaxis(Rl, 0, -1), order)
                    Kii = _tree(np.moveaxis(Kii, 0, -1), order)
                    if mutate.get("r_f32"):
                        R = f32(R)
                    oi = ic + (i if i < ni else i % ni)
                    o = a + oi
                    Pc = P[cams[oi]]
                    h = q.h[o]
                    w = sw[o] * sw[o]
                    yv = ((Pc[:, 0] * h[0] + Pc[:, 1] * h[1]) + Pc[:, 2] * h[2]) + Pc[:, 3] * h[3]
                    if dim == 12:
                        L = Pc[:, :3] * s_all[l][None, :]
                        u_, v_ = p.obs[o]
                        cu, cv, cuv = sb2 * u_, sb2 * v_, sb2 * (u_ * u_ + v_ * v_)
                        Mi = w * np.array([[1, 0, -cu], [0, 1, -cv], [-cu, -cv, cuv]])
                    else:
                        q4 = Pc * s_all[l][None, :]
                        aw = ((q4[:, 0] * lw[l, 0] + q4[:, 1] * lw[l, 1]) + q4[:, 2] * lw[l, 2]) + q4[:, 3] * lw[l, 3]
                        L = q4[:, 1:] - (lb[l] * aw)[:, None] * lw[l, None, 1:]
                        D00, D02, D12 = (x_[o] for x_ in q.D)
                        Mi = w * np.array([[D00 * D00, 0, D00 * D02], [0, D00 * D00, D00 * D12],
                                           [D00 * D02, D00 * D12, D02 * D02 + D12 * D12]])
                    Sg = sig[t]
                    SL = _dot3(Sg, L.T, order)
                    rl, lr, lsl = _dot3(R, L.T, order), _dot3(L, R.T, order), _dot3(L, SL, order)
                    Syy = Kii - rl - lr + lsl
                    Syy = np.triu(Syy) + np.triu(Syy, 1).T
                    lev = 0.0
                    for e in seq(9):
                        lev = lev + Mi.reshape(-1)[e] * Syy.reshape(-1)[e]
                    iz = 1.0 / yv[2]
                    if mutate.get("iz_f32"):
                        iz = float(f32(iz))
                    j0, j1 = -yv[0] * iz * iz, -yv[1] * iz * iz
                    a0 = iz * Syy[0] + j0 * Syy[2]
                    a1 = iz * Syy[1] + j1 * Syy[2]
                    row = [lev, a0[0] * iz + a0[2] * j0, a0[1] * iz + a0[2] * j1, a1[1] * iz + a1[2] * j1]
                    if i < ni:
                        out[row0 + ic + i] = row
                    elif row0 + ic + i < n_rows:
                        stray.append((row0 + ic + i, row))
        row0 += k
    for r, row in stray:
        out[r] = row
    return out


# ======== the cases of tests/test_cov_bounds.py and tests/test_gpu_cov_bounds.py
def case_problem(name, step, robust="NONE", lam=0.0):
    """The operand_bounds problem of one covariance case: the state of tests/landmark_covariance_reference.py (step 1 with the
    Jl column scaling on, the library's default)."""
    import landmark_covariance_reference as L
    p = L.problem(name)
    cams, lms, obs = L.state(p, step)
    if step == 1:
        return OB.Pose(p.n_cams, p.lm_off, p.cam_idx, obs, cams, lms, L.ALPHA, lam, robust, L.HUBER[1], scale_jl=True)
    return OB.Joint(p.n_cams, p.lm_off, p.cam_idx, obs, cams, lms, lam, robust, L.HUBER[2])


# (name, step, robust, lambda; lambda = 0: the free gauge)
CASES = ([("small", s, "NONE", lam) for s in (1, 2) for lam in (0.0, 1e-4)] + [("p22", 2, "NONE", 0.0)] +
         [("p24", s, "NONE", 0.0) for s in (1, 2)] + [("medium", s, "NONE", lam) for s in (1, 2) for lam in (1e-4, 1.0)] +
         [("long", s, "NONE", 0.0) for s in (1, 2)] + [("small", s, "HUBER", 0.0) for s in (1, 2)])


# the cases of the OBSERVATION stage: the smallest shapes that reach every loop edge of obs_cov (`tracks`:
# landmark_covariance_reference.TRACK_EDGES), the robust weight, the damped system
OBS_CASES = ([("small", s, "NONE", lam) for s in (1, 2) for lam in (0.0, 1e-4)] + [("small", s, "HUBER", 0.0) for s in (1, 2)] +
             [("medium", s, "NONE", lam) for s in (1, 2) for lam in (1e-4, 1.0)] + [("tracks", s, "NONE", 0.0) for s in (1, 2)])

_SYS, _EMU = {}, {}


def system(name, step, robust, lam):
    """The reference of one case (sc_bounds.dense_system at the case's lambda), computed once, shared by the CPU and the GPU
    module and left unchanged."""
    key = (name, step, robust, lam)
    if key not in _SYS:
        _SYS[key] = SB.dense_system(case_problem(name, step, robust, lam), step == 2)
    return _SYS[key]


def emulated(name, step, robust, lam, order):
    """emulate_case of one case and summation order (the observation rows: on OBS_CASES), computed once and left unchanged."""
    key = (name, step, robust, lam, order)
    if key not in _EMU:
        _EMU[key] = emulate_case(system(name, step, robust, lam).p, step == 2, order, obs=(name, step, robust, lam) in OBS_CASES)
    return _EMU[key]


def report(tag, out, bad):
    """Print the worst err / bound of every check ("COVBOUND ..."), then assert that no entry is over and every exact fact holds."""
    ratios = {k: worst(*v) for k, v in out.items()}
    print(f"COVBOUND {tag} " + " ".join(f"{k}={r[0]:.3g}" for k, r in ratios.items()))
    over = [f"{k}: {r[2]} entries over, worst {r[0]:.3g} at flat index {r[1]}" for k, r in ratios.items() if r[2]]
    assert not bad and not over, "\n".join(bad + over)


def pair_tile_counts(p, dim):
    """The numbers of 64 x 64 tiles the dim x dim blocks C[c_i, c_j] of the camera pairs of some landmark lie on (1, 2 or 4)."""
    seen = set()
    for l in range(p.n_lms):
        cams = p.cam_idx[p.lm_off[l]:p.lm_off[l + 1]]
        span = (dim * cams + dim - 1) // NB - (dim * cams) // NB + 1
        seen |= {int(a * b) for a in set(span.tolist()) for b in set(span.tolist())}
    return seen


def emulate_case(p, joint, order, mutate=None, obs=True):
    """The whole chain in fp64: assembly (sc_bounds.emulate_assembly), Q Q^T, factor, inverse, camera blocks, C, landmark
    blocks, observation rows (obs; sig0: the Sigma_l without the gauge correction that obs_cov reads).  Returns a dict of what
    the device hands out: R, Q, inv, panel, cam, lm (solver coordinates), obs and the operands q."""
    mutate = mutate or {}
    M, _, q = SB.emulate_assembly(p, joint, order)
    dim = q.dim
    n = dim * p.n_cams
    N = padded(n)
    Q = None
    if p.lam == 0.0:
        Q, ok = emulate_gauge(p.cams, q.sig, getattr(q, "ncw", None), dim)
        assert ok
        M[:n, :n] += np.triu(_dot(Q, Q.T, order))
    buf, info = SB.emulate_factor(M)
    assert info == 0
    R = np.triu(buf[:, :N])
    W = emulate_inverse(R, order, mutate)
    cam = emulate_camera(W, Q, n, dim, order, mutate)
    inv, panel = emulate_lauum(W, order, mutate)
    lm = emulate_landmarks(p, q, inv, panel, Q, dim, order, mutate=mutate)
    d = dict(R=R, Q=Q, inv=inv, panel=panel, cam=cam, lm=lm, q=q, n=n, N=N, dim=dim)
    if obs:  # obs_cov reads lm_cov's output with nq = 0 (povar_cov.hip: observation_rows), whatever the gauge
        d["sig0"] = lm if Q is None else emulate_landmarks(p, q, inv, panel, None, dim, order)
        d["obs"] = emulate_observations(p, q, inv, panel, d["sig0"], dim, order)
    return d


def check_all(sy, d, coords=1, ids=None):
    """Every check of the module docstring on one set of buffers (the device's, or emulate_case's): {check: (err, bound)} and
    the list of exact facts that do not hold.  The camera, landmark and observation checks run on what d holds of `cam`,
    `lm` (both in `coords`) and `obs`: an observation call returns rows only."""
    out, bad = {}, []
    Cs = c_symmetric(d["inv"], d["panel"])[:sy.n, :sy.n]
    stages = [assembly_check(sy, d["R"], d["Q"]), inverse_check(d["R"], d["inv"], sy.n)]
    if "cam" in d:
        stages.append(camera_check(d["inv"], d["Q"], d["cam"], sy.n, sy.dim, coords, sy))
    stages.append(lauum_check(d["inv"], d["panel"]))
    if "lm" in d:
        stages.append(landmark_check(sy, Cs, d["Q"], d["lm"], ids, coords))
    if "obs" in d:  # (the rows have no coordinates: gauge- and scaling-invariant)
        stages.append(observation_check(sy, Cs, d["obs"], ids))
    for res in stages:
        bad += res.pop("exact", [])
        out.update(res)
    if d["Q"] is not None:
        out["gauge"] = gauge_check(d["Q"])
        e, b, _ = gauge_span(sy, d["Q"])
        out["span"] = (e, b)
    return out, bad


# ======== mutations: (name, mutate dict, check, the flat indices of that check the mutation touches)
def mutations(d, p):
    """Plausible kernel defects applied to the emulated output (emulate_case's mutate): each must be reported by `check` on the
    entries it touches, and every other check must stay clean (tests/test_cov_bounds.py)."""
    N, n, dim = d["N"], d["n"], d["dim"]
    nb = N // NB
    tile = lambda I, J, r0=0, r1=NB, c0=0, c1=NB: {(NB * I + r) * N + NB * J + c for r in range(r0, r1) for c in range(c0, c1)}
    cam_blk = lambda c: {c * dim * dim + e for e in range(dim * dim)}
    lm_blk = lambda ls: {9 * int(l) + e for l in ls for e in range(9)}
    l3 = int(np.flatnonzero(p.n_l >= 3)[0])
    # a camera whose rows straddle a 64-edge, observed by some landmark
    strad = [c for c in range(p.n_cams) if (dim * c) // NB != (dim * c + dim - 1) // NB and p.n_c[c] > 0]
    out = [("lauum_k_start", {"lauum_k_start": (nb - 1, 0)}, "lauum", tile(nb - 1, 0)),
           ("lauum_k_end", {"lauum_k_end": (0, 0)}, "lauum", tile(0, 0)),
           ("trmm_k_first", {"trmm_k_first": (0, nb - 1)}, "inverse", tile(0, nb - 1)),
           ("trmm_alpha", {"trmm_alpha": (0, 1)}, "inverse", tile(0, 1)),
           ("gram_mask_le", {"gram_mask": 1}, "camera", cam_blk(1)),
           ("w_tile_1e-10", {"w_tile": (0, nb - 1)}, "inverse", tile(0, nb - 1, 0, 16)),  # (an entry of W enters its row of W R)
           ("c_tile_1e-10", {"c_tile": (1, 0)}, "lauum", tile(1, 0, 0, 2, 32, 48)),
           ("no_transpose", {"no_transpose": l3}, "landmark", {9 * l3 + e for e in range(9)}),
           # every landmark has its i == j pairs, whose entries lie on diagonal tiles: the wrong buffer touches every block
           ("cov_at_wrong_buffer", {"cov_at": "wrong_buffer"}, "landmark", lm_blk(range(p.n_lms)))]
    if strad:  # the own block of a camera across a 64-edge, read by the landmarks that observe such a camera
        seen = [l for l in range(p.n_lms) if np.isin(p.cam_idx[p.lm_off[l]:p.lm_off[l + 1]], strad).any()]
        out.append(("cov_at_transposed", {"cov_at": "transposed"}, "landmark", lm_blk(seen)))
    if d["Q"] is not None:
        out += [("qqt_twice", {"qqt": ("qqt_twice", 2)}, "camera", cam_blk(2)),
                ("qqt_none", {"qqt": ("qqt_none", 2)}, "camera", cam_blk(2)),
                ("t_group_skipped", {"t_group": l3}, "landmark", {9 * l3 + e for e in range(9)})]
    return out


def obs_chunk(dim):
    """SCD_CHUNK / SCDH_CHUNK (povar_kernels_sc.hpp): the staging chunk of obs_cov."""
    return 64 if dim == 12 else 32


def mutations_obs(sy, d):
    """Plausible defects of obs_cov alone, applied to the emulated rows (emulate_observations' mutate; "corrected": Sigma_l
    taken with the gauge correction, i.e. d["lm"] for d["sig0"]): (name, mutate, the checks that must report it, the rows of
    an all-landmark call it touches).  Every buffer the other checks read stays as it is.  A mutation is listed where the
    shape has what it needs (tests/test_cov_bounds.py asserts which shapes do)."""
    p, dim, q = sy.p, sy.dim, d["q"]
    chunk = obs_chunk(dim)
    both, every = ("observation_h", "observation_c"), set(range(len(p.cam_idx)))
    track = lambda l: set(range(int(p.lm_off[l]), int(p.lm_off[l + 1])))
    blk = lambda c: {(dim * int(c)) // NB, (dim * int(c) + dim - 1) // NB}
    out = [("iz_f32", {"iz_f32": True}, ("observation_c",), every), ("r_f32", {"r_f32": True}, both, every)]
    # a tile of C off the diagonal that the pair (a camera across a 64-edge, a camera of an earlier block row) of some landmark reads
    tile = None
    for l in range(p.n_lms):
        cams = p.cam_idx[p.lm_off[l]:p.lm_off[l + 1]]
        for ca in cams:
            lo = [cb for cb in cams if len(blk(ca)) == 2 and max(blk(cb)) < min(blk(ca))]
            if lo and tile is None:
                tile = (max(blk(ca)), max(blk(lo[0])))
    if tile is not None:
        rows = set()
        for l in range(p.n_lms):
            a, b = int(p.lm_off[l]), int(p.lm_off[l + 1])
            in_i = np.array([tile[0] in blk(c) for c in p.cam_idx[a:b]])
            in_j = np.array([tile[1] in blk(c) for c in p.cam_idx[a:b]])
            if in_i.any() and in_j.any():
                rows |= {a + int(i) for i in np.flatnonzero(in_i | in_j)}
        out.append(("c_tile_1e-10", {"c_tile": tile}, both, rows))
    if p.robust == "HUBER" and np.any(q.sw < 1):
        out.append(("sw_f32", {"sw_f32": True}, ("observation_h",), set(np.flatnonzero(q.sw < 1).tolist())))
    if d["Q"] is not None:
        out.append(("corrected", {"corrected": True}, both, every))
    k = p.n_l
    two = np.flatnonzero((k > chunk) & (k <= 2 * chunk))
    if len(two):  # (the rows i < k - chunk of the first chunk meet their own index again in the second one)
        l = int(two[0])
        out.append(("kii_any_chunk", {"kii_any_chunk": l}, both, {int(p.lm_off[l]) + i for i in range(int(k[l]) - chunk)}))
    full = np.flatnonzero(k == chunk)
    if len(full):
        out.append(("skip_last_j", {"skip_last_j": int(full[0])}, both, track(int(full[0]))))
    l17 = np.flatnonzero(k == 17)
    if len(l17) and int(p.lm_off[l17[0] + 1]) < len(p.cam_idx):
        l = int(l17[0])
        out.append(("unmasked", {"unmasked": l}, both, {r for r in range(int(p.lm_off[l]) + 17, int(p.lm_off[l]) + 32) if r < len(p.cam_idx)}))
    if k.max() > chunk:  # (the first pass of sixteen of every later chunk walks the chunk staged last)
        l = int(np.argmax(k))
        out.append(("stale_oj", {"stale_oj": l}, both,
                    {int(p.lm_off[l]) + i for ic in range(chunk, int(k[l]), chunk) for i in range(ic, min(ic + 16, int(k[l])))}))
    return out


def emulate_obs_mutation(sy, d, order, mutate):
    """The rows of an all-landmark call with one defect of mutations_obs, from the clean buffers of d (emulate_case)."""
    sig = d["lm"] if mutate.get("corrected") else d["sig0"]
    return emulate_observations(sy.p, d["q"], d["inv"], d["panel"], sig, sy.dim, order, mutate=mutate)
