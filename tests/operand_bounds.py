"""Componentwise rounding-error bounds for the OPERANDS both steps hand to the power series: a long-double reference of
every number linearize_* / prepare_* leave behind and, from the same chain run on absolute values, a bound on
|dev - ref| for EVERY entry (helper module of tests/test_operand_bounds.py and tests/test_gpu_operand_bounds.py; not a test
module).  tests/rounding_bounds.py holds the E0 kernels to such bounds but takes these operands from the context under test
as exact numbers; the normwise tests against the oracle see them only as relative 2-norms over all cameras or landmarks,
which the hub cameras and the well-conditioned landmarks carry.  Conventions as in rounding_bounds.py: LD, gam, first-order
bounds with every gamma rounded up (u = 2^-53; an FMA rounds once, so every count is an upper one; the second-order terms
are covered by rounding every count up and a final factor 1 + 1e-6).

Inputs are only what the caller set: graph, image points, cameras, landmarks, alpha, lambda, robust norm and threshold, eps,
solver type, Jl scaling on or off (Pose / Joint below).  One exception, stated at B^-1.

Weights (both steps).  rounding_bounds.weights / weights_joint give compute_error_weight's weight in long double and rho_i,
the relative error of the device's one, charged wherever the reference's r2 (1 + its own relative error) reaches t^2 (there
the device may also take the other branch, and then the two weights differ by at most that much); no entry is excluded.
Step 1: rho_i bounds w = t / sqrt(r2) recomputed through six roundings of p and its own gamma_4; pose_residual
(povar_kernels.hpp:263-276) forms sb (P0 - u P2) per entry first, seven roundings, and the kernels keep sqrt(w) and square
it again (OpLinearize :781, cm_gram :2473-2477, PrepObs::set :1508): (7/6) rho + 3 u <= 2 rho since rho >= gamma_4.  So the
weight w_i carries 2 rho_i and its square root rho_i.  Step 2: weights_joint's rho is that of sqrt(w) (hom_project's
residual, povar_kernels_joint.hpp:25-35); w = sw sw carries 2 rho.

Step 1 (pOSE).  Per observation i of camera c and landmark l: h = [X_l; 1], (u, v), sb^2 = 1 - alpha, sa^2 = alpha.
  dsb      sb = sqrt(1 - alpha), sa = sqrt(alpha) in fp64 (set_alpha, povar_lm.hip:200-203): the difference and the root,
           gamma_2 each; sb sb: gamma_4 + 1 (cam_finish_linearize :2534, cam_build_binv :2597).
  DIAG2    cm_gram (:2448-2492) sums m_k hh_j, m = w (1, u, v, u^2 + v^2), hh = h_i h_j, into four moments of ten entries;
           cam_finish_linearize (:2505-2538) sums the items in sixteen streams and a fixed-order final sum, and takes
           diag2 = g0_jj (rows 0, 1) or sb^2 g3_jj (row 2).  Every summand is non-negative: the bound is relative.  Per
           summand: u u, v v, their sum, w (4), hh (1), m hh (1); sb sb (5) and its product with g (1): k = 12; the sum in
           any tree gamma_{n_c}.  bound = gamma_{n_c + 12} diag2 + sum_i 2 rho_i summand_i.  No observations: exactly 0.
  SIGMA    1 / (eps + sqrt(diag2)) (:2536): half of diag2's relative error, the root, the sum of two non-negative numbers,
           the division: E(diag2) / (2 diag2) + gamma_3.  diag2 = 0: 1 / eps to gamma_3.
  JL SCALE OpLinearize (:769-803) and lpl_pass<0> (povar_kernels_lpl.hpp:519-528) square the entries of pose_jl (:279-294) with s = 1:
           jl = (sb sw) (P0j - u P2j) 1: the entry a = P0j - u P2j is computed and may cancel, err(a) <= gamma_2 am,
           am = |P0j| + |u| |P2j|; cb = sb sw (dsb + rho + 1), cb a (1): err(jl) <= sb sw (gamma_7 + rho) am =: ejl (rows 2, 3:
           am = |P0j|, fewer roundings).  tot = sum of 4 n_l squares, any order (registers, a segmented scan, wave_sum of
           lm_long): E(tot) = sum 2 |jl| ejl + gamma_{4 n_l + 1} tot; s = 1 / (eps + sqrt(tot)): E(s) = s (E(tot) / (2 tot) +
           gamma_3).  set_jl_col_scaling(False): exactly 1.0.
  HLL_INV  OpPrepare (:808-881) / prepare_lpl (povar_kernels_lpl.hpp:647-743): H = sum of the 4 n_l rows jl_a jl_b with the STORED scale in
           the entry, jl = cb a s_a: err(jl) <= sb sw s_a (gamma_8 + rho + E(s_a) / s_a) am =: ejl (the reference uses its
           own s).  E(H)_ab = sum (|jl_a| ejl_b + |jl_b| ejl_a) + gamma_{4 n_l + 1} sum |jl_a| |jl_b| (+ u (|H_aa| + lambda) for
           POWER_SCHUR_COMPLEMENT's lambda on the diagonal).  inv3 (:209-224) is cofactors over determinant; on absolute
           values E(a b - c d) = |a| E(b) + |b| E(a) + |c| E(d) + |d| E(c) + gamma_2 (|a b| + |c d|), the determinant's three
           terms alike with gamma_3, and E(Hi_ij) = (E(cof_ij) + |Hi_ij| E(det)) / |det| + gamma_2 |Hi_ij| (the reciprocal and
           the product).  The bound scales with each landmark's own cancellation; no condition number appears and no
           landmark is left out.  First order in E(det) / |det|: inv3_bound asserts E(det) < 2^-10 |det| for every landmark
           it is given (edge_problem(0): the largest ratio is recorded in tests/test_operand_bounds.py).
  B        b = sigma sum_i Jp_i^T D^2 (r_i - Jl_i Hi (Jl^T r)_l).  r: pose_residual's seven roundings (PrepObs::set: six),
           sw and dsb: err(r_k) <= (gamma_10 + rho) rm_k, rm_k = sb sw (|P0| + |u| |P2|) . |h| (rows 2, 3: sa sw (|P0| . |h| +
           |u|)).  g = Jl^T r sums 4 n_l products: E(g) = sum (|jl| err(r) + |r| ejl) + gamma_{4 n_l + 1} sum |jl| |r|.
           w = Hi g with the reference's OWN long-double Hi and E(Hi) of the previous item as an operand perturbation (in
           lane-per-landmark mode b is formed from prepare_lpl's own inv3, BUF_HLL_INV from OpPrepare through
           ensure_legacy): E(w) = |Hi| E(g) + E(Hi) |g| + gamma_3 |Hi| |g|.  e = r - Jl w: E(e) = err(r) + |jl| E(w) + ejl |w| +
           gamma_4 (|r| + |jl| |w|).  q = pose_q (:307-314): at most six roundings, dsb and rho: E(q) = (the same positive
           map of E(e)) + (gamma_8 + rho) qm.  Y_c = sum h_j q_m over the camera in any tree (LDS accumulators, partial
           records, the cold view, cam_cold_sum, cm_scatter + cam_sum_items): E(Y) = sum |h_j| E(q_m) + gamma_{n_c + 1} Ym.
           b = sigma Y (:2733, :2856): E(b) = sigma E(Y) + |Y| E(sigma) + u |b|.  No observations: exactly 0.
  B_INV    a right-residual check (a forward bound would need cond(B)).  B_ref = sigma Hpp sigma + lambda I in long
           double from the reference's moments, with the DEVICE's sigma taken as exact -- here and only here: sigma has
           been checked above, and B is defined with the stored sigma.  cam_build_binv (:2588-2616): the moment (k = 6 per
           summand as for DIAG2, gamma_{n_c} for the sum), sb sb and its product (6), two sigmas (2), lambda (1):
           E(B)_ik = sigma_i sigma_k (gamma_{n_c + 15} |moment|_ik + sum 2 rho (its summands)) + u lambda [i = k].
           chol_inverse_16 (:2546-2582) solves L L^T x = e_col per column: by Higham (2nd ed., Thm 10.3 / 10.4) the
           computed column solves (B + dB) x = e_col with |dB| <= gamma_{3 n + 1} |L| |L^T|, and (|L| |L^T|)_ik <=
           sqrt(B_ii B_kk) (Cauchy-Schwarz on the rows of L), so for every entry
               |B_ref X_dev - I|_ij <= sum_k (gamma_{3 n + 1} sqrt(B_ii B_kk) + E(B)_ik) |X_dev|_kj =: R_ij
           Symmetry: X - X^T = B^-1 R' - R'^T B^-1 for the true residual R', so |X - X^T| <= |X| R + (|X| R)^T to first order:
           "twice that bound" carried through |B^-1|.  No observations: B = lambda I and X = I / lambda to gamma_3 (a root
           and two divisions), the off-diagonal entries exactly 0.

Step 2 (RIPOBA; the header of povar_kernels_joint.hpp, rounding_bounds.system_joint is its fp64 restatement).  pc = P X =
(x, y, z) are computed 4-term dots, D = (1/z, -x/z^2, -y/z^2) with the magnitudes A and errors E00, E02, E12 of
rounding_bounds.py (kD = 2: hom_project): a small |z| inflates every bound through err(z) / |z|.
  JL SCALE H  OpLinearizeH (:105-131) / lpl_pass_h<0>: jl_j = sw (D00 P0j + D02 P2j) (hom_jl4 :37-46), magnitude
           jm = sw (A00 |P0j| + A02 |P2j|), err <= sw (E00 |P0j| + E02 |P2j|) + (gamma_4 + rho) jm; tot_j sums 2 n_l squares:
           E(tot) = sum 2 |jl| ejl + gamma_{2 n_l + 1} tot; s as in step 1.
  HLL_INV  Jl3 = Jl4 N_l, Jl4 = jl s with the stored s (one more rounding and E(s) / s), N_l from long-double house4,
           the device's fp64 reflector carried as dN = gamma_25 (rounding_bounds.py): jl3 = jl4[1:] - beta (jl4 . w) w[1:]
           (jl3_of_jl4 :56-63: a 4-term dot, two products, the difference: 7): ejl3 = |N_l|^T ejl4 + (gamma_8 + dN) jl3m
           with jl3m = |N_l|^T |jl4|.  H3 + lambda I, E(H) and inv3 as in step 1 with 2 n_l rows (hinv_damped :149-154).
  DIAG2, SIGMA  cm_gram_h (:457-492): m = w (D00^2, D00 D02, D00 D12, D02^2 + D12^2), hh = X_i X_j; diag2 = g0_jj or g3_jj
           (cam_finish_linearize_h :521-527): non-negative summands, each with the relative error of its own D:
           err(m0) = m0 (2 rho + 2 E00 / A00 + gamma_2), err(m3) = w (2 A02 E02 + 2 A12 E12) + m3 (2 rho + gamma_4), then hh
           and the product (2) and gamma_{n_c} for the sum.  SIGMA as in step 1.
  NC_HOUSEHOLDER  cam_finish_linearize_h (:528-539): nv = sqrt of a 12-term sum of squares (gamma_12 halved, the root:
           gamma_7), w0 = P0 +- nv with equal signs (gamma_8), w[1:] = P[1:] exactly, beta = 2 / w^T w (two w0's, the
           twelve-term sum, the division: gamma_29).  An entry beta w_i w_j of N_c moves by dNc = gamma_45 at most.  Also
           N_c^T vec(P_c) = 0 for the DEVICE's reflector within dNc |N_c|^T |P_c| (evaluated in long double).
  B_JOINT  r = sw (x/z - u, y/z - v) with rounding_bounds.weights_joint's err(x/z); g, w, e as in step 1 with 2 n_l rows;
           q = hom_q (:70-72): E(q0) = sw (A00 E(e0) + E00 |e0|) + (gamma_2 + rho) qm0, q2 alike with gamma_3; Y, sigma as
           in step 1; b11 = N_c^T y12 (nt_apply :589-595: a 12-term dot, two products, the difference: gamma_15) with the
           reference's long-double reflector and dNc: E(b11) = |N_c|^T E(y12) + (gamma_15 + dNc) |N_c|^T |y12|.
  B_INV_JOINT  the residual form above with n = 11 and B_ref = N_c^T (sigma A sigma) N_c + lambda I from the reference's
           moments, its long-double reflector and the device's sigma.  cam_build_binv_h (:545-586): E(sigma A sigma)_ik =
           sigma_i sigma_k (sum of the summands' own errors + gamma_{n_c + 4} |moment|); T = A N and M = N^T T add
           gamma_15 + dNc each on |N_c|^T (sigma |A| sigma) |N_c| (the magnitude Gram): E(B) = |N_c|^T E(sAs) |N_c| +
           2 (gamma_16 + dNc) |N_c|^T (sigma Am sigma) |N_c| + u lambda [i = k].

Slack and the mutation scales measured with these bounds: tests/test_operand_bounds.py's docstring.
"""
import numpy as np

import rounding_bounds as RB
from rounding_bounds import LD, U64, ULD, gam

F = np.float64
FP64 = RB.MODELS["fp64"]


def g(k, u=U64):
    return gam(k, u) if np.ndim(k) else float(gam(k, u))


def _f(a):
    return np.asarray(a).astype(F)


def _ab(a):
    return np.abs(_f(a))


class Pose:
    """A step-1 problem as the caller sets it.  solver: "POWER_VARPROJ" | "POWER_SCHUR_COMPLEMENT" (lambda on the landmark
    blocks); scale_jl: set_jl_col_scaling."""

    def __init__(self, n_cams, lm_off, cam_idx, obs, cams, lms, alpha, lam, robust="NONE", huber=1.0, eps=1e-5,
                 solver="POWER_VARPROJ", scale_jl=True):
        self.n_cams = int(n_cams)
        self.lm_off = np.asarray(lm_off, dtype=np.int64)
        self.cam_idx = np.asarray(cam_idx, dtype=np.int64)
        self.obs = np.asarray(obs, dtype=F).reshape(-1, 2)
        self.cams = np.asarray(cams, dtype=F).reshape(-1, 12)
        self.lms = np.asarray(lms, dtype=F).reshape(len(self.lm_off) - 1, -1)
        self.alpha, self.lam, self.robust, self.huber, self.eps = float(alpha), float(lam), robust, float(huber), float(eps)
        self.solver, self.scale_jl = solver, bool(scale_jl)
        self.n_l = np.diff(self.lm_off)
        assert (self.n_l > 0).all(), "landmarks without observations are out of scope (Hll^-1 is undefined)"
        self.n_lms = len(self.n_l)
        self.n_c = np.bincount(self.cam_idx, minlength=self.n_cams)
        self.lm = np.repeat(np.arange(self.n_lms), self.n_l)
        self.order = np.argsort(self.cam_idx, kind="stable")
        cs = self.cam_idx[self.order]
        self.cst = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]]) if len(cs) else np.zeros(0, dtype=np.int64)
        self.chere = cs[self.cst] if len(cs) else cs

    @property
    def lam_lm(self):
        return self.lam if self.solver == "POWER_SCHUR_COMPLEMENT" else 0.0


class Joint(Pose):
    """A step-2 problem as the caller sets it (lms: homogeneous, [n_lms, 4])."""

    def __init__(self, n_cams, lm_off, cam_idx, obs, cams, lms_h, lam, robust="NONE", huber=1.0, eps=1e-5):
        super().__init__(n_cams, lm_off, cam_idx, obs, cams, lms_h, 0.0, lam, robust, huber, eps)

    @property
    def lam_lm(self):
        return self.lam


def lsum(p, a):
    """Per-landmark sums (the observations are landmark-major) in a's dtype."""
    return np.add.reduceat(a, p.lm_off[:-1], axis=0)


def csum(p, a, keep=None):
    """Per-camera sums in a's dtype (np.bincount would cast to float64); keep: per-observation mask of the summands."""
    out = np.zeros((p.n_cams,) + a.shape[1:], dtype=a.dtype)
    if keep is not None:
        a = np.where(keep.reshape((-1,) + (1,) * (a.ndim - 1)), a, a.dtype.type(0))
    if len(a):
        out[p.chere] = np.add.reduceat(a[p.order], p.cst, axis=0)
    return out


# ---- inv3: cofactors over determinant (povar_kernels.hpp:209-224), entry k of the result = (m[a] m[b] - m[c] m[d]) / det
_COF = [(4, 8, 5, 7), (2, 7, 1, 8), (1, 5, 2, 4), (5, 6, 3, 8), (0, 8, 2, 6), (2, 3, 0, 5), (3, 7, 4, 6), (1, 6, 0, 7), (0, 4, 1, 3)]
DET_RATIO = 2.0 ** -10


def inv3_bound(H, EH, u=U64):
    """(Hi [n, 3, 3] long double, E(Hi) [n, 3, 3], E(det) / |det| [n]) of inv3 applied to H + dH, |dH| <= EH
    (module docstring: HLL_INV).  Asserts the first-order condition E(det) < 2^-10 |det| for every block."""
    m = np.asarray(H, dtype=LD).reshape(-1, 9)
    E = np.asarray(EH, dtype=F).reshape(-1, 9)
    ma = _ab(m)
    g2, g3 = g(2, u), g(3, u)
    cof = np.stack([m[:, a] * m[:, b] - m[:, c] * m[:, d] for a, b, c, d in _COF], 1)
    Ecof = np.stack([ma[:, a] * E[:, b] + ma[:, b] * E[:, a] + ma[:, c] * E[:, d] + ma[:, d] * E[:, c]
                     + g2 * (ma[:, a] * ma[:, b] + ma[:, c] * ma[:, d]) for a, b, c, d in _COF], 1)
    ca = _ab(cof)
    det = cof[:, 0] * m[:, 0] + cof[:, 1] * m[:, 3] + cof[:, 2] * m[:, 6]
    Edet = sum(ca[:, k] * E[:, j] + ma[:, j] * Ecof[:, k] + g3 * ca[:, k] * ma[:, j] for k, j in ((0, 0), (1, 3), (2, 6)))
    da = _ab(det)
    ratio = Edet / da
    assert (ratio < DET_RATIO).all(), ("E(det) / |det| too large for a first-order bound", float(ratio.max()), int(np.argmax(ratio)))
    Hi = cof / det[:, None]
    EHi = (Ecof + _ab(Hi) * Edet[:, None]) / da[:, None] + g2 * _ab(Hi)
    return Hi.reshape(-1, 3, 3), EHi.reshape(-1, 3, 3), ratio


def _scale(tot, Etot, eps, u):
    """1 / (eps + sqrt(tot)) and its bound for tot >= 0 with |d tot| <= Etot (module docstring: SIGMA)."""
    s = 1 / (LD(eps) + np.sqrt(tot))
    tf = _f(tot)
    rel = np.where(tf > 0, Etot / np.where(tf > 0, 2 * tf, 1.0), 0.0) + g(3, u)
    return s, _f(s) * rel


def _mutated_sigma(sig, d2, mutate):
    """The SIGMA reference under the test hooks sigma_no_eps and scale (b and B keep the unmutated one)."""
    if mutate.get("sigma_no_eps"):
        with np.errstate(divide="ignore"):
            sig = 1 / np.sqrt(d2)
    return sig * LD(mutate.get("scale", {}).get("SIGMA", 1))


class Ref:
    """References (long double) and bounds (float64) by operand name: ref["SIGMA"], bound["SIGMA"], ..."""

    def __init__(self):
        self.ref, self.bound, self.aux = {}, {}, {}

    def put(self, name, ref, bound):
        self.ref[name] = np.asarray(ref, dtype=LD)
        self.bound[name] = np.asarray(bound, dtype=F) * (1 + 1e-6)


def _gram_moments(p, m, em, hh, keep, u):
    """(G, Gm, EG) [n_cams, 4, 4, 4]: the moments sum_i m_ik hh_i, their magnitudes, and the summands' own errors em plus
    hh and the product (gamma_2); the sum's gamma is added by the caller."""
    t = m[:, :, None, None] * hh[:, None, :, :]
    ta = _ab(t)
    e = em[:, :, None, None] * _ab(hh)[:, None, :, :] + g(2, u) * ta
    return csum(p, t, keep), csum(p, ta, keep), csum(p, e, keep)


def binv_check(R, name, p, X_dev):
    """(residual [n_cams, n, n], its bound, |X - X^T|, its bound) of the device's inverse blocks against R's B_ref (module
    docstring: B_INV).  X_dev: [n_cams, n, n] row-major as exported."""
    a = R.aux[name]
    n, u = a["n"], a["u"]
    X = np.asarray(X_dev, dtype=F).reshape(-1, n, n)
    Xa = np.abs(X)
    res = _ab(np.einsum("cik,ckj->cij", a["B"], X.astype(LD)) - np.eye(n, dtype=LD)[None])
    d = np.sqrt(_f(np.einsum("cii->ci", a["B"])))
    W = g(3 * n + 1, u) * d[:, :, None] * d[:, None, :] + a["EB"]
    Rb = np.einsum("cik,ckj->cij", W, Xa) * (1 + 1e-6)
    XR = np.einsum("cik,ckj->cij", Xa, Rb)
    return res, Rb, np.abs(X - np.transpose(X, (0, 2, 1))), (XR + np.transpose(XR, (0, 2, 1))) * (1 + 1e-6)


# ======== step 1
def _hpp_pose(G, sb2):
    """[n_cams, 12, 12] from the moments G[c, k, i, j] (cam_build_binv's block pattern, povar_kernels.hpp:2598-2607);
    with magnitudes for G: the same pattern without the signs."""
    nC = G.shape[0]
    H = np.zeros((nC, 3, 4, 3, 4), dtype=G.dtype)
    H[:, 0, :, 0, :] = G[:, 0]
    H[:, 1, :, 1, :] = G[:, 0]
    H[:, 2, :, 2, :] = sb2 * G[:, 3]
    for k in range(2):
        H[:, k, :, 2, :] = -sb2 * G[:, k + 1]
        H[:, 2, :, k, :] = -sb2 * G[:, k + 1]
    return H.reshape(nC, 12, 12)


def pose_operands(p, sigma_dev=None, mutate=None, u=U64):
    """Ref of DIAG2, SIGMA [12 n_cams], JL_COL_SCALE [3 n_lms], HLL_INV [9 n_lms], B [12 n_cams] and, with the device's
    sigma given, the B_INV parts (binv_check).  mutate: test hook (a dict) that perturbs the reference's chain:
      drop_gram: observation indices left out of the Gram moments      w_one: observation indices whose weight is taken as 1
      sigma_no_eps: True                                               drop_b: observation indices left out of b
      scale: {operand name: factor} applied to that reference          entry: {operand name: (flat index, factor)}
      lam_missing: (camera, diagonal index) of B without lambda."""
    mutate = mutate or {}
    model = FP64 if u == U64 else RB.MODELS["longdouble"]
    R = Ref()
    c, lm = p.cam_idx, p.lm
    n = len(c)
    sb2, sa2 = LD(1) - LD(p.alpha), LD(p.alpha)
    sb, sa = np.sqrt(sb2), np.sqrt(sa2)
    fsb, fsa = float(sb), float(sa)
    P, X, uv = p.cams[c].astype(LD), p.lms[lm].astype(LD), p.obs.astype(LD)
    Pa, Xa = np.abs(p.cams[c]), np.abs(p.lms[lm])
    U, V = uv[:, 0], uv[:, 1]
    Ua, Va = np.abs(p.obs[:, 0]), np.abs(p.obs[:, 1])
    hx = [X[:, 0], X[:, 1], X[:, 2]]
    w, rho = RB.weights(p, P, hx, uv, sb2, sa2, model)
    if "w_one" in mutate:
        w = w.copy()
        w[np.asarray(mutate["w_one"])] = 1
    sw, swa = np.sqrt(w), _f(np.sqrt(w))
    R.aux["w"] = _f(w)
    h = np.concatenate([X, np.ones((n, 1), dtype=LD)], 1)
    ha = np.concatenate([Xa, np.ones((n, 1))], 1)
    # ---- Gram moments, DIAG2, SIGMA
    m = w[:, None] * np.stack([np.ones(n, dtype=LD), U, V, U * U + V * V], 1)
    em = (2 * rho[:, None] + g(4, u)) * _ab(m)
    keep = None
    if "drop_gram" in mutate:
        keep = np.ones(n, dtype=bool)
        keep[np.asarray(mutate["drop_gram"])] = False
    G, Gm, EG = _gram_moments(p, m, em, h[:, :, None] * h[:, None, :], keep, u)
    dj = np.arange(4)
    d2 = np.concatenate([G[:, 0, dj, dj], G[:, 0, dj, dj], sb2 * G[:, 3, dj, dj]], 1)
    Ed2 = np.concatenate([EG[:, 0, dj, dj], EG[:, 0, dj, dj], fsb ** 2 * EG[:, 3, dj, dj]], 1) + g(p.n_c + 6, u)[:, None] * _f(d2)
    d2 = d2 * LD(mutate.get("scale", {}).get("DIAG2", 1))
    R.put("DIAG2", d2.reshape(-1), Ed2.reshape(-1))
    sig, Esig = _scale(d2, Ed2, p.eps, u)
    R.put("SIGMA", _mutated_sigma(sig, d2, mutate).reshape(-1), Esig.reshape(-1))
    # ---- the Jl rows without the column scale: a = P0j - u P2j (rows 0, 1), P0j (rows 2, 3)
    P3 = [P[:, 4 * k:4 * k + 3] for k in range(3)]
    P3a = [Pa[:, 4 * k:4 * k + 3] for k in range(3)]
    rows = [sb * sw[:, None] * (P3[0] - U[:, None] * P3[2]), sb * sw[:, None] * (P3[1] - V[:, None] * P3[2]),
            sa * sw[:, None] * P3[0], sa * sw[:, None] * P3[1]]
    am = [fsb * swa[:, None] * (P3a[0] + Ua[:, None] * P3a[2]), fsb * swa[:, None] * (P3a[1] + Va[:, None] * P3a[2]),
          fsa * swa[:, None] * P3a[0], fsa * swa[:, None] * P3a[1]]
    nl4 = 4 * p.n_l
    if p.scale_jl:
        tot = lsum(p, sum(r * r for r in rows))
        Etot = lsum(p, sum(2 * _ab(r) * (g(7, u) + rho)[:, None] * a for r, a in zip(rows, am))) + g(nl4 + 1, u)[:, None] * _f(tot)
        s, Es = _scale(tot, Etot, p.eps, u)
        s = s * LD(mutate.get("scale", {}).get("JL_COL_SCALE", 1))
    else:
        s, Es = np.ones((p.n_lms, 3), dtype=LD), np.zeros((p.n_lms, 3))
    R.put("JL_COL_SCALE", s.reshape(-1), Es.reshape(-1))
    # ---- HLL_INV
    sl, sla = s[lm], _f(s)[lm]
    ds = (Es / _f(s))[lm]
    jl = [r * sl for r in rows]
    jla = [_ab(r) for r in jl]
    ejl = [a * sla * (g(8, u) + rho[:, None] + ds) for a in am]
    H = lsum(p, sum(r[:, :, None] * r[:, None, :] for r in jl))
    Hm = lsum(p, sum(r[:, :, None] * r[:, None, :] for r in jla))
    EH = lsum(p, sum(r[:, :, None] * e[:, None, :] + e[:, :, None] * r[:, None, :] for r, e in zip(jla, ejl))) + g(nl4 + 1, u)[:, None, None] * Hm
    if p.lam_lm:
        H = H + LD(p.lam_lm) * np.eye(3, dtype=LD)[None]
        EH = EH + u * (Hm + p.lam_lm) * np.eye(3)[None]
    Hi, EHi, ratio = inv3_bound(H, EH, u)
    R.aux["det_ratio"], R.aux["H"] = ratio, H
    Hi_b = Hi
    if "entry" in mutate and "HLL_INV" in mutate["entry"]:
        i, fac = mutate["entry"]["HLL_INV"]
        Hi = Hi.copy()
        Hi.reshape(-1)[i] *= LD(fac)
    R.put("HLL_INV", Hi.reshape(-1), EHi.reshape(-1))
    # ---- B
    Pm = [Pa[:, 4 * k] * Xa[:, 0] + Pa[:, 4 * k + 1] * Xa[:, 1] + Pa[:, 4 * k + 2] * Xa[:, 2] + Pa[:, 4 * k + 3] for k in range(3)]
    pk = [P[:, 4 * k] * X[:, 0] + P[:, 4 * k + 1] * X[:, 1] + P[:, 4 * k + 2] * X[:, 2] + P[:, 4 * k + 3] for k in range(3)]
    r = [sb * sw * (pk[0] - U * pk[2]), sb * sw * (pk[1] - V * pk[2]), sa * sw * (pk[0] - U), sa * sw * (pk[1] - V)]
    rm = [fsb * swa * (Pm[0] + Ua * Pm[2]), fsb * swa * (Pm[1] + Va * Pm[2]), fsa * swa * (Pm[0] + Ua), fsa * swa * (Pm[1] + Va)]
    Er = [(g(10, u) + rho) * t for t in rm]
    ra = [_ab(t) for t in r]
    gl = lsum(p, sum(j * t[:, None] for j, t in zip(jl, r)))
    gm = lsum(p, sum(j * t[:, None] for j, t in zip(jla, ra)))
    Eg = lsum(p, sum(j * e[:, None] + ej * t[:, None] for j, e, ej, t in zip(jla, Er, ejl, ra))) + g(nl4 + 1, u)[:, None] * gm
    Hia, ga = _ab(Hi_b), _ab(gl)
    w3 = np.einsum("lab,lb->la", Hi_b, gl)
    w3m = np.einsum("lab,lb->la", Hia, ga)
    Ew3 = np.einsum("lab,lb->la", Hia, Eg) + np.einsum("lab,lb->la", EHi, ga) + g(3, u) * w3m
    w3o, w3a, Ew3o = w3[lm], _ab(w3)[lm], Ew3[lm]
    e = [t - (j * w3o).sum(1) for t, j in zip(r, jl)]
    Ee = [er + (j * Ew3o).sum(1) + (ej * w3a).sum(1) + g(4, u) * (t + (j * w3a).sum(1)) for er, j, ej, t in zip(Er, jla, ejl, ra)]
    ea = [_ab(t) for t in e]
    q = [sw * (sb * e[0] + sa * e[2]), sw * (sb * e[1] + sa * e[3]), -sw * sb * (U * e[0] + V * e[1])]
    qmap = lambda v: [swa * (fsb * v[0] + fsa * v[2]), swa * (fsb * v[1] + fsa * v[3]), swa * fsb * (Ua * v[0] + Va * v[1])]
    qm, Eq = qmap(ea), qmap(Ee)
    Eq = [a + (g(8, u) + rho) * b for a, b in zip(Eq, qm)]
    keep_b = None
    if "drop_b" in mutate:
        keep_b = np.ones(n, dtype=bool)
        keep_b[np.asarray(mutate["drop_b"])] = False
    Y = csum(p, np.stack([q[mm] * h[:, j] for mm in range(3) for j in range(4)], 1), keep_b)
    Ym = csum(p, np.stack([qm[mm] * ha[:, j] for mm in range(3) for j in range(4)], 1))
    EY = csum(p, np.stack([Eq[mm] * ha[:, j] for mm in range(3) for j in range(4)], 1)) + g(p.n_c + 1, u)[:, None] * Ym
    R.aux["Y"], R.aux["EY"] = Y, EY * (1 + 1e-6)
    b = sig * Y
    if "entry" in mutate and "B" in mutate["entry"]:
        i, fac = mutate["entry"]["B"]
        b = b.copy()
        b.reshape(-1)[i] *= LD(fac)
    R.put("B", b.reshape(-1), (_f(sig) * EY + _ab(Y) * Esig + u * _ab(b)).reshape(-1))
    # (the chain's own numbers, for tests/sc_bounds.py: per observation w, rho; per landmark s, Hi; per camera sigma, moments)
    R.aux["chain"] = dict(w=w, rho=rho, s=s, Es=Es, Hi=Hi_b, EHi=EHi, sig=sig, Esig=Esig, G=G, Gm=Gm, EG=EG, sb2=sb2)
    # ---- B_INV parts: B_ref with the device's sigma
    if sigma_dev is not None:
        sd = np.asarray(sigma_dev, dtype=F).reshape(-1, 12)
        Hpp = _hpp_pose(G, sb2)
        Hm_ = np.abs(_hpp_pose(Gm, fsb ** 2))
        EHp = np.abs(_hpp_pose(EG, fsb ** 2))
        ss = sd[:, :, None] * sd[:, None, :]
        B = sd.astype(LD)[:, :, None] * Hpp * sd.astype(LD)[:, None, :] + LD(p.lam) * np.eye(12, dtype=LD)[None]
        if "lam_missing" in mutate:
            cc, k = mutate["lam_missing"]
            B[cc, k, k] -= LD(p.lam)
        EB = ss * (EHp + g(p.n_c + 9, u)[:, None, None] * Hm_) + u * p.lam * np.eye(12)[None]
        R.aux["B_INV"] = dict(B=B, EB=EB * (1 + 1e-6), n=12, u=u)
    return R


# ======== step 2
def house12(Pc):
    """(w [n, 12], beta [n]) of cam_finish_linearize_h's reflector (povar_kernels_joint.hpp:528-539) in Pc's dtype."""
    nv = np.sqrt((Pc * Pc).sum(1))
    w = Pc.copy()
    w[:, 0] = Pc[:, 0] + np.where(Pc[:, 0] >= 0, nv, -nv)
    return w, 2 / (w * w).sum(1)


def _nt12(w, b, a, sign=-1):
    """N_c^T a = a[1:] - beta (w . a) w[1:] per camera (sign = +1 with |w|: the map |N_c|^T)."""
    return a[:, 1:] + sign * (b * (w * a).sum(1))[:, None] * w[:, 1:]


def _ntan(w, b, A, sign=-1):
    """N_c^T A N_c per camera for A [n, 12, 12] (sign = +1 with |w|, |A|: the magnitude map)."""
    T = A[:, :, 1:] + sign * (b[:, None] * np.einsum("cik,ck->ci", A, w))[:, :, None] * w[:, None, 1:]
    return T[:, 1:, :] + sign * (b[:, None] * np.einsum("ck,ckj->cj", w, T))[:, None, :] * w[:, 1:, None]


def joint_operands(p, sigma_dev=None, mutate=None, u=U64):
    """Ref of DIAG2, SIGMA [12 n_cams], JL_COL_SCALE_H [4 n_lms], HLL_INV [9 n_lms], NC_HOUSEHOLDER [13 n_cams], B_JOINT
    [11 n_cams] and, with the device's sigma given, the B_INV_JOINT parts.  mutate: as pose_operands, plus
      beta_double: camera indices whose reflector's beta is doubled."""
    mutate = mutate or {}
    R = Ref()
    c, lm = p.cam_idx, p.lm
    n = len(c)
    g2, g3, g4 = (g(k, u) for k in (2, 3, 4))
    P, X = p.cams[c].astype(LD), p.lms[lm].astype(LD)
    Pa, Xa = np.abs(p.cams[c]), np.abs(p.lms[lm])
    Pr, Par = [P[:, 4 * r:4 * r + 4] for r in range(3)], [Pa[:, 4 * r:4 * r + 4] for r in range(3)]
    px, py, pz = ((Pr[r] * X).sum(1) for r in range(3))
    xm, ym, zm = ((Par[r] * Xa).sum(1) for r in range(3))
    az = _ab(pz)
    ezr = g4 * zm / az
    D = [1 / pz, -px / (pz * pz), -py / (pz * pz)]
    A = [1 / az, _ab(px) / az ** 2, _ab(py) / az ** 2]
    E = [A[0] * (ezr + u), A[1] * (2 * ezr + 2 * u) + g4 * xm / az ** 2, A[2] * (2 * ezr + 2 * u) + g4 * ym / az ** 2]
    sw, rho = RB.weights_joint(p, px, py, pz, xm, ym, zm, u)
    if "w_one" in mutate:
        sw = sw.copy()
        sw[np.asarray(mutate["w_one"])] = 1
    swa = _f(sw)
    w, wa = sw * sw, swa * swa
    R.aux["w"] = wa
    # ---- Gram moments, DIAG2, SIGMA
    m = w[:, None] * np.stack([D[0] * D[0], D[0] * D[1], D[0] * D[2], D[1] * D[1] + D[2] * D[2]], 1)
    ma = _ab(m)
    rD0 = ezr + u
    em = np.stack([ma[:, 0] * (2 * rho + 2 * rD0 + g2), wa * A[0] * E[1] + ma[:, 1] * (2 * rho + rD0 + g2),
                   wa * A[0] * E[2] + ma[:, 2] * (2 * rho + rD0 + g2), wa * 2 * (A[1] * E[1] + A[2] * E[2]) + ma[:, 3] * (2 * rho + g4)], 1)
    keep = None
    if "drop_gram" in mutate:
        keep = np.ones(n, dtype=bool)
        keep[np.asarray(mutate["drop_gram"])] = False
    G, Gm, EG = _gram_moments(p, m, em, X[:, :, None] * X[:, None, :], keep, u)
    dj = np.arange(4)
    d2 = np.concatenate([G[:, 0, dj, dj], G[:, 0, dj, dj], G[:, 3, dj, dj]], 1)
    Ed2 = np.concatenate([EG[:, 0, dj, dj], EG[:, 0, dj, dj], EG[:, 3, dj, dj]], 1) + g(p.n_c, u)[:, None] * _f(d2)
    d2 = d2 * LD(mutate.get("scale", {}).get("DIAG2", 1))
    R.put("DIAG2", d2.reshape(-1), Ed2.reshape(-1))
    sig, Esig = _scale(d2, Ed2, p.eps, u)
    R.put("SIGMA", _mutated_sigma(sig, d2, mutate).reshape(-1), Esig.reshape(-1))
    # ---- Jl4 rows without the column scale, JL_COL_SCALE_H
    rows = [sw[:, None] * (D[0][:, None] * Pr[k] + D[k + 1][:, None] * Pr[2]) for k in range(2)]
    jm = [swa[:, None] * (A[0][:, None] * Par[k] + A[k + 1][:, None] * Par[2]) for k in range(2)]
    ej = [swa[:, None] * (E[0][:, None] * Par[k] + E[k + 1][:, None] * Par[2]) + (g4 + rho)[:, None] * jm[k] for k in range(2)]
    nl2 = 2 * p.n_l
    tot = lsum(p, sum(r * r for r in rows))
    Etot = lsum(p, sum(2 * _ab(r) * e for r, e in zip(rows, ej))) + g(nl2 + 1, u)[:, None] * _f(tot)
    s, Es = _scale(tot, Etot, p.eps, u)
    s = s * LD(mutate.get("scale", {}).get("JL_COL_SCALE_H", 1))
    R.put("JL_COL_SCALE_H", s.reshape(-1), Es.reshape(-1))
    # ---- HLL_INV of H3 + lambda I
    lw, lb = RB.house4(p.lms.astype(LD))
    lwa, lba = _ab(lw)[lm], _f(lb)[lm]
    lwo, lbo = lw[lm], lb[lm]
    dn = g(25, u)
    sl, sla = s[lm], _f(s)[lm]
    ds = (Es / _f(s))[lm]
    jl4 = [r * sl for r in rows]
    ej4 = [e * sla + (ds + u) * _ab(j) for e, j in zip(ej, jl4)]
    jl3 = [RB._nt(lwo, lbo, j) for j in jl4]
    jl3m = [RB._nt(lwa, lba, _ab(j), +1) for j in jl4]
    ejl3 = [RB._nt(lwa, lba, e, +1) + (g(8, u) + dn) * jm3 for e, jm3 in zip(ej4, jl3m)]
    jl3a = [_ab(j) for j in jl3]
    H = lsum(p, sum(r[:, :, None] * r[:, None, :] for r in jl3))
    Hm = lsum(p, sum(r[:, :, None] * r[:, None, :] for r in jl3a))
    EH = lsum(p, sum(r[:, :, None] * e[:, None, :] + e[:, :, None] * r[:, None, :] for r, e in zip(jl3a, ejl3))) + g(nl2 + 1, u)[:, None, None] * Hm
    H = H + LD(p.lam_lm) * np.eye(3, dtype=LD)[None]
    EH = EH + u * (Hm + p.lam_lm) * np.eye(3)[None]
    Hi, EHi, ratio = inv3_bound(H, EH, u)
    R.aux["det_ratio"], R.aux["H"] = ratio, H
    Hi_b = Hi
    if "entry" in mutate and "HLL_INV" in mutate["entry"]:
        i, fac = mutate["entry"]["HLL_INV"]
        Hi = Hi.copy()
        Hi.reshape(-1)[i] *= LD(fac)
    R.put("HLL_INV", Hi.reshape(-1), EHi.reshape(-1))
    # ---- NC_HOUSEHOLDER
    cw, cb = house12(p.cams.astype(LD))
    if "beta_double" in mutate:
        cb = cb.copy()
        cb[np.asarray(mutate["beta_double"])] *= 2
    cwa, cba = _ab(cw), _f(cb)
    Ecw = np.zeros((p.n_cams, 12))
    Ecw[:, 0] = g(8, u) * cwa[:, 0]
    R.put("NC_HOUSEHOLDER", np.concatenate([cw, cb[:, None]], 1).reshape(-1), np.concatenate([Ecw, (g(29, u) * cba)[:, None]], 1).reshape(-1))
    dnc = g(45, u)
    R.aux["dnc"] = dnc
    # ---- B_JOINT
    uvL = p.obs.astype(LD)
    qx, qy = px / pz, py / pz
    r = [sw * (qx - uvL[:, 0]), sw * (qy - uvL[:, 1])]
    e0 = [g4 * xm / az + _ab(qx) * (ezr + 2 * u) + u * np.abs(p.obs[:, 0]), g4 * ym / az + _ab(qy) * (ezr + 2 * u) + u * np.abs(p.obs[:, 1])]
    ra = [_ab(t) for t in r]
    Er = [swa * e + (rho + u) * t for e, t in zip(e0, ra)]
    gl = lsum(p, sum(j * t[:, None] for j, t in zip(jl3, r)))
    gm = lsum(p, sum(j * t[:, None] for j, t in zip(jl3a, ra)))
    Eg = lsum(p, sum(j * e[:, None] + ej_ * t[:, None] for j, e, ej_, t in zip(jl3a, Er, ejl3, ra))) + g(nl2 + 1, u)[:, None] * gm
    Hia, ga = _ab(Hi_b), _ab(gl)
    w3 = np.einsum("lab,lb->la", Hi_b, gl)
    w3m = np.einsum("lab,lb->la", Hia, ga)
    Ew3 = np.einsum("lab,lb->la", Hia, Eg) + np.einsum("lab,lb->la", EHi, ga) + g3 * w3m
    w3o, w3a, Ew3o = w3[lm], _ab(w3)[lm], Ew3[lm]
    e = [t - (j * w3o).sum(1) for t, j in zip(r, jl3)]
    Ee = [er + (j * Ew3o).sum(1) + (ej_ * w3a).sum(1) + g4 * (t + (j * w3a).sum(1)) for er, j, ej_, t in zip(Er, jl3a, ejl3, ra)]
    ea = [_ab(t) for t in e]
    q = [sw * D[0] * e[0], sw * D[0] * e[1], sw * (D[1] * e[0] + D[2] * e[1])]
    qm = [swa * A[0] * ea[0], swa * A[0] * ea[1], swa * (A[1] * ea[0] + A[2] * ea[1])]
    Eq = [swa * (A[0] * Ee[0] + E[0] * ea[0]) + (g2 + rho) * qm[0], swa * (A[0] * Ee[1] + E[0] * ea[1]) + (g2 + rho) * qm[1],
          swa * (A[1] * Ee[0] + A[2] * Ee[1] + E[1] * ea[0] + E[2] * ea[1]) + (g3 + rho) * qm[2]]
    keep_b = None
    if "drop_b" in mutate:
        keep_b = np.ones(n, dtype=bool)
        keep_b[np.asarray(mutate["drop_b"])] = False
    Y = csum(p, np.stack([q[mm] * X[:, j] for mm in range(3) for j in range(4)], 1), keep_b)
    Ym = csum(p, np.stack([qm[mm] * Xa[:, j] for mm in range(3) for j in range(4)], 1))
    EY = csum(p, np.stack([Eq[mm] * Xa[:, j] for mm in range(3) for j in range(4)], 1)) + g(p.n_c + 1, u)[:, None] * Ym
    y12 = sig * Y
    Ey12 = _f(sig) * EY + _ab(Y) * Esig + u * _ab(y12)
    b11 = _nt12(cw, cb, y12)
    b11m = _nt12(cwa, cba, _ab(y12), +1)
    if "entry" in mutate and "B_JOINT" in mutate["entry"]:
        i, fac = mutate["entry"]["B_JOINT"]
        b11 = b11.copy()
        b11.reshape(-1)[i] *= LD(fac)
    R.put("B_JOINT", b11.reshape(-1), (_nt12(cwa, cba, Ey12, +1) + (g(15, u) + dnc) * b11m).reshape(-1))
    # (the chain's own numbers, for tests/sc_bounds.py)
    R.aux["chain"] = dict(sw=sw, rho=rho, D=D, A=A, E=E, jl3=jl3, jl3a=jl3a, ejl3=ejl3, Hi=Hi_b, EHi=EHi, sig=sig, Esig=Esig,
                          G=G, Gm=Gm, EG=EG, cw=cw, cb=cb)
    # ---- B_INV_JOINT parts
    if sigma_dev is not None:
        sd = np.asarray(sigma_dev, dtype=F).reshape(-1, 12)

        def hpp(Gx):
            nC = Gx.shape[0]
            Hh = np.zeros((nC, 3, 4, 3, 4), dtype=Gx.dtype)
            Hh[:, 0, :, 0, :] = Gx[:, 0]
            Hh[:, 1, :, 1, :] = Gx[:, 0]
            Hh[:, 2, :, 2, :] = Gx[:, 3]
            for k in range(2):
                Hh[:, k, :, 2, :] = Gx[:, k + 1]
                Hh[:, 2, :, k, :] = Gx[:, k + 1]
            return Hh.reshape(nC, 12, 12)
        ss = sd[:, :, None] * sd[:, None, :]
        SAS = sd.astype(LD)[:, :, None] * hpp(G) * sd.astype(LD)[:, None, :]
        SASm = ss * hpp(Gm)
        ESAS = ss * (hpp(EG) + g(p.n_c + 4, u)[:, None, None] * hpp(Gm))
        B = _ntan(cw, cb, SAS) + LD(p.lam) * np.eye(11, dtype=LD)[None]
        if "lam_missing" in mutate:
            cc, k = mutate["lam_missing"]
            B[cc, k, k] -= LD(p.lam)
        EB = _ntan(cwa, cba, ESAS, +1) + 2 * (g(16, u) + dnc) * _ntan(cwa, cba, SASm, +1) + u * p.lam * np.eye(11)[None]
        R.aux["B_INV_JOINT"] = dict(B=B, EB=EB * (1 + 1e-6), n=11, u=u)
    return R


def nc_nullspace(R, p, ncw_dev):
    """(|N_dev^T vec(P)| [n_cams, 11], its bound) for the device's reflectors (module docstring: NC_HOUSEHOLDER)."""
    d = np.asarray(ncw_dev, dtype=F).reshape(-1, 13)
    Pc = p.cams.astype(LD)
    v = _nt12(d[:, :12].astype(LD), d[:, 12].astype(LD), Pc)
    return _ab(v), R.aux["dnc"] * _nt12(np.abs(d[:, :12]), d[:, 12], np.abs(p.cams), +1) * (1 + 1e-6)


def report(name, per, dev, ref, bound, counts):
    """One line about the worst entry of an operand: its camera or landmark (per entries each), that one's observation
    count and err / bound, in the manner of rounding_bounds.check."""
    r, i, over = RB.check(np.asarray(dev).reshape(-1), np.asarray(ref).reshape(-1), np.asarray(bound).reshape(-1))
    k = i // per
    return r, over, f"{name}: worst entry {i % per} of block {k} (n_obs={int(counts[k])}) err/bound={r:.3g} over={over}"


# ======== fp64 NumPy emulations in the kernels' operation order (test_operand_bounds.py)
def chol_inverse(A):
    """chol_inverse_16 (povar_kernels.hpp:2546-2582) for A [n_cams, n, n] in fp64: the same operation order, every product
    rounded (NumPy does not contract to FMAs)."""
    A = np.array(A, dtype=F)
    nC, n, _ = A.shape
    L = np.zeros_like(A)
    for j in range(n):
        dd = A[:, j, j].copy()
        for k in range(j):
            dd = dd - L[:, j, k] * L[:, j, k]
        L[:, j, j] = np.sqrt(dd)
        for l in range(j + 1, n):
            sv = A[:, j, l].copy()
            for k in range(j):
                sv = sv - L[:, l, k] * L[:, j, k]
            L[:, l, j] = sv / L[:, j, j]
    X = np.zeros_like(A)
    for col in range(n):
        x = np.zeros((nC, n))
        for i in range(n):
            sv = np.full(nC, 1.0 if i == col else 0.0)
            for k in range(i):
                sv = sv - L[:, i, k] * x[:, k]
            x[:, i] = sv / L[:, i, i]
        for i in range(n - 1, -1, -1):
            sv = x[:, i].copy()
            for k in range(i + 1, n):
                sv = sv - L[:, k, i] * x[:, k]
            x[:, i] = sv / L[:, i, i]
        X[:, :, col] = x
    return X


def _inv3_f(m):
    cof = np.stack([m[:, a] * m[:, b] - m[:, c] * m[:, d] for a, b, c, d in _COF], 1)
    det = cof[:, 0] * m[:, 0] + cof[:, 1] * m[:, 3] + cof[:, 2] * m[:, 6]
    return cof * (1.0 / det)[:, None]


def _add_at(n, idx, a):
    out = np.zeros((n,) + a.shape[1:])
    np.add.at(out, idx, a)  # (row order, one rounding per add)
    return out


def emulate_pose(p, form):
    """Every step-1 operand in fp64.  form "obs": OpLinearize / OpPrepare (pose_residual, pose_jl, the stored sqrt(w));
    "lpl": lpl_pass<0> / prepare_lpl (PrepObs::set rebuilds the row from P - P2 u and the translation column; cm_gram in
    gather mode recomputes the weight).  Sums in row order."""
    c, lm = p.cam_idx, p.lm
    n = len(c)
    sa, sb = np.sqrt(p.alpha), np.sqrt(1.0 - p.alpha)
    P, X, U, V = p.cams[c], p.lms[lm], p.obs[:, 0], p.obs[:, 1]
    h = np.concatenate([X, np.ones((n, 1))], 1)
    Pr = [P[:, 4 * k:4 * k + 4] for k in range(3)]
    m0, m1 = sb * (Pr[0] - Pr[2] * U[:, None]), sb * (Pr[1] - Pr[2] * V[:, None])
    res = [RB._dot(m0, h), RB._dot(m1, h), RB._dot(sa * Pr[0], h) - sa * U, RB._dot(sa * Pr[1], h) - sa * V]
    r2 = res[0] * res[0] + res[1] * res[1] + res[2] * res[2] + res[3] * res[3]
    w = np.where(r2 < p.huber * p.huber, 1.0, p.huber / np.sqrt(r2)) if p.robust == "HUBER" else np.ones(n)
    sw = np.sqrt(w)
    out = {}
    # cm_gram, cam_finish_linearize
    ww = sw * sw
    m = np.stack([ww, ww * U, ww * V, ww * (U * U + V * V)], 1)
    G = _add_at(p.n_cams, c, m[:, :, None, None] * (h[:, :, None] * h[:, None, :])[:, None])
    dj = np.arange(4)
    sb2 = sb * sb
    d2 = np.concatenate([G[:, 0, dj, dj], G[:, 0, dj, dj], sb2 * G[:, 3, dj, dj]], 1)
    sig = 1.0 / (p.eps + np.sqrt(d2))
    out["DIAG2"], out["SIGMA"] = d2.reshape(-1), sig.reshape(-1)
    # the Jl column scale (pose_jl with s = 1)
    cb, ca = sb * sw, sa * sw

    def jl_rows(s):
        return [cb[:, None] * (Pr[0][:, :3] - Pr[2][:, :3] * U[:, None]) * s, cb[:, None] * (Pr[1][:, :3] - Pr[2][:, :3] * V[:, None]) * s,
                ca[:, None] * Pr[0][:, :3] * s, ca[:, None] * Pr[1][:, :3] * s]
    if p.scale_jl:
        r1 = jl_rows(np.ones((n, 3)))
        s = 1.0 / (p.eps + np.sqrt(_add_at(p.n_lms, lm, r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2] + r1[3] * r1[3])))
    else:
        s = np.ones((p.n_lms, 3))
    out["JL_COL_SCALE"] = s.reshape(-1)
    if form == "obs":
        jl = jl_rows(s[lm])
        rr = [sw * t for t in res]
    else:
        a0, a1 = Pr[0][:, :3] - Pr[2][:, :3] * U[:, None], Pr[1][:, :3] - Pr[2][:, :3] * V[:, None]
        t0, t1 = Pr[0][:, 3] - Pr[2][:, 3] * U, Pr[1][:, 3] - Pr[2][:, 3] * V
        rr = [cb * (RB._dot(a0, X) + t0), cb * (RB._dot(a1, X) + t1),
              ca * (RB._dot(Pr[0][:, :3], X) + Pr[0][:, 3] - U), ca * (RB._dot(Pr[1][:, :3], X) + Pr[1][:, 3] - V)]
        sl = s[lm]
        jl = [cb[:, None] * a0 * sl, cb[:, None] * a1 * sl, ca[:, None] * Pr[0][:, :3] * sl, ca[:, None] * Pr[1][:, :3] * sl]
    idx = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    red = np.zeros((n, 9))
    for k in range(4):
        for t, (a, b) in enumerate(idx):
            red[:, t] = red[:, t] + jl[k][:, a] * jl[k][:, b]
        for a in range(3):
            red[:, 6 + a] = red[:, 6 + a] + jl[k][:, a] * rr[k]
    tot = _add_at(p.n_lms, lm, red)
    Hm = np.stack([tot[:, 0], tot[:, 1], tot[:, 2], tot[:, 1], tot[:, 3], tot[:, 4], tot[:, 2], tot[:, 4], tot[:, 5]], 1)
    Hm[:, [0, 4, 8]] += p.lam_lm
    Hi = _inv3_f(Hm)
    out["HLL_INV"] = Hi.reshape(-1)
    w3 = np.stack([Hi[:, 3 * a] * tot[:, 6] + Hi[:, 3 * a + 1] * tot[:, 7] + Hi[:, 3 * a + 2] * tot[:, 8] for a in range(3)], 1)[lm]
    e = [rr[k] - (jl[k][:, 0] * w3[:, 0] + jl[k][:, 1] * w3[:, 1] + jl[k][:, 2] * w3[:, 2]) for k in range(4)]
    q = [sw * (sb * e[0] + sa * e[2]), sw * (sb * e[1] + sa * e[3]), -sw * sb * (U * e[0] + V * e[1])]
    Y = _add_at(p.n_cams, c, np.stack([h[:, j] * q[mm] for mm in range(3) for j in range(4)], 1))
    out["B"] = (Y * sig).reshape(-1)
    # cam_build_binv
    Hpp = _hpp_pose(G, sb2)
    A = Hpp * sig[:, :, None] * sig[:, None, :]
    A[:, np.arange(12), np.arange(12)] += p.lam
    out["B_INV"] = chol_inverse(A).reshape(-1)
    out["_B"] = A
    return out


def emulate_joint(p):
    """Every step-2 operand in fp64 in the kernels' operation order.  One form: OpLinearizeH / OpPrepareH and lpl_pass_h<0> /
    prepare_lpl_h share hom_project, hom_jl4, house4, jl3_of_jl4 and hom_q, and sqrt(w) of the stored weight
    (prepare_lpl_h povar_kernels_lpl.hpp:780, cm_gram_h :473-477) is the per-observation kernels' stored sqrt(w) bit for bit; only the order
    of the sums differs, which the bounds leave free.  Sums in row order."""
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
    out = {}
    ww = sw * sw
    m = np.stack([ww * D00 * D00, ww * D00 * D02, ww * D00 * D12, ww * (D02 * D02 + D12 * D12)], 1)
    G = _add_at(p.n_cams, c, m[:, :, None, None] * (X[:, :, None] * X[:, None, :])[:, None])
    dj = np.arange(4)
    d2 = np.concatenate([G[:, 0, dj, dj], G[:, 0, dj, dj], G[:, 3, dj, dj]], 1)
    sig = 1.0 / (p.eps + np.sqrt(d2))
    out["DIAG2"], out["SIGMA"] = d2.reshape(-1), sig.reshape(-1)
    Pc = p.cams
    nv = np.zeros(p.n_cams)
    for k in range(12):
        nv = nv + Pc[:, k] * Pc[:, k]
    nv = np.sqrt(nv)
    cw = Pc.copy()
    cw[:, 0] = Pc[:, 0] + np.where(Pc[:, 0] >= 0, nv, -nv)
    wtw = np.zeros(p.n_cams)
    for k in range(12):
        wtw = wtw + cw[:, k] * cw[:, k]
    cb = 2.0 / wtw
    out["NC_HOUSEHOLDER"] = np.concatenate([cw, cb[:, None]], 1).reshape(-1)

    def jl4_rows(s):
        return [sw[:, None] * (D00[:, None] * Pr[0] + D02[:, None] * Pr[2]) * s, sw[:, None] * (D00[:, None] * Pr[1] + D12[:, None] * Pr[2]) * s]
    j1 = jl4_rows(np.ones((n, 4)))
    s = 1.0 / (p.eps + np.sqrt(_add_at(p.n_lms, lm, j1[0] * j1[0] + j1[1] * j1[1])))
    out["JL_COL_SCALE_H"] = s.reshape(-1)
    lw, lb = RB.house4(p.lms)
    wl, bl = lw[lm], lb[lm]
    jl4 = jl4_rows(s[lm])
    jl3 = [j[:, 1:] - (bl * RB._dot(j, wl))[:, None] * wl[:, 1:] for j in jl4]
    rr = [sw * r0, sw * r1]
    idx = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    red = np.zeros((n, 9))
    for k in range(2):
        for t, (a, b) in enumerate(idx):
            red[:, t] = red[:, t] + jl3[k][:, a] * jl3[k][:, b]
    for a in range(3):
        red[:, 6 + a] = jl3[0][:, a] * rr[0] + jl3[1][:, a] * rr[1]
    tot = _add_at(p.n_lms, lm, red)
    Hm = np.stack([tot[:, 0], tot[:, 1], tot[:, 2], tot[:, 1], tot[:, 3], tot[:, 4], tot[:, 2], tot[:, 4], tot[:, 5]], 1)
    Hm[:, [0, 4, 8]] += p.lam_lm
    Hi = _inv3_f(Hm)
    out["HLL_INV"] = Hi.reshape(-1)
    w3 = np.stack([Hi[:, 3 * a] * tot[:, 6] + Hi[:, 3 * a + 1] * tot[:, 7] + Hi[:, 3 * a + 2] * tot[:, 8] for a in range(3)], 1)[lm]
    e = [rr[k] - (jl3[k][:, 0] * w3[:, 0] + jl3[k][:, 1] * w3[:, 1] + jl3[k][:, 2] * w3[:, 2]) for k in range(2)]
    q = [sw * D00 * e[0], sw * D00 * e[1], sw * (D02 * e[0] + D12 * e[1])]
    Y = _add_at(p.n_cams, c, np.stack([X[:, j] * q[mm] for mm in range(3) for j in range(4)], 1))
    y12 = Y * sig
    wy = RB._dot(cw, y12)
    out["B_JOINT"] = (y12[:, 1:] - (cb[:, None] * cw[:, 1:]) * wy[:, None]).reshape(-1)
    # cam_build_binv_h
    Hh = np.zeros((p.n_cams, 3, 4, 3, 4))
    Hh[:, 0, :, 0, :] = G[:, 0]
    Hh[:, 1, :, 1, :] = G[:, 0]
    Hh[:, 2, :, 2, :] = G[:, 3]
    for k in range(2):
        Hh[:, k, :, 2, :] = G[:, k + 1]
        Hh[:, 2, :, k, :] = G[:, k + 1]
    A = Hh.reshape(-1, 12, 12) * sig[:, :, None] * sig[:, None, :]
    aw = np.zeros((p.n_cams, 12))
    for k in range(12):
        aw = aw + A[:, :, k] * cw[:, None, k]
    T = A[:, :, 1:] - (cb[:, None] * aw)[:, :, None] * cw[:, None, 1:]
    wt = np.zeros((p.n_cams, 11))
    for k in range(12):
        wt = wt + cw[:, k, None] * T[:, k, :]
    M = T[:, 1:, :] - (cb[:, None, None] * cw[:, 1:, None]) * wt[:, None, :]
    M[:, np.arange(11), np.arange(11)] += p.lam
    out["B_INV_JOINT"] = chol_inverse(M).reshape(-1)
    out["_B"] = M
    return out


# ======== the mutations of test_operand_bounds.py (and of the hand-run GPU mutation check): defects on the reference side
def flagged(dev, ref, bound, per):
    """The blocks (cameras or landmarks, per entries each) with an entry over its bound."""
    err = np.abs(np.asarray(dev, dtype=LD).reshape(-1) - np.asarray(ref, dtype=LD).reshape(-1)).astype(F)
    return set(np.flatnonzero((~(err <= np.asarray(bound).reshape(-1))).reshape(-1, per).any(1)).tolist())


def entry_scale(R, name, i):
    """The smallest power of ten that exceeds ten times the relative bound of entry i of an operand."""
    return 10.0 ** np.ceil(np.log10(10 * R.bound[name][i] / abs(float(R.ref[name][i]))))


def structural_mutations(p, R, joint):
    """[(name, mutate dict, [(operand, per, blocks that must be reported or None = every block)])] for a problem with its
    unmutated reference R: the defects the normwise tests let through (tests/test_operand_bounds.py)."""
    c = p.cam_idx
    first = lambda cam: int(np.flatnonzero(c == cam)[0])
    c1, c2 = int(np.flatnonzero(p.n_c == 1)[0]), int(np.flatnonzero(p.n_c == 2)[0])
    mid = int(np.flatnonzero((p.n_c > 20) & (p.n_c < 400))[0])
    sn, bn, binv, nb = ("JL_COL_SCALE_H", "B_JOINT", "B_INV_JOINT", 11) if joint else ("JL_COL_SCALE", "B", "B_INV", 12)
    sper = 4 if joint else 3
    l2 = int(np.flatnonzero(p.n_l == 2)[0])
    hs = entry_scale(R, "HLL_INV", 9 * l2 + 1)
    out = [("gram_item_dropped", {"drop_gram": [first(c1), first(c2)]}, [("DIAG2", 12, {c1, c2}), ("SIGMA", 12, {c1, c2})]),
           ("sigma_without_eps", {"sigma_no_eps": True}, [("SIGMA", 12, None)]),
           ("hll_inv_unsymmetric", {"entry": {"HLL_INV": (9 * l2 + 1, 1 + hs)}}, [("HLL_INV", 9, {l2})]),
           ("lambda_missing_in_B", {"lam_missing": (mid, 5)}, [(binv, nb * nb, {mid})]),
           ("cold_observation_missing_from_b", {"drop_b": [first(mid)]}, [(bn, nb, {mid})]),
           ("diag2_scaled", {"scale": {"DIAG2": 1 + 1e-9}}, [("DIAG2", 12, set(np.flatnonzero(p.n_c > 0).tolist()))]),
           ("sigma_scaled", {"scale": {"SIGMA": 1 + 1e-9}}, [("SIGMA", 12, None)]),
           ("jl_scale_scaled", {"scale": {sn: 1 + 1e-9}}, [(sn, sper, None)])]
    if p.robust == "HUBER":
        w = R.aux["w"]
        i = int(np.flatnonzero(w < 0.7)[0])
        out.append(("weight_taken_as_one", {"w_one": [i]}, [("DIAG2", 12, {int(c[i])}), (sn, sper, {int(p.lm[i])})]))
    if joint:
        out.append(("beta_doubled", {"beta_double": [c1]}, [("NC_HOUSEHOLDER", 13, {c1})]))
    return out
