"""Componentwise rounding-error bounds for the E0 kernels of both steps: a long-double reference of each kernel's own
factorisation and, from the same chain run on absolute values, a bound on |y_dev - y_ref| for EVERY output entry (helper
module of tests/test_rounding_bounds.py, tests/test_gpu_e0_bounds.py and tests/test_gpu_e0h_bounds.py; not a test module).
Step 1 (pOSE: Step1, evaluate, emulate, edge_problem) comes first, step 2 (RIPOBA: Step2, evaluate_joint, emulate_joint,
edge_problem_joint) after it.

Why componentwise.  A relative 2-norm over 12 n_cams outputs is dominated by the hub cameras: a tail camera's block can be
dropped, doubled or stale without moving it past 1e-12; and for the fp32 terms no normwise tolerance fits, because an
ill-conditioned 3x3 landmark block G amplifies the fp32 error of u = Jl^T Jp x (|G| |u| >> |G u|).  A bound built from the
magnitudes of every intermediate (Higham, "Accuracy and Stability of Numerical Algorithms", 2nd ed., 3.1-3.5: a k-term dot
product or a chain of k dependent operations is exact for operands perturbed by at most gamma_k = k u / (1 - k u)) scales
with the data: it checks the smallest camera as hard as the largest and does not depend on cond(G).

The factorisation ("C-form": lpl_forward / lpl_backward in povar_kernels.hpp, ck_obs_forward / ck_obs_backward in
povar_kernels_ck.hpp, ck32_obs_forward / ck32_obs_backward in povar_kernels_ck_f32.hpp, E0Core of e0_lm_cached).  Per
observation i of camera c and landmark l, with h~ = [X_l; 1], z = sigma * x, Z_c = z_c as a 3x4 matrix (P's layout), P3 the
first three columns of the linearisation point P_c, (u, v) the image point, sb^2 = 1 - alpha, w_i the robust weight:

    forward   d = Z_c h~,   a = w_i C_i d,   u_l += P3^T a,     C_i = [[1, 0, -cu], [0, 1, -cv], [-cu, -cv, cuv]],
              cu = sb^2 u,  cv = sb^2 v,  cuv = sb^2 (u^2 + v^2)
    middle    g_l = G_l u_l,   G_l = S_l Hi_l S_l  (Hi: BUF_HLL_INV, S: diag of BUF_JL_COL_SCALE)
    backward  q = w_i C_i (P3 g_l),   Y_c += [h~; 1] (x) q  (entry 4 m + j = h~_j q_m),   y = sigma * Y

This is the reference's Jp^T D^2 Jl Hll^-1 Jl^T D^2 Jp with the sb / sa rows merged (sa^2 + sb^2 = 1): Jl0^T D^2 Jp0 z =
P3^T C d exactly (tests/exact_rational.py builds the explicit rows; test_rounding_bounds.py checks the restatement against
them).  Its intermediates are NOT bounded by |Jp|, |Jl| of the explicit tiles, so the magnitudes follow this algebra.  The
inputs -- G (from Hi and S), sigma, the cameras, the landmarks -- are the doubles of the context under test, taken as exact
numbers (the device's Hll^-1 differs from the oracle's by 1e-10 at venice size, far above any fp64 rounding bound of E0;
tests/operand_bounds.py holds these operands themselves to bounds that scale with each landmark's cancellation).  The
weights are compute_error_weight's (oracle/povar_oracle.c; HUBER: min(1, t / |r|) of the pOSE residual at the linearisation
point; CAUCHY and NONE: 1 in these kernels).

The bound.  The same chain on absolute values gives magnitudes Dm = |Z| |h~|, Um_i = |P3|^T |w| |C| Dm, U_l = sum_i Um_i,
Gm_l = |G_l| U_l, Qm_i = |w| |C| |P3| Gm_l, Ym_c = sum_i |h~| (x) Qm_i.  An error vector E is carried along the same positive
linear maps, and every stage adds (its rounding count) x (its magnitude):

    E_fwd,i = kf_i Um_i                    kf_i = gamma_KF + dZ + dh + dP + dC + rho_i
    E_u,l   = sum_i E_fwd,i + gamma_{n_l}^lm U_l (+ the fixed-point quantisation of e0_ck_det, below)
    E_g,l   = |G_l| E_u,l + kG Gm_l        kG = gamma_KG + dG
    E_q,i   = |w||C||P3| E_g,l + kb_i Qm_i  kb_i = gamma_KB + dh + dP + dC + rho_i
    E_Y,c   = sum_i (|h~| (x) E_q,i + gamma_1 |h~| (x) Qm_i) + (gamma_16^32 [fp32 only] + gamma_{n_c}^64) Ym_c
    bound   = sigma E_Y + u64 sigma Ym + floor

(first order: the second-order terms are O(k^2 u^2) of the same magnitudes; each gamma below is rounded up to cover them).

Counts, from the kernel sources (u = the arithmetic's unit roundoff; an FMA rounds once, so every count is an upper one):
  KF = 12  d = Z h~: a 4-term dot (4); a = w C d: a2 = w (cuv d2 - cu d0 - cv d1) is a 3-term dot and the product by w (4);
           P3^T a: a 3-term dot (3); E0Core scales by the Jl column scale on the fly (+1).
  KG = 3   g = G u: a 3-term dot.
  KB = 8   e = P3 g (3); q = w C e (4); E0Core's scale (+1).  (The product h~_j q_m is the gamma_1 of E_Y.)
  lm       u_l sums n_l contributions in some order (registers, a segmented scan, ds_add in arrival order): gamma_{n_l}, per
           landmark -- for fp32 (ds_add_f32) that is gamma_{n_l} of fp32, not one global constant.
  cam      Y_c sums n_c observation contributions in fp64 in any tree (chunk registers, the segmented wavefront scan, the LDS
           accumulators, partial records, the cold view, the per-camera sums): gamma_{n_c}; e0_ck_f32 first sums a chunk
           (<= CK_HMAX = 16 rows, ck_layout.hpp) in fp32: + gamma_16 of fp32.
  operands (relative perturbation of a stored operand against the reference's exact value):
           dZ  = u64 (z = sigma x, cam_apply_inc) [+ u32: the fp32 record, ck32_load_z]
           dh  = 0 (fp64) | u32 (the fp32 landmark record, ck32_records)
           dP  = 0 (fp64) | u32 (P3 and the translation in fp32, ck32_records)
           dG  = 2 u64 (G = s_a Hi_ab s_b: two products, prepare_lpl) [+ u32: ck32_records]
           duv = 0 (fp64: a packed point unpacks to the correctly rounded k / 10^6, the file's double -- ck_pack_one packs
                 only what survives that round trip) | 3 u32 (packed fp32 rows:
                 (float) k -- inexact for |k| >= 2^24, i.e. |coordinate| > 16.78 --, 1e-6f and the product; a float2 row
                 rounds once)
           dsb2 = gamma_4^64 (sb = sqrt(1 - alpha) in fp64 and sb * sb, against the exact 1 - alpha) [+ u32: (float) sb2]
           dC  = dsb2 + 2 duv + gamma_3 (cuv = sb2 (u u + v v): u, v squared, summed, scaled; cu, cv round less)
  rho_i    HUBER only (and only where the reference's r2 (1 + its own relative error) reaches t^2: elsewhere both sides take
           w = 1).  The weight is recomputed from r = (sb (p0 - u p2), sb (p1 - v p2), sa (p0 - u), sa (p1 - v)), p = P3 h + t.
           Near convergence r is the difference of much larger numbers: with Pm_k = |P3_k| |h| + |t_k|,
             err(p_k) <= (gamma_4 + dP + dh) Pm_k,   err(a) <= err(p0) + |u| err(p2) + (duv + gamma_2)(|p0| + |u p2|)
             err(c)   <= err(p0) + (duv + u)(|p0| + |u|)        (b, e alike)
             err(r2)  <= 2 (sb2 (|a| err(a) + |b| err(b)) + sa2 (|c| err(c) + |e| err(e))) + (gamma_4 + dsb2) r2
             rho_i    = err(r2) / (2 r2) + gamma_4      (w = t rsq(r2): rsq about 1 ulp, then Newton steps; t rounded once)
           i.e. rho ~ u (|P||h| + |t| + |uv||p2|) / |r|, not a few ulps, wherever |r| is small against its terms.  The same
           rho enters the forward and the backward C (both recompute w).
           stored: series_res does not recompute the weight, it reads the one the linearisation left
           (povar_kernels_res.hpp:442-447: V2::w, or the stored sqrt squared).  That one comes from pose_residual
           (povar_kernels.hpp:264-277) and error_weight (:235-239): the entries sb (P0j - P2j u) of the merged row round three
           times before the 4-term dot, so err(p_k) carries gamma_7 instead of gamma_4 (kp = 7); sa u rounds before it is
           subtracted (k1 = 2: err(c) <= err(p0) + (duv + 2 u)(|p0| + |u|)); w = t / sqrt(r2) is er2 / 2 + 2 u, its stored sqrt
           er2 / 4 + 2 u, the square of that er2 / 2 + 5 u (kw = 5 instead of 4).  Model "fp64_stored_w"; every other count
           of the resident body is e0_ck's (ck_obs_forward, ck_obs_backward unchanged; tests/series_bounds.py cites the lines).
  floor    an absolute 2^-149 per fp32 operation (underflow to subnormals) added at each stage (2^-1074 for fp64).
  det      e0_ck_det sums u_l in 64-bit fixed point on the grid 2^(E + L - 61), 2^E > the largest |contribution| of the
           landmark (first walk), L = ceil(log2 n_l) (povar_kernels_ck_det.hpp:13): each of the n_l contributions rounds by
           at most 2^(E + L - 62) <= 2^(L - 61) max|contribution|; the sum is exact, and its conversion back rounds once.

The explicit-tile modes (E0_TILES / E0_TILES_LDSACC: materialize_tiles + OpE0Tiles) evaluate Jl^T (Jp x) with the stored
Jp = sb sw sigma Jp0 and Jl = sb sw s Jl0; there the magnitudes are |Jl0|^T D^2 |Jp0| |z| (with |Jl0| built from
|P0| + |u| |P2|, since the tile entry P0 - u P2 is computed and may cancel) and the chain
|Jp0|^T D^2 |Jl0| |G| |Jl0|^T D^2 |Jp0| |z| (as exact_rational._rows builds the rows), with KF = 24 (Jp entries: three
products, 3; Jp x: a 12-term dot, 12; Jl entries: P0 - u P2 and three scalings, 5; Jl^T t: 4), KG = 3 (Hi tot) and KB = 13
(Jl v: 3; Jl entries: 5; pose_q: 4; then gamma_1 for h~ q).

Step 2 (RIPOBA: homogeneous landmarks X in R^4, tangent bases).  One application takes the previous term x11 (11 per
camera) to the next one; with N = (I - beta w w^T)[:, 1:] the Householder bases of cameras (BUF_NC_HOUSEHOLDER) and
landmarks (house4 of X), pc = P X = (x, y, z), D = [[1/z, 0, -x/z^2], [0, 1/z, -y/z^2]], sw = sqrt of the robust weight:

    input     z = sigma (N_c x11)
    forward   t = sw D (Z X) (2-vector, Z = z_c as 3x4),   U4_l += P^T D^T (sw t)
    middle    u3 = N_l^T (s o U4),   g3 = Hi u3,   G4 = s o (N_l g3)        (s: BUF_JL_COL_SCALE_H, Hi: BUF_HLL_INV, 3x3)
    backward  q = sw D^T (sw D (P G4)),   Y_c += X (x) q  (entry 4 m + j = X_j q_m)
    tail      y11 = N_c^T (sigma o Y),   t_next = B^-1_c y11               (BUF_B_INV_JOINT, 11x11)

This ambient form (e0_ck_h) and the per-observation form Jl3 = sw D P diag(s) N_l of the other kernels are the same
reference: u3 = sum Jl3^T t = N_l^T (s o U4), Jl3 g3 = sw D P G4 (the header of povar_kernels_ck_joint.hpp).  The operands
-- the cameras and landmarks of the linearisation point, sigma, s, Hi, the camera reflectors (w, beta), B^-1 -- are the
doubles of the context under test taken as exact numbers; that THEY are right, entry by entry, is the business of
tests/operand_bounds.py (test_operand_bounds.py, test_gpu_operand_bounds.py: a long-double reference and a bound for every
operand of both steps, built from what the caller set), not of this module.  N_l is not readable: the reference recomputes
house4 in long double from X, and the model carries the device's fp64 w0, beta as an operand perturbation dN.  Hi is used
as the landmark records keep it (its upper triangle); OpE0H reads all nine entries, so |Hi - Hi^T| u3m is added (zero for
a symmetric inverse).  Weights: compute_error_weight's (HUBER: min(1, t / |r|), r = (x/z - u, y/z - v); CAUCHY and NONE: 1,
so CAUCHY has no branch and nothing to round) in long double; the device stores the fp64 weight at linearisation and every
kernel applies its sqrt twice per pass.

The step-2 bound.  Magnitudes use |N| = |I| + beta |w| |w|^T and |D| = A = (|1/z|, |x|/z^2, |y|/z^2); x, y, z are computed
4-term dots, err(x) <= gamma_4 (|P0| . |X|) =: gamma_4 xm, so with ez = gamma_4 zm / |z|

    E00 = A00 (ez + u),   E02 = A02 (2 ez + kD u) + gamma_4 xm / z^2     (E12 alike)

-- a small |z| inflates the bound through err(z) / |z|, not through a constant.  With dm = |X| . |Z| and the input error
Ez = gamma_15 sigma (|[0; x]| + beta |w| (|w[1:]| . |x|)) (an 11-term dot, beta w_i wt, the difference, sigma:
nc_z_entry, povar_kernels_joint.hpp:613-620: the one body of cam_cold_sum_binv_h and cam_binv_axpy_h, povar_kernels_cam.hpp):

    Ed   = |X| . Ez + gamma_4 dm
    tm_k = sw (A00 dm_k + A_k2 dm_2),    Et_k = sw (A00 Ed_k + A_k2 Ed_2 + E00 dm_k + E_k2 dm_2) + (gamma_3 + rho) tm_k
    em   = sw |D|^T tm,                  Ee   = sw (|D|^T Et + E^T tm) + (gamma_2 | gamma_3 + rho) em
    vm   = |P|^T em,                     Ev   = |P|^T Ee + (gamma_kv + rho) vm
    UM_l = sum vm,                       EU   = sum Ev  (+ the fixed-point grid of e0_ck_h_det, below)
    u3m  = |N_l|^T (s o UM),             Eu3  = |N_l|^T (s o EU) + (gamma_klm + gamma_{n_l} + dN) u3m
    g3m  = |Hi| u3m,                     Eg3  = |Hi| Eu3 + gamma_3 g3m + |Hi - Hi^T| u3m
    G4m  = s o (|N_l| g3m),              EG4  = s o (|N_l| Eg3) + (gamma_7 + dN) G4m
    pm   = |P| G4m,                      Ep   = |P| EG4 + gamma_4 pm
    sm, qm, Es, Eq as tm, em, Et, Ee;    Ym_c = sum |X| (x) qm,   EY = sum (|X| (x) Eq + gamma_1 |X| (x) qm) + gamma_{n_c} Ym
    y12m = sigma Ym,                     Ey12 = sigma EY + u y12m
    y11m = |N_c|^T y12m,                 Ey11 = |N_c|^T Ey12 + gamma_15 y11m
    bound = |B^-1| Ey11 + gamma_11 |B^-1| y11m

The per-observation and the ambient form have the SAME magnitudes: jl4m^T tm = |P|^T (sw |D|^T tm) = vm entry by entry, and
|N_l|^T distributes over the landmark's sum.  Only the counts differ, one ModelH per family:

  kD       D02 beyond 2 ez.  hom_project (povar_kernels_joint.hpp:25-35): z z and the division, 2.  ckh_project
           (povar_kernels_ck_joint.hpp:91-101): D00 D00 carries D00's own rounding twice and rounds, x iz2 rounds, 4.
  t, s     hom_jp_x (:65-69): a product, an FMA, the scale: gamma_3; d: a 4-term dot (gamma_4).  ckh_obs_backward
           (ck_joint:125-127): dot4 (gamma_4 on pm), then the same three.
  e, q     sw D00 t: two products (gamma_2); sw (D02 t0 + D12 t1): gamma_3 (ckh_obs_forward, ck_joint:112; hom_q, :70-72).
  kv       ambient: P0j e0 + P1j e1 + P2j e2 (ck_joint:113-116), gamma_3, on top of e's gamma_3: 6.  Jl3 form: the entry
           sw (D00 P + D02 P2) s of hom_jl4 (:37-46): product, FMA, two scalings, 4 (it replaces e's count, not adds to it;
           6 and 4 are both upper counts of the same sum Ev).
  klm      ambient, ckh_landmark_step (ck_joint:176-194): s o U4 (1), aw a 4-term dot (4), hbeta aw hw and the difference
           (3): 8.  Jl3 form, jl3_of_jl4 (:56-63): the same 7, then jl3 t0 + jl3' t1 (:216, :351, :782): 9.
  n_l      the landmark's sum in any order (LDS atomics in arrival order, a segmented scan, wave_sum of lm_long): gamma_{n_l}.
  back     G4: hbeta times a 3-term dot (4), gw hw, the difference, s (3): gamma_7 (ck_joint:189-193).  Jl3 form: jl3_of_jl4's
           7 on the row, hom_jl4's 4 where the ambient form has dot4's 4, a 3-term dot where it has hom_jp_x's 3: the same 14.
  n_c      X_j q_m rounds once (or is an FMA into the sum); the camera's sum in any tree (chunk registers, LDS accumulators of
           either stride, partial records of capped accumulators, the cold view, block_sum_dpp; adding zeros is exact):
           gamma_{n_c}.
  tail     sigma (1); nt_apply (:589-595): a 12-term dot, beta w wy (2), the difference: gamma_15; the B^-1 row: an 11-term
           dot (binv_row11 :602-607; CamJoint::solve, povar_kernels_cam.hpp:189-200; cam_binv_axpy_h :364-401 after cam_cold_sum: the same counts).
  dN       house4 (:48-55): nv = sqrt of a 4-term sum of squares (gamma_4 at most), w0 = X.x +- nv with equal signs (one
           more: gamma_5), beta = 2 / (sum of four squares, w0^2 among them: 2 gamma_5 + 1, the sum 4, the division 1:
           gamma_15 at most); an entry beta w_i w_j of N moves by gamma_15 + 2 gamma_5 <= gamma_25 of itself <= of |N|.
  rho_i    HUBER only, the relative error of the stored weight's sqrt (it enters four times: twice per pass):
             err(x/z) <= gamma_4 xm / |z| + |x/z| (ez + u),   err(r0) <= err(x/z) + u (|x/z| + |u|)
             rel = (2 (|r0| err(r0) + |r1| err(r1))) / r2 + gamma_3,   rho = rel / 4 + gamma_4
           (w = t / sqrt(r2) halves rel, its sqrt halves it again; t t, two square roots, the division).  rho is charged
           wherever r2 (1 + rel) reaches t^2 -- also where the device may take the other branch of r2 < t^2: then one side
           has sw = 1 and the other (t^2 / r2)^(1/4) within rel / 4 of it --, no entry is left out.
  det      e0_ck_h_det sums U4 on the grid 2^(E + L - 61), 2^E > the largest |component| of the landmark's contributions
           (first walk), L = ceil(log2 n_l) (povar_kernels_ck_det.hpp:250-287, :355-377): each contribution rounds by at most
           2^(L - 61) max vm; the integer sum is exact and its conversion back rounds once.

First order, every gamma rounded up, as for step 1; no underflow floor (the cameras have unit norm and the terms of the
first five steps stay far above 2^-1022; the camera without observations has bound 0 and must be exactly 0).

Slack.  On the problems of test_rounding_bounds.py, NumPy emulations that follow the kernels' operation order and operand
roundings reach at most the err/bound ratios recorded in that module's docstring; a ratio near 1 would mean a count is
missing, a ratio of 1e-6 a vacuous bound.
"""
import numpy as np

LD = np.longdouble
U64 = 2.0 ** -53
U32 = 2.0 ** -24
ULD = float(np.finfo(np.longdouble).eps) / 2
BLOCK = 1 << 19  # observations per block of the reference (whole landmarks)


def gam(k, u):
    k = np.asarray(k, dtype=np.float64)
    return k * u / (1.0 - k * u)


class Model:
    """The rounding model of one kernel family (module docstring)."""

    def __init__(self, name, u, form="C", u_lm=None, kf=12, kg=3, kb=8, dz=U64, dh=0.0, dp=0.0, dg=2 * U64, duv=0.0,
                 dsb2=None, chunk32=False, det=False, eta=2.0 ** -1074, kp=4, k1=1, kw=4):
        self.name, self.u, self.form = name, u, form
        self.kp, self.k1, self.kw = kp, k1, kw  # (rho_i: the counts of the weight's residual -- module docstring)
        self.u_lm = u if u_lm is None else u_lm
        self.kf, self.kg, self.kb = kf, kg, kb
        self.dz, self.dh, self.dp, self.dg, self.duv = dz, dh, dp, dg, duv
        self.dsb2 = float(gam(4, U64)) if dsb2 is None else dsb2
        self.dc = self.dsb2 + 2 * duv + float(gam(3, u))
        self.chunk32, self.det, self.eta = chunk32, det, eta


MODELS = {
    # e0_lpl, e0_ck, E0Core (lane-per-observation implicit kernels): fp64 C-form
    "fp64": Model("fp64", U64),
    # series_res (povar_kernels_res.hpp): the fp64 C-form with the STORED weight of the linearisation (rho_i: "stored")
    "fp64_stored_w": Model("fp64_stored_w", U64, kp=7, k1=2, kw=5),
    # e0_ck_det: fp64 C-form, u_l in fixed point
    "det": Model("det", U64, det=True),
    # e0_ck_f32 (include/povar_hip.h: the fp32 contract)
    "fp32": Model("fp32", U32, dz=U64 + U32, dh=U32, dp=U32, dg=2 * U64 + U32, duv=3 * U32,
                  dsb2=float(gam(4, U64)) + U32, chunk32=True, eta=2.0 ** -149),
    # the stored-tile modes (E0_TILES, E0_TILES_LDSACC)
    "explicit": Model("explicit", U64, form="explicit", kf=24, kg=3, kb=13, dg=0.0),
    # the long-double reference itself (checked against exact rationals): every operand exact but G (one rounding)
    "longdouble": Model("longdouble", ULD, dz=ULD, dg=ULD, duv=0.0, dsb2=ULD, eta=0.0),
}


class Step1:
    """The operands of one prepared step-1 system, as exact numbers."""

    def __init__(self, n_cams, lm_off, cam_idx, obs, cams, lms, alpha, sigma, G, robust="NONE", huber=1.0):
        self.n_cams = int(n_cams)
        self.lm_off = np.asarray(lm_off, dtype=np.int64)
        self.cam_idx = np.asarray(cam_idx, dtype=np.int64)
        self.obs = np.asarray(obs, dtype=np.float64).reshape(-1, 2)
        self.cams = np.asarray(cams, dtype=np.float64).reshape(-1, 12)
        self.lms = np.asarray(lms, dtype=np.float64).reshape(-1, 3)
        self.alpha = float(alpha)
        self.sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
        self.G = np.asarray(G, dtype=LD).reshape(-1, 3, 3)
        self.robust, self.huber = robust, float(huber)
        self.n_l = np.diff(self.lm_off)
        self.n_c = np.bincount(self.cam_idx, minlength=self.n_cams)

    @classmethod
    def from_context(cls, ctx, obs, alpha, robust="NONE", huber=1.0):
        from povar_amd import capi
        hi = ctx.get_buffer(capi.BUF_HLL_INV).reshape(-1, 3, 3).astype(LD)
        s = ctx.get_buffer(capi.BUF_JL_COL_SCALE).reshape(-1, 3).astype(LD)
        G = s[:, :, None] * hi * s[:, None, :]
        return cls(ctx.n_cams, ctx.lm_off, ctx.cam_idx, obs, ctx.get_cameras(), ctx.get_landmarks(), alpha,
                   ctx.get_buffer(capi.BUF_POSE_SCALING), G, robust, huber)


def _seg(starts, a):
    return np.add.reduceat(a, starts, axis=0) if len(a) else a


def huber_rho(P, t, hx, uv, sb2, sa2, model):
    """Relative error of the recomputed HUBER weight per observation (module docstring: rho_i), and the reference r2."""
    f = np.float64
    ab = lambda a: np.abs(a.astype(f))
    p = [P[:, 4 * k] * hx[0] + P[:, 4 * k + 1] * hx[1] + P[:, 4 * k + 2] * hx[2] + P[:, 4 * k + 3] for k in range(3)]
    Pm = [ab(P[:, 4 * k]) * ab(hx[0]) + ab(P[:, 4 * k + 1]) * ab(hx[1]) + ab(P[:, 4 * k + 2]) * ab(hx[2]) + ab(P[:, 4 * k + 3])
          for k in range(3)]
    u, v = uv[:, 0], uv[:, 1]
    a, b, c, e = p[0] - u * p[2], p[1] - v * p[2], p[0] - u, p[1] - v
    r2 = sb2 * (a * a + b * b) + sa2 * (c * c + e * e)
    kp = float(gam(model.kp, model.u)) + model.dp + model.dh
    ep = [kp * m for m in Pm]
    d2 = model.duv + float(gam(2, model.u))
    ea = ep[0] + np.abs(u) * ep[2] + d2 * (ab(p[0]) + np.abs(u) * ab(p[2]))
    eb = ep[1] + np.abs(v) * ep[2] + d2 * (ab(p[1]) + np.abs(v) * ab(p[2]))
    d1 = model.duv + model.k1 * model.u
    ec = ep[0] + d1 * (ab(p[0]) + np.abs(u))
    ee = ep[1] + d1 * (ab(p[1]) + np.abs(v))
    fs, fa = float(sb2), float(sa2)
    r2f = np.maximum(r2.astype(f), 1e-300)
    er2 = 2 * (fs * (ab(a) * ea + ab(b) * eb) + fa * (ab(c) * ec + ab(e) * ee)) + (float(gam(4, model.u)) + model.dsb2) * r2f
    rho = er2 / (2 * r2f) + float(gam(model.kw, model.u))
    return rho, r2, er2 / r2f


def weights(prob, P, hx, uv, sb2, sa2, model):
    n = len(uv)
    if prob.robust != "HUBER":
        return np.ones(n, dtype=LD), np.zeros(n)
    rho, r2, rel = huber_rho(P, LD(prob.huber), hx, uv, sb2, sa2, model)
    t2 = LD(prob.huber) ** 2
    w = np.where(r2 < t2, LD(1), LD(prob.huber) / np.sqrt(r2))
    near = r2.astype(np.float64) * (1 + rel) >= float(t2)  # (where the device could take the other branch or w < 1)
    return w, np.where(near, rho, 0.0)


def evaluate(prob, x, model=MODELS["fp64"], want_parts=False, mutate=None):
    """(y_ref, bound): the long-double C-form E0 x and the componentwise bound of `model`, both [12 n_cams].
    mutate: test hook (a dict) that perturbs the reference's chain -- test_rounding_bounds.py's mutations."""
    f = np.float64
    sig = prob.sigma.astype(LD)
    z = (sig * np.asarray(x, dtype=np.float64).astype(LD)).reshape(-1, 12)
    zm = np.abs(z).astype(f)
    sb2 = LD(1) - LD(prob.alpha)
    sa2 = LD(prob.alpha)
    Y = np.zeros((prob.n_cams, 12), dtype=LD)
    Ym = np.zeros((prob.n_cams, 12))
    EY = np.zeros((prob.n_cams, 12))
    u = model.u
    g1 = float(gam(1, u))
    n_lms = len(prob.lm_off) - 1
    l0 = 0
    while l0 < n_lms:
        l1 = int(np.searchsorted(prob.lm_off, prob.lm_off[l0] + BLOCK, side="right")) - 1
        l1 = max(l1, l0 + 1)
        o0, o1 = int(prob.lm_off[l0]), int(prob.lm_off[l1])
        nl = prob.n_l[l0:l1]
        keep = nl > 0
        lm = np.repeat(np.arange(l0, l1), nl)
        c = prob.cam_idx[o0:o1]
        uv = prob.obs[o0:o1]
        if mutate and "uv" in mutate:
            uv = mutate["uv"](uv, o0, o1)
        uvl = uv.astype(LD)
        X = prob.lms[lm].astype(LD)
        hx = [X[:, 0], X[:, 1], X[:, 2]]
        P = prob.cams[c].astype(LD)
        Z = z[c]
        w, rho = weights(prob, P, hx, uvl, sb2, sa2, model)
        if mutate and "w" in mutate:
            w = mutate["w"](w, o0, o1)
        wm = np.abs(w.astype(f))
        cu, cv = sb2 * uvl[:, 0], sb2 * uvl[:, 1]
        cuv = sb2 * (uvl[:, 0] ** 2 + uvl[:, 1] ** 2)
        Cm = np.abs(np.stack([cu, cv, cuv], 1).astype(f))
        Xm = np.abs(prob.lms[lm])
        Pf = np.abs(prob.cams[c])
        # ---- forward (the reference in long double, the magnitudes in double)
        d = [hx[0] * Z[:, 4 * r] + hx[1] * Z[:, 4 * r + 1] + hx[2] * Z[:, 4 * r + 2] + Z[:, 4 * r + 3] for r in range(3)]
        Dm = [Xm[:, 0] * zm[c, 4 * r] + Xm[:, 1] * zm[c, 4 * r + 1] + Xm[:, 2] * zm[c, 4 * r + 2] + zm[c, 4 * r + 3]
              for r in range(3)]
        a = [w * (d[0] - cu * d[2]), w * (d[1] - cv * d[2]), w * (cuv * d[2] - cu * d[0] - cv * d[1])]
        red = np.stack([P[:, m] * a[0] + P[:, 4 + m] * a[1] + P[:, 8 + m] * a[2] for m in range(3)], 1)
        if model.form == "C":
            Am = [wm * (Dm[0] + Cm[:, 0] * Dm[2]), wm * (Dm[1] + Cm[:, 1] * Dm[2]),
                  wm * (Cm[:, 2] * Dm[2] + Cm[:, 0] * Dm[0] + Cm[:, 1] * Dm[1])]
            Um = np.stack([Pf[:, m] * Am[0] + Pf[:, 4 + m] * Am[1] + Pf[:, 8 + m] * Am[2] for m in range(3)], 1)
        else:
            Jl, T, D2 = _explicit_rows(Pf, uv, Dm, float(sb2), float(sa2))
            Um = sum(wm[:, None] * D2[r] * T[r][:, None] * Jl[r] for r in range(4))
        kf = float(gam(model.kf, u)) + model.dz + model.dh + model.dp + model.dc + rho
        Ef = kf[:, None] * Um + model.kf * model.eta
        starts = (prob.lm_off[l0:l1] - o0)[keep]
        ul = np.zeros((l1 - l0, 3), dtype=LD)
        Ul = np.zeros((l1 - l0, 3))
        Eu = np.zeros((l1 - l0, 3))
        ul[keep] = _seg(starts, red)
        Ul[keep] = _seg(starts, Um)
        Eu[keep] = _seg(starts, Ef)
        Eu += gam(nl, model.u_lm)[:, None] * Ul + (nl * model.eta)[:, None]
        if model.det:
            Umax = np.zeros(l1 - l0)
            Umax[keep] = np.maximum.reduceat(Um.max(1), starts)
            L = np.ceil(np.log2(np.maximum(nl, 1)))
            Eu += (nl * 2.0 ** (L - 61) * Umax)[:, None] * (1 + 8 * U64) + U64 * Ul
        # ---- middle
        G = prob.G[l0:l1]
        if mutate and "G" in mutate:
            G = mutate["G"](G, l0, l1)
        Gf = np.abs(G.astype(f))
        g = np.einsum("lab,lb->la", G, ul)
        Gm = np.einsum("lab,lb->la", Gf, Ul)
        Eg = np.einsum("lab,lb->la", Gf, Eu) + (float(gam(model.kg, u)) + model.dg) * Gm + model.kg * model.eta
        # ---- backward
        gl, Gml, Egl = g[lm - l0], Gm[lm - l0], Eg[lm - l0]
        e = [P[:, 4 * k] * gl[:, 0] + P[:, 4 * k + 1] * gl[:, 1] + P[:, 4 * k + 2] * gl[:, 2] for k in range(3)]
        q = np.stack([w * (e[0] - cu * e[2]), w * (e[1] - cv * e[2]), w * (cuv * e[2] - cu * e[0] - cv * e[1])], 1)
        kb = float(gam(model.kb, u)) + model.dh + model.dp + model.dc + rho
        if model.form == "C":
            def back(V):
                em = [Pf[:, 4 * k] * V[:, 0] + Pf[:, 4 * k + 1] * V[:, 1] + Pf[:, 4 * k + 2] * V[:, 2] for k in range(3)]
                return np.stack([wm * (em[0] + Cm[:, 0] * em[2]), wm * (em[1] + Cm[:, 1] * em[2]),
                                 wm * (Cm[:, 2] * em[2] + Cm[:, 0] * em[0] + Cm[:, 1] * em[1])], 1)
            Qm, Eq = back(Gml), back(Egl)
            hm = np.concatenate([Xm, np.ones((len(Xm), 1))], 1)
            ym = (Qm[:, :, None] * hm[:, None, :]).reshape(-1, 12)
            ey = (Eq[:, :, None] * hm[:, None, :]).reshape(-1, 12)
        else:
            ym, ey = (_explicit_back(Jl, D2, wm, Xm, uv, V) for V in (Gml, Egl))
        ey = ey + (kb[:, None] + g1) * ym + (model.kb + 1) * model.eta
        h4 = [hx[0], hx[1], hx[2], np.ones(len(uv), dtype=LD)]
        y = np.stack([q[:, mm] * h4[j] for mm in range(3) for j in range(4)], 1)
        # ---- per camera: camera-sorted, summed with reduceat (np.bincount would cast to float64)
        order = np.argsort(c, kind="stable")
        cs = c[order]
        cst = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]])
        cams_here = cs[cst]
        Y[cams_here] += np.add.reduceat(y[order], cst, axis=0)
        Ym[cams_here] += np.add.reduceat(ym[order], cst, axis=0)
        EY[cams_here] += np.add.reduceat(ey[order], cst, axis=0)
        l0 = l1
    ksum = gam(prob.n_c, U64) + (float(gam(16, U32)) if model.chunk32 else 0.0)
    EY += ksum[:, None] * Ym + prob.n_c[:, None] * model.eta
    sf = prob.sigma.reshape(-1, 12)
    y_ref = (sig.reshape(-1, 12) * Y).reshape(-1)
    bound = (sf * EY + U64 * sf * Ym).reshape(-1) * (1 + 1e-6)
    if want_parts:
        return y_ref, bound, dict(Ym=(sf * Ym).reshape(-1))
    return y_ref, bound


def _explicit_rows(Pf, uv, Dm, sb2, sa2):
    au, av = np.abs(uv[:, 0]), np.abs(uv[:, 1])
    jl0 = Pf[:, 0:3] + au[:, None] * Pf[:, 8:11]
    jl1 = Pf[:, 4:7] + av[:, None] * Pf[:, 8:11]
    Jl = [jl0, jl1, Pf[:, 0:3], Pf[:, 4:7]]
    T = [Dm[0] + au * Dm[2], Dm[1] + av * Dm[2], Dm[0], Dm[1]]
    return Jl, T, [sb2, sb2, sa2, sa2]


def _explicit_back(Jl, D2, wm, Xm, uv, V):
    s = [wm * D2[r] * (Jl[r] * V).sum(1) for r in range(4)]
    hm = np.concatenate([Xm, np.ones((len(Xm), 1))], 1)
    au, av = np.abs(uv[:, 0]), np.abs(uv[:, 1])
    blocks = [s[0] + s[2], s[1] + s[3], au * s[0] + av * s[1]]
    return np.concatenate([b[:, None] * hm for b in blocks], 1)


def check(y_dev, y_ref, bound):
    """(worst err / bound, index of it, number of entries over their bound)."""
    err = np.abs(np.asarray(y_dev, dtype=LD) - y_ref).astype(np.float64)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(ratio))
    return float(ratio[i]), i, int((ratio > 1).sum())


# ---- NumPy emulations of the kernels' operation order and operand roundings (test_rounding_bounds.py)
def emulate(prob, x, dtype, packed=True, chunk=16):
    """E0 x as e0_ck (dtype float64) or e0_ck_f32 (float32) evaluates it: operands rounded where the kernel stores them,
    the per-observation chain in dtype, u_l summed in dtype in row order, each camera's observations summed in chunks of
    `chunk` rows in dtype, the chunk sums in fp64."""
    f, T = np.float64, dtype
    z = prob.sigma * np.asarray(x, dtype=f)  # (cam_apply_inc: fp64)
    Zs = z.reshape(-1, 12).astype(T)
    lm = np.repeat(np.arange(len(prob.lm_off) - 1), prob.n_l)
    c = prob.cam_idx
    Pc = prob.cams.astype(T)
    Gd = prob.G.astype(f).astype(T)
    X = prob.lms.astype(T)
    uv = prob.obs
    uvt = uv.astype(T)
    if packed:  # (a point packs where k * 1e-6 is the file's double: the layout checks it per point)
        k = np.rint(uv * 1e6)
        pk = np.all(k * 1e-6 == uv, axis=1) & np.all(np.abs(k) < 2 ** 31, axis=1)
        if T == np.float32:  # (ck32_unpack; the fp64 kernels unpack to the file's double itself)
            uvt[pk] = k[pk].astype(T) * T(1e-6)
    sb = np.sqrt(f(1.0 - prob.alpha))
    sb2, sa2 = T(sb * sb), T(np.sqrt(prob.alpha) ** 2)
    P, Z, h, U, V = Pc[c], Zs[c], X[lm], uvt[:, 0], uvt[:, 1]
    if prob.robust == "HUBER":
        p = [P[:, 4 * k] * h[:, 0] + P[:, 4 * k + 1] * h[:, 1] + P[:, 4 * k + 2] * h[:, 2] + P[:, 4 * k + 3] for k in range(3)]
        a, b, cc, e = p[0] - U * p[2], p[1] - V * p[2], p[0] - U, p[1] - V
        r2 = sb2 * (a * a + b * b) + sa2 * (cc * cc + e * e)
        t = T(prob.huber)
        w = np.where(r2 < t * t, T(1), t / np.sqrt(r2)).astype(T)
    else:
        w = np.ones(len(c), dtype=T)
    cu, cv, cuv = sb2 * U, sb2 * V, sb2 * (U * U + V * V)
    d = [h[:, 0] * Z[:, 4 * r] + h[:, 1] * Z[:, 4 * r + 1] + h[:, 2] * Z[:, 4 * r + 2] + Z[:, 4 * r + 3] for r in range(3)]
    a = [w * (d[0] - cu * d[2]), w * (d[1] - cv * d[2]), w * (cuv * d[2] - cu * d[0] - cv * d[1])]
    red = np.stack([P[:, m] * a[0] + P[:, 4 + m] * a[1] + P[:, 8 + m] * a[2] for m in range(3)], 1)
    n_l = len(prob.lm_off) - 1
    ul = np.zeros((n_l, 3), dtype=T)
    for i in range(len(c)):  # arrival order: row order (one rounding per add, as ds_add)
        ul[lm[i]] += red[i]
    g = np.einsum("lab,lb->la", Gd, ul).astype(T)
    gl = g[lm]
    e = [P[:, 4 * k] * gl[:, 0] + P[:, 4 * k + 1] * gl[:, 1] + P[:, 4 * k + 2] * gl[:, 2] for k in range(3)]
    q = [w * (e[0] - cu * e[2]), w * (e[1] - cv * e[2]), w * (cuv * e[2] - cu * e[0] - cv * e[1])]
    h4 = [h[:, 0], h[:, 1], h[:, 2], np.ones(len(c), dtype=T)]
    y = np.stack([q[m] * h4[j] for m in range(3) for j in range(4)], 1).astype(T)
    Y = np.zeros((prob.n_cams, 12), dtype=f)
    order = np.argsort(c, kind="stable")
    for cam in range(prob.n_cams):
        rows = order[c[order] == cam]
        for s0 in range(0, len(rows), chunk):
            acc = np.zeros(12, dtype=T)
            for i in rows[s0:s0 + chunk]:
                acc = (acc + y[i]).astype(T)
            Y[cam] += acc.astype(f)
    return (prob.sigma.reshape(-1, 12) * Y).reshape(-1)


# ---- problems
def system(n_cams, lm_off, cam_idx, obs, cams, lms, alpha, robust="NONE", huber=1.0, eps=1e-5):
    """sigma and G = S (S Hll S)^-1 S of a step-1 system in fp64 (the roles of BUF_POSE_SCALING, BUF_JL_COL_SCALE and
    BUF_HLL_INV; taken as exact numbers like a context's).  Returns (Step1, s, Hi)."""
    lm_off = np.asarray(lm_off, dtype=np.int64)
    cam_idx = np.asarray(cam_idx, dtype=np.int64)
    n_l = len(lm_off) - 1
    lm = np.repeat(np.arange(n_l), np.diff(lm_off))
    P = np.asarray(cams, dtype=np.float64).reshape(-1, 12)[cam_idx].reshape(-1, 3, 4)
    X = np.asarray(lms, dtype=np.float64)[lm]
    h = np.concatenate([X, np.ones((len(X), 1))], 1)
    u, v = obs[:, 0], obs[:, 1]
    sa, sb = np.sqrt(alpha), np.sqrt(1 - alpha)
    p = np.einsum("nij,nj->ni", P, h)
    res = np.stack([sb * (p[:, 0] - u * p[:, 2]), sb * (p[:, 1] - v * p[:, 2]), sa * (p[:, 0] - u), sa * (p[:, 1] - v)], 1)
    r2 = (res ** 2).sum(1)
    w = np.where(r2 < huber * huber, 1.0, huber / np.sqrt(np.maximum(r2, 1e-300))) if robust == "HUBER" else np.ones(len(u))
    sw = np.sqrt(w)
    Jl = np.stack([sb * (P[:, 0, :3] - u[:, None] * P[:, 2, :3]), sb * (P[:, 1, :3] - v[:, None] * P[:, 2, :3]),
                   sa * P[:, 0, :3], sa * P[:, 1, :3]], 1) * sw[:, None, None]
    H = np.zeros((n_l, 3, 3))
    np.add.at(H, lm, np.einsum("nra,nrb->nab", Jl, Jl))
    s = 1.0 / (eps + np.sqrt(np.einsum("laa->la", H)))
    Hi = np.linalg.inv(s[:, :, None] * H * s[:, None, :])
    d2 = np.zeros((n_cams, 12))
    hh = h * h
    jp2 = np.concatenate([(sb * sb + sa * sa) * hh, (sb * sb + sa * sa) * hh, sb * sb * (u * u + v * v)[:, None] * hh], 1) * w[:, None]
    np.add.at(d2, cam_idx, jp2)
    sigma = (1.0 / (eps + np.sqrt(d2))).reshape(-1)
    G = s.astype(LD)[:, :, None] * Hi.astype(LD) * s.astype(LD)[:, None, :]
    return Step1(n_cams, lm_off, cam_idx, obs, cams, lms, alpha, sigma, G, robust, huber), s, Hi


EDGE_HUBER = 0.3


def edge_problem(seed=0):
    """A graph built to take the paths a Zipf graph's normwise check cannot see (generated like test_gpu_fuzz's random
    problems: affine-leaning cameras, landmark-major observations):
      * 4 hub cameras with ~3000 observations each (many 16-row chunks, more than one workgroup's share);
      * >= 30 % of the cameras with one or two observations;
      * 6 landmarks with 70-100 observations (more than a wavefront);
      * 60 two-view landmarks seen by a camera and its near twin (near-parallel rays: cond(Hll) >= 1e6);
      * image coordinates up to ~60 (|u| > 16.78: a packed fp32 row's (float) k is inexact there);
      * every point on the six-decimal grid (k * 1e-6: the chunk layout packs the rows; FLAG_NO_PACKED_ROWS keeps doubles);
      * residuals that EDGE_HUBER splits (a fifth or more on either side of the threshold).
    Returns (n_cams, lm_off, cam_idx, obs, cams, lms)."""
    rng = np.random.default_rng(seed)
    n_hub, n_mid, n_tail, n_twin = 4, 60, 56, 30
    n_c = n_hub + n_mid + n_tail + n_twin
    cams = np.zeros((n_c, 12))
    cams[:, :8] = 4.0 * rng.normal(size=(n_c, 8))
    cams[:, 8:11] = 0.05 * rng.normal(size=(n_c, 3))
    cams[:, 11] = 1.0
    twin_of = np.arange(n_hub, n_hub + n_twin)  # camera t and n_c - n_twin + t are near twins
    cams[n_c - n_twin:] = cams[twin_of] + 1e-5 * rng.normal(size=(n_twin, 12))
    lists = []
    hubs, mids = np.arange(n_hub), np.arange(n_hub, n_hub + n_mid)
    tails = np.arange(n_hub + n_mid, n_hub + n_mid + n_tail)
    for _ in range(4000):  # ordinary landmarks: hubs and middle cameras
        k = int(rng.integers(2, 6))
        pool = np.r_[hubs, rng.choice(mids, k, replace=False)]
        lists.append(np.sort(rng.choice(pool, k, replace=False)))
    for t in tails:  # every tail camera: one or two observations
        for _ in range(int(rng.integers(1, 3))):
            lists.append(np.sort(np.r_[t, rng.choice(np.r_[hubs, mids], int(rng.integers(1, 4)), replace=False)]))
    for _ in range(6):  # long landmarks
        lists.append(np.sort(rng.choice(np.r_[hubs, mids, n_c - n_twin + np.arange(n_twin)], int(rng.integers(70, 95)), replace=False)))
    for t in range(60):  # two views with near-parallel rays
        a = t % n_twin
        lists.append(np.array([twin_of[a], n_c - n_twin + a]))
    rng.shuffle(lists)
    degs = np.array([len(x) for x in lists])
    lm_off = np.concatenate([[0], np.cumsum(degs)]).astype(np.int32)
    cam_idx = np.concatenate(lists).astype(np.int32)
    X = 2.0 * rng.normal(size=(len(lists), 3))
    lm = np.repeat(np.arange(len(lists)), degs)
    P = cams[cam_idx].reshape(-1, 3, 4)
    p = np.einsum("nij,nj->ni", P, np.concatenate([X[lm], np.ones((len(lm), 1))], 1))
    obs = p[:, :2] / p[:, 2:3] + rng.normal(scale=0.05, size=(len(lm), 2))
    obs[rng.random(len(lm)) < 0.05] += rng.normal(scale=3.0, size=(1, 2))  # outliers for the robust norms
    obs = np.rint(obs * 1e6) / 1e6
    return n_c, lm_off, cam_idx, obs, cams, X


# ======== step 2 (RIPOBA: homogeneous landmarks, tangent bases) -- the module docstring's second half
class ModelH:
    """The rounding model of one step-2 kernel family (module docstring: step 2)."""

    def __init__(self, name, u, kd, kv, klm, det=False, dn=None):
        self.name, self.u, self.kd, self.kv, self.klm, self.det = name, u, kd, kv, klm, det
        self.dn = float(gam(25, u)) if dn is None else dn


MODELS_H = {
    # e0_ck_h (either stride): ckh_project, the ambient U4 / G4 through LDS, N_l, s, Hll^-1 once per slot
    "ckh": ModelH("ckh", U64, kd=4, kv=6, klm=8),
    # e0_ck_h_det: the same with U4 summed on the fixed-point grid
    "ckh_det": ModelH("ckh_det", U64, kd=4, kv=6, klm=8, det=True),
    # e0_lpl_h, e0_lm_cached_h, lm_regular / lm_long<OpE0H>: hom_project, hom_jl4, jl3_of_jl4 per observation
    "jl3": ModelH("jl3", U64, kd=2, kv=4, klm=9),
    # the long-double reference itself (checked against exact rationals with the reflectors given: dn = 0 there)
    "longdouble": ModelH("longdouble", ULD, kd=4, kv=6, klm=8),
}


class Step2:
    """The operands of one prepared joint system, as exact numbers.  lw: optional [n_lms, 5] landmark reflectors (w, beta)
    taken as given instead of recomputed from X (test_rounding_bounds.py's exact-rational case)."""

    def __init__(self, n_cams, lm_off, cam_idx, obs, cams, lms_h, sigma, s, hi, ncw, binv, robust="NONE", huber=1.0, lw=None):
        f = np.float64
        self.n_cams = int(n_cams)
        self.lm_off = np.asarray(lm_off, dtype=np.int64)
        self.cam_idx = np.asarray(cam_idx, dtype=np.int64)
        self.obs = np.asarray(obs, dtype=f).reshape(-1, 2)
        self.cams = np.asarray(cams, dtype=f).reshape(-1, 12)
        self.lms = np.asarray(lms_h, dtype=f).reshape(-1, 4)
        self.sigma = np.asarray(sigma, dtype=f).reshape(-1, 12)
        self.s = np.asarray(s, dtype=f).reshape(-1, 4)
        self.hi = np.asarray(hi, dtype=f).reshape(-1, 3, 3)
        self.ncw = np.asarray(ncw, dtype=f).reshape(-1, 13)
        self.binv = np.asarray(binv, dtype=f).reshape(-1, 11, 11)
        self.robust, self.huber = robust, float(huber)
        self.lw = None if lw is None else np.asarray(lw, dtype=f).reshape(-1, 5)
        self.n_l = np.diff(self.lm_off)
        self.n_c = np.bincount(self.cam_idx, minlength=self.n_cams)
        self.lm = np.repeat(np.arange(len(self.n_l)), self.n_l)

    @classmethod
    def from_context(cls, ctx, obs, robust="NONE", huber=1.0):
        """After linearize_homogeneous and prepare_joint (the cameras and landmarks are the linearisation point)."""
        from povar_amd import capi
        return cls(ctx.n_cams, ctx.lm_off, ctx.cam_idx, obs, ctx.get_cameras(), ctx.get_landmarks_homogeneous(),
                   ctx.get_buffer(capi.BUF_POSE_SCALING), ctx.get_buffer(capi.BUF_JL_COL_SCALE_H), ctx.get_buffer(capi.BUF_HLL_INV),
                   ctx.get_buffer(capi.BUF_NC_HOUSEHOLDER), ctx.get_buffer(capi.BUF_B_INV_JOINT), robust, huber)


def house4(X, sign=None):
    """(w [n, 4], beta [n]) of house4 (povar_kernels_joint.hpp:48) in X's dtype; sign: +-1 per row instead of X.x >= 0."""
    nv = np.sqrt(X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1] + X[:, 2] * X[:, 2] + X[:, 3] * X[:, 3])
    sg = np.where(X[:, 0] >= 0, 1, -1) if sign is None else sign
    w = X.copy()
    w[:, 0] = X[:, 0] + sg * nv
    return w, 2 / (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2] + w[:, 3] * w[:, 3])


def _nt(w, b, a, sign=-1):
    """N^T a = a[1:] - beta (w . a) w[1:] per row (sign = +1 with |w|: the map |N|^T = |I| + beta |w| |w|^T)."""
    return a[:, 1:] + sign * (b * (w * a).sum(1))[:, None] * w[:, 1:]


def _n(w, b, g, sign=-1):
    """N g = [0; g] - beta (w[1:] . g) w per row."""
    out = sign * (b * (w[:, 1:] * g).sum(1))[:, None] * w
    out[:, 1:] += g
    return out


def ambient(prob, t):
    """N_c t per camera in long double: the basis-independent image of a tangent 11-vector per camera, [12 n_cams]."""
    return _n(prob.ncw[:, :12].astype(LD), prob.ncw[:, 12].astype(LD), np.asarray(t, dtype=np.float64).reshape(-1, 11).astype(LD)).reshape(-1)


def weights_joint(prob, px, py, pz, xm, ym, zm, u):
    """(sw, rho): sqrt of compute_error_weight's weight in long double from r = (x / z - u, y / z - v), and the relative error
    of the stored fp64 one against it (module docstring: rho_i of step 2)."""
    n = len(px)
    if prob.robust != "HUBER":  # CAUCHY: w = 1 in compute_error_weight (oracle/povar_oracle.c): nothing to round
        return np.ones(n, dtype=LD), np.zeros(n)
    f = np.float64
    uv = prob.obs.astype(LD)
    qx, qy = px / pz, py / pz
    r0, r1 = qx - uv[:, 0], qy - uv[:, 1]
    r2 = r0 * r0 + r1 * r1
    g4 = float(gam(4, u))
    az = np.abs(pz.astype(f))
    e0 = g4 * xm / az + np.abs(qx.astype(f)) * (g4 * zm / az + 2 * u) + u * np.abs(prob.obs[:, 0])
    e1 = g4 * ym / az + np.abs(qy.astype(f)) * (g4 * zm / az + 2 * u) + u * np.abs(prob.obs[:, 1])
    r2f = np.maximum(r2.astype(f), 1e-300)
    rel = (2 * (np.abs(r0.astype(f)) * e0 + np.abs(r1.astype(f)) * e1)) / r2f + float(gam(3, u))
    t2 = LD(prob.huber) ** 2
    w = np.where(r2 < t2, LD(1), LD(prob.huber) / np.sqrt(np.maximum(r2, LD(1e-300))))
    near = r2f * (1 + rel) >= float(t2)
    return np.sqrt(w), np.where(near, rel / 4 + g4, 0.0)


def evaluate_joint(prob, x, model=MODELS_H["ckh"], mutate=None, want_parts=False):
    """(t_ref, bound), both [11 n_cams]: the long-double next term B^-1 N_c^T sigma E0 sigma N_c x of the joint system and the
    componentwise bound of `model` on |t_dev - t_ref| for a device that starts from the same x (its own previous term).
    mutate: test hook (a dict) that perturbs the reference's chain -- test_rounding_bounds.py's mutations."""
    f, u = np.float64, model.u
    mutate = mutate or {}
    g1, g2, g3, g4 = (float(gam(k, u)) for k in (1, 2, 3, 4))
    nC = prob.n_cams
    x = np.asarray(x, dtype=f).reshape(nC, 11)
    wc, bc = prob.ncw[:, :12], prob.ncw[:, 12]
    wcL, bcL, wca = wc.astype(LD), bc.astype(LD), np.abs(wc)
    sig, sigL = prob.sigma, prob.sigma.astype(LD)
    # ---- z = sigma (N_c x): an 11-term dot, beta w_i wt (2), the difference, sigma
    z = sigL * _n(wcL, bcL, x.astype(LD))
    if "z" in mutate:
        z = mutate["z"](z)
    Ez = float(gam(15, u)) * sig * _n(wca, bc, np.abs(x), +1)
    c, lm = prob.cam_idx, prob.lm
    P, X = prob.cams[c].astype(LD), prob.lms[lm].astype(LD)
    Pa, Xa = np.abs(prob.cams[c]), np.abs(prob.lms[lm])
    Pr, Par = [P[:, 4 * r:4 * r + 4] for r in range(3)], [Pa[:, 4 * r:4 * r + 4] for r in range(3)]
    px, py, pz = ((Pr[r] * X).sum(1) for r in range(3))
    xm, ym, zm = ((Par[r] * Xa).sum(1) for r in range(3))
    # ---- D and its error: x, y, z are computed dots (gamma_4 of |P_r| . |X|), so a small |z| inflates through err(z) / |z|
    iz = 1 / pz
    D = [iz, -px * iz * iz, -py * iz * iz]
    az = np.abs(pz.astype(f))
    ezr = g4 * zm / az
    A = [1 / az, np.abs(px.astype(f)) / az ** 2, np.abs(py.astype(f)) / az ** 2]
    E = [A[0] * (ezr + u), A[1] * (2 * ezr + model.kd * u) + g4 * xm / az ** 2, A[2] * (2 * ezr + model.kd * u) + g4 * ym / az ** 2]
    sw, rho = weights_joint(prob, px, py, pz, xm, ym, zm, u)
    if "sw" in mutate:
        sw = mutate["sw"](sw)
    sw2 = mutate["sw2"](sw) if "sw2" in mutate else sw  # (the second of the two factors sw of either pass)
    swa = np.abs(sw.astype(f))

    def two_rows(a, Ea, am):
        """(rows, magnitudes, errors) of sw D applied to a 3-vector given with its magnitude and error: 2 values."""
        v = [sw * (D[0] * a[0] + D[1] * a[2]), sw * (D[0] * a[1] + D[2] * a[2])]
        vm = [swa * (A[0] * am[0] + A[1] * am[2]), swa * (A[0] * am[1] + A[2] * am[2])]
        Ev = [swa * (A[0] * Ea[k] + A[k + 1] * Ea[2] + E[0] * am[k] + E[k + 1] * am[2]) + (g3 + rho) * vm[k] for k in range(2)]
        return v, vm, Ev

    def three_cols(t, Et, tm):
        """sw D^T applied to a 2-vector: 3 values (hom_q without its fourth entry)."""
        v = [sw2 * D[0] * t[0], sw2 * D[0] * t[1], sw2 * (D[1] * t[0] + D[2] * t[1])]
        vm = [swa * A[0] * tm[0], swa * A[0] * tm[1], swa * (A[1] * tm[0] + A[2] * tm[1])]
        Ev = [swa * (A[0] * Et[0] + E[0] * tm[0]) + (g2 + rho) * vm[0], swa * (A[0] * Et[1] + E[0] * tm[1]) + (g2 + rho) * vm[1],
              swa * (A[1] * Et[0] + A[2] * Et[1] + E[1] * tm[0] + E[2] * tm[1]) + (g3 + rho) * vm[2]]
        return v, vm, Ev

    # ---- forward: t = sw D (Z X), v = P^T D^T (sw t)
    Z, Za, EZ = z[c], np.abs(z[c].astype(f)), Ez[c]
    d = [(X * Z[:, 4 * r:4 * r + 4]).sum(1) for r in range(3)]
    dm = [(Xa * Za[:, 4 * r:4 * r + 4]).sum(1) for r in range(3)]
    Ed = [(Xa * EZ[:, 4 * r:4 * r + 4]).sum(1) + g4 * dm[r] for r in range(3)]
    t, tm, Et = two_rows(d, Ed, dm)
    e, em, Ee = three_cols(t, Et, tm)
    v = sum(Pr[r] * e[r][:, None] for r in range(3))
    vm = sum(Par[r] * em[r][:, None] for r in range(3))
    Ev = sum(Par[r] * Ee[r][:, None] for r in range(3)) + (float(gam(model.kv, u)) + rho)[:, None] * vm
    # ---- per landmark
    nl = prob.n_l
    keep = nl > 0
    starts = prob.lm_off[:-1][keep]
    n_lms = len(nl)

    def lsum(a, dtype):
        out = np.zeros((n_lms, a.shape[1]), dtype=dtype)
        out[keep] = np.add.reduceat(a, starts, axis=0)
        return out
    U, UM, EU = lsum(v, LD), lsum(vm, f), lsum(Ev, f)
    if model.det:
        vmax = np.zeros(n_lms)
        vmax[keep] = np.maximum.reduceat(vm.max(1), starts)
        L = np.ceil(np.log2(np.maximum(nl, 1)))
        EU += (nl * 2.0 ** (L - 61) * vmax)[:, None] * (1 + 8 * U64) + U64 * UM
    sL, sa = prob.s.astype(LD), np.abs(prob.s)
    if prob.lw is None:
        lw, lb = house4(prob.lms.astype(LD), mutate["sign"](np.where(prob.lms[:, 0] >= 0, 1, -1)) if "sign" in mutate else None)
        dn = model.dn
    else:
        lw, lb, dn = prob.lw[:, :4].astype(LD), prob.lw[:, 4].astype(LD), 0.0
    lwa, lba = np.abs(lw.astype(f)), lb.astype(f)
    a, am, Ea = sL * U, sa * UM, sa * EU
    u3, u3m = _nt(lw, lb, a), _nt(lwa, lba, am, +1)
    Eu3 = _nt(lwa, lba, Ea, +1) + (float(gam(model.klm, u)) + gam(nl, u) + dn)[:, None] * u3m
    hi = prob.hi
    if "hi" in mutate:
        hi = mutate["hi"](hi)
    up = np.triu(hi)
    hs = up + np.transpose(np.triu(hi, 1), (0, 2, 1))  # (the upper triangle, as the landmark records keep it)
    asym = np.abs(hi - np.transpose(hi, (0, 2, 1)))    # (OpE0H reads all nine entries)
    ha = np.abs(hs)
    g, gm = np.einsum("lab,lb->la", hs.astype(LD), u3), np.einsum("lab,lb->la", ha, u3m)
    Eg = np.einsum("lab,lb->la", ha, Eu3) + g3 * gm + np.einsum("lab,lb->la", asym, u3m)
    G4, G4m = sL * _n(lw, lb, g), sa * _n(lwa, lba, gm, +1)
    EG4 = sa * _n(lwa, lba, Eg, +1) + (float(gam(7, u)) + dn) * G4m
    # ---- backward: q = hom_q(sw D (P G4)), Y_c += X (x) q
    G, Gm, EG = G4[lm], G4m[lm], EG4[lm]
    p = [(Pr[r] * G).sum(1) for r in range(3)]
    pm = [(Par[r] * Gm).sum(1) for r in range(3)]
    Ep = [(Par[r] * EG).sum(1) + g4 * pm[r] for r in range(3)]
    s2, s2m, Es2 = two_rows(p, Ep, pm)
    q, qm, Eq = three_cols(s2, Es2, s2m)
    y = np.stack([X[:, j] * q[m] for m in range(3) for j in range(4)], 1)
    ym_ = np.stack([Xa[:, j] * qm[m] for m in range(3) for j in range(4)], 1)
    ey = np.stack([Xa[:, j] * Eq[m] for m in range(3) for j in range(4)], 1) + g1 * ym_
    order = np.argsort(c, kind="stable")
    cs = c[order]
    cst = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]])
    here = cs[cst]
    Y, Ym, EY = np.zeros((nC, 12), dtype=LD), np.zeros((nC, 12)), np.zeros((nC, 12))
    if len(c):
        Y[here], Ym[here], EY[here] = (np.add.reduceat(w_[order], cst, axis=0) for w_ in (y, ym_, ey))
    EY += gam(prob.n_c, u)[:, None] * Ym
    # ---- the camera tail: sigma, N_c^T (nt_apply: a 12-term dot, beta w_j wy (2), the difference), the B^-1 row
    y12, y12m, Ey12 = sigL * Y, sig * Ym, sig * EY + u * sig * Ym
    if "y12" in mutate:
        y12 = mutate["y12"](y12)
    y11, y11m = _nt(wcL, bcL, y12), _nt(wca, bc, y12m, +1)
    Ey11 = _nt(wca, bc, Ey12, +1) + float(gam(15, u)) * y11m
    ba = np.abs(prob.binv)
    t_ref = np.einsum("cij,cj->ci", prob.binv.astype(LD), y11).reshape(-1)
    tm_ = np.einsum("cij,cj->ci", ba, y11m)
    bound = ((np.einsum("cij,cj->ci", ba, Ey11) + float(gam(11, u)) * tm_) * (1 + 1e-6)).reshape(-1)
    if want_parts:
        return t_ref, bound, dict(z=z, tm=tm_.reshape(-1), pz=pz, sw=sw, rho=rho)
    return t_ref, bound


def _dot(a, b):
    out = a[:, 0] * b[:, 0]
    for k in range(1, a.shape[1]):
        out = out + a[:, k] * b[:, k]
    return out


def emulate_joint(prob, x, form):
    """The next term in fp64 in the kernels' operation order.  form "ambient": e0_ck_h (ckh_project's one division, U4 summed
    in row order, N_l, s, Hll^-1 once per landmark); "jl3": e0_lpl_h / e0_lm_cached_h / OpE0H (hom_project's three divisions,
    hom_jl4, jl3_of_jl4 per observation).  Both: the stored weight's sqrt twice per pass, the camera sums in row order, then
    cam_cold_sum_binv_h's tail (CamJoint::solve, povar_kernels_cam.hpp).  (NumPy does not contract to FMAs: every product rounds.)"""
    f = np.float64
    nC = prob.n_cams
    x = np.asarray(x, dtype=f).reshape(nC, 11)
    wc, bc, sg = prob.ncw[:, :12], prob.ncw[:, 12], prob.sigma
    wt = _dot(wc[:, 1:], x)
    z = (np.concatenate([np.zeros((nC, 1)), x], 1) - (bc * wt)[:, None] * wc) * sg
    c, lm = prob.cam_idx, prob.lm
    P, X, Z = prob.cams[c], prob.lms[lm], z[c]
    Pr = [P[:, 4 * r:4 * r + 4] for r in range(3)]
    px, py, pz = (_dot(Pr[r], X) for r in range(3))
    if prob.robust == "HUBER":  # (lpl_pass_h<0> / OpLinearizeH: hom_project's residual, error_weight; the weight is stored)
        r0, r1 = px / pz - prob.obs[:, 0], py / pz - prob.obs[:, 1]
        r2 = r0 * r0 + r1 * r1
        sw = np.sqrt(np.where(r2 < prob.huber * prob.huber, 1.0, prob.huber / np.sqrt(np.maximum(r2, 1e-300))))
    else:
        sw = np.ones(len(c))
    if form == "ambient":
        D00 = 1 / pz
        iz2 = D00 * D00
        D02, D12 = -px * iz2, -py * iz2
    else:
        D00, D02, D12 = 1 / pz, -px / (pz * pz), -py / (pz * pz)
    d = [_dot(X, Z[:, 4 * r:4 * r + 4]) for r in range(3)]
    t0, t1 = sw * (D00 * d[0] + D02 * d[2]), sw * (D00 * d[1] + D12 * d[2])
    n_lms = len(prob.n_l)
    lw, lb = house4(prob.lms)
    s, hi = prob.s, prob.hi
    H = [hi[:, 0, 0], hi[:, 0, 1], hi[:, 0, 2], hi[:, 1, 1], hi[:, 1, 2], hi[:, 2, 2]]

    def hmul(r):
        return np.stack([H[0] * r[:, 0] + H[1] * r[:, 1] + H[2] * r[:, 2], H[1] * r[:, 0] + H[3] * r[:, 1] + H[4] * r[:, 2],
                         H[2] * r[:, 0] + H[4] * r[:, 1] + H[5] * r[:, 2]], 1)
    if form == "ambient":
        e0, e1, e2 = sw * D00 * t0, sw * D00 * t1, sw * (D02 * t0 + D12 * t1)
        v = Pr[0] * e0[:, None] + Pr[1] * e1[:, None] + Pr[2] * e2[:, None]
        U = np.zeros((n_lms, 4))
        np.add.at(U, lm, v)  # (row order, one rounding per add)
        a = s * U
        aw = _dot(a, lw)
        u3 = a[:, 1:] - (lb * aw)[:, None] * lw[:, 1:]
        g3 = hmul(u3)
        gw = lb * _dot(lw[:, 1:], g3)
        G4 = s * (np.concatenate([np.zeros((n_lms, 1)), g3], 1) - gw[:, None] * lw)
        G = G4[lm]
        p = [_dot(Pr[r], G) for r in range(3)]
        s0, s1 = sw * (D00 * p[0] + D02 * p[2]), sw * (D00 * p[1] + D12 * p[2])
    else:
        sl, wl, bl = s[lm], lw[lm], lb[lm]
        jl4 = [np.stack([sw * (D00 * Pr[r][:, j] + (D02, D12)[r] * Pr[2][:, j]) * sl[:, j] for j in range(4)], 1) for r in range(2)]
        jl3 = [jl4[r][:, 1:] - (bl * _dot(jl4[r], wl))[:, None] * wl[:, 1:] for r in range(2)]
        red = np.zeros((n_lms, 3))
        np.add.at(red, lm, jl3[0] * t0[:, None] + jl3[1] * t1[:, None])
        g = hmul(red)[lm]
        s0, s1 = _dot(jl3[0], g), _dot(jl3[1], g)
    q = [sw * D00 * s0, sw * D00 * s1, sw * (D02 * s0 + D12 * s1)]
    y = np.stack([X[:, j] * q[m] for m in range(3) for j in range(4)], 1)
    Y = np.zeros((nC, 12))
    np.add.at(Y, c, y)
    y12 = Y * sg
    wy = _dot(wc, y12)
    y11 = y12[:, 1:] - (bc[:, None] * wc[:, 1:]) * wy[:, None]
    out = np.zeros((nC, 11))
    for j in range(11):
        out += prob.binv[:, :, j] * y11[:, j:j + 1]
    return out.reshape(-1)


def system_joint(n_cams, lm_off, cam_idx, obs, cams, lms_h, lam, robust="NONE", huber=1.0, eps=1e-5):
    """A prepared joint system in fp64 (the roles of BUF_POSE_SCALING, BUF_JL_COL_SCALE_H, BUF_HLL_INV, BUF_NC_HOUSEHOLDER and
    BUF_B_INV_JOINT, taken as exact numbers like a context's): povar_kernels_joint.hpp's header comment in NumPy."""
    lm_off, cam_idx = np.asarray(lm_off, dtype=np.int64), np.asarray(cam_idx, dtype=np.int64)
    cams, X4 = np.asarray(cams, dtype=np.float64).reshape(-1, 12), np.asarray(lms_h, dtype=np.float64).reshape(-1, 4)
    n_l = len(lm_off) - 1
    lm = np.repeat(np.arange(n_l), np.diff(lm_off))
    P, X = cams[cam_idx].reshape(-1, 3, 4), X4[lm]
    pc = np.einsum("nij,nj->ni", P, X)
    px, py, pz = pc[:, 0], pc[:, 1], pc[:, 2]
    r2 = (px / pz - obs[:, 0]) ** 2 + (py / pz - obs[:, 1]) ** 2
    w = np.where(r2 < huber * huber, 1.0, huber / np.sqrt(np.maximum(r2, 1e-300))) if robust == "HUBER" else np.ones(len(lm))
    sw = np.sqrt(w)
    D = np.zeros((len(lm), 2, 3))
    D[:, 0, 0] = D[:, 1, 1] = 1 / pz
    D[:, 0, 2], D[:, 1, 2] = -px / pz ** 2, -py / pz ** 2
    J4 = sw[:, None, None] * np.einsum("nra,naj->nrj", D, P)
    col = np.zeros((n_l, 4))
    np.add.at(col, lm, (J4 ** 2).sum(1))
    s = 1.0 / (eps + np.sqrt(col))
    lw, lb = house4(X4)
    N = (np.eye(4)[None] - lb[:, None, None] * lw[:, :, None] * lw[:, None, :])[:, :, 1:]
    Jl3 = np.einsum("nrj,njk->nrk", J4 * s[lm][:, None, :], N[lm])
    H = np.zeros((n_l, 3, 3))
    np.add.at(H, lm, np.einsum("nra,nrb->nab", Jl3, Jl3))
    hi = np.linalg.inv(H + lam * np.eye(3)[None])
    hi = 0.5 * (hi + np.transpose(hi, (0, 2, 1)))
    Jp = np.einsum("nra,nj->nraj", sw[:, None, None] * D, X).reshape(-1, 2, 12)
    A = np.zeros((n_cams, 12, 12))
    np.add.at(A, cam_idx, np.einsum("nra,nrb->nab", Jp, Jp))
    sigma = 1.0 / (eps + np.sqrt(np.einsum("caa->ca", A)))
    nv = np.linalg.norm(cams, axis=1)
    wc = cams.copy()
    wc[:, 0] += np.where(cams[:, 0] >= 0, nv, -nv)
    bc = 2.0 / (wc * wc).sum(1)
    Nc = (np.eye(12)[None] - bc[:, None, None] * wc[:, :, None] * wc[:, None, :])[:, :, 1:]
    B = np.einsum("cai,cab,cbj->cij", Nc, sigma[:, :, None] * A * sigma[:, None, :], Nc) + lam * np.eye(11)[None]
    prob = Step2(n_cams, lm_off, cam_idx, obs, cams, X4, sigma, s, hi, np.concatenate([wc, bc[:, None]], 1), np.linalg.inv(B),
                 robust, huber)
    # the series' first term -B^-1 b, b = N_c^T sigma Jp12^T (r - Jl3 Hll^-1 Jl3^T r): where the real term sequence starts
    r = sw[:, None] * np.stack([px / pz - obs[:, 0], py / pz - obs[:, 1]], 1)
    jr = np.zeros((n_l, 3))
    np.add.at(jr, lm, np.einsum("nra,nr->na", Jl3, r))
    e = r - np.einsum("nra,na->nr", Jl3, np.einsum("lab,lb->la", hi, jr)[lm])
    b12 = np.zeros((n_cams, 12))
    np.add.at(b12, cam_idx, np.einsum("nra,nr->na", Jp, e))
    prob.t0 = -np.einsum("cij,cj->ci", prob.binv, np.einsum("cai,ca->ci", Nc, sigma * b12)).reshape(-1)
    return prob


EDGE_HUBER_H = 0.03
EDGE_LAM_H = 1e-4


def edge_problem_joint(seed=0):
    """edge_problem's graph plus one camera without observations, with step-2 state that takes the paths the step-2 kernels
    can get wrong:
      * landmarks with X.x < 0, X.x > 0 and exactly X.x = 0, each at least a tenth (house4's sign branch);
      * X_w != 1 on more than a fifth of the landmarks (un-normalised, as between apply_joint and normalize_joint);
      * cameras of unit Frobenius norm with vec(P)[0] of either sign (the N_c reflector), near twins kept near;
      * 36 landmarks of at most four observations moved (through X_w) to a depth of 1e-2 of the typical one in their first
        camera -- every observation stays valid (|z| >= 1e-5);
      * image points = projections + N(0, 0.02) noise, 5 % outliers, on the six-decimal grid: EDGE_HUBER_H splits the residuals.
    Returns (n_cams, lm_off, cam_idx, obs, cams, lms_h)."""
    n_c, lm_off, cam_idx, _, _, _ = edge_problem(seed)
    rng = np.random.default_rng(seed + 1000)
    n_twin = 30
    n_l = len(lm_off) - 1
    cams = rng.normal(size=(n_c + 1, 12))
    cams[:, 8:11] *= 0.1
    cams[:, 11] = 5 + rng.random(n_c + 1)
    cams[n_c - n_twin:n_c] = cams[4:4 + n_twin] + 1e-5 * rng.normal(size=(n_twin, 12))
    cams /= np.linalg.norm(cams, axis=1, keepdims=True)
    X = np.concatenate([rng.normal(size=(n_l, 3)), np.ones((n_l, 1))], 1)
    X[rng.random(n_l) < 0.12, 0] = 0.0
    scaled = rng.random(n_l) < 0.3
    X[scaled] *= rng.uniform(0.5, 2.0, size=(int(scaled.sum()), 1))
    lm = np.repeat(np.arange(n_l), np.diff(lm_off))
    depth = lambda: np.einsum("nj,nj->n", cams[cam_idx][:, 8:12], X[lm])
    typical = float(np.median(np.abs(depth())))
    short = np.flatnonzero((np.diff(lm_off) <= 4) & ~scaled)
    for l in rng.choice(short, 36, replace=False):
        P2 = cams[cam_idx[lm_off[l]], 8:12]
        X[l, 3] = (1e-2 * typical - P2[:3] @ X[l, :3]) / P2[3]
    pc = np.einsum("nij,nj->ni", cams[cam_idx].reshape(-1, 3, 4), X[lm])
    obs = pc[:, :2] / pc[:, 2:3] + rng.normal(scale=0.02, size=(len(lm), 2))
    obs[rng.random(len(lm)) < 0.05] += rng.normal(scale=1.0, size=(1, 2))
    obs = np.rint(obs * 1e6) / 1e6
    return n_c + 1, lm_off, cam_idx, obs, cams, X
