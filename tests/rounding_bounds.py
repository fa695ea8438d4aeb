"""Componentwise rounding-error bounds for the step-1 E0 kernels: a long-double reference of each kernel's own factorisation
and, from the same chain run on absolute values, a bound on |y_dev - y_ref| for EVERY output entry (helper module of
tests/test_rounding_bounds.py and tests/test_gpu_e0_bounds.py; not a test module).

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
numbers (the device's Hll^-1 differs from the oracle's by 1e-10 at venice size, far above any fp64 rounding bound).  The
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
                 dsb2=None, chunk32=False, det=False, eta=2.0 ** -1074):
        self.name, self.u, self.form = name, u, form
        self.u_lm = u if u_lm is None else u_lm
        self.kf, self.kg, self.kb = kf, kg, kb
        self.dz, self.dh, self.dp, self.dg, self.duv = dz, dh, dp, dg, duv
        self.dsb2 = float(gam(4, U64)) if dsb2 is None else dsb2
        self.dc = self.dsb2 + 2 * duv + float(gam(3, u))
        self.chunk32, self.det, self.eta = chunk32, det, eta


MODELS = {
    # e0_lpl, e0_ck, E0Core (lane-per-observation implicit kernels): fp64 C-form
    "fp64": Model("fp64", U64),
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
    kp = float(gam(4, model.u)) + model.dp + model.dh
    ep = [kp * m for m in Pm]
    d2 = model.duv + float(gam(2, model.u))
    ea = ep[0] + np.abs(u) * ep[2] + d2 * (ab(p[0]) + np.abs(u) * ab(p[2]))
    eb = ep[1] + np.abs(v) * ep[2] + d2 * (ab(p[1]) + np.abs(v) * ab(p[2]))
    d1 = model.duv + model.u
    ec = ep[0] + d1 * (ab(p[0]) + np.abs(u))
    ee = ep[1] + d1 * (ab(p[1]) + np.abs(v))
    fs, fa = float(sb2), float(sa2)
    r2f = np.maximum(r2.astype(f), 1e-300)
    er2 = 2 * (fs * (ab(a) * ea + ab(b) * eb) + fa * (ab(c) * ec + ab(e) * ee)) + (float(gam(4, model.u)) + model.dsb2) * r2f
    rho = er2 / (2 * r2f) + float(gam(4, model.u))
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
