"""A componentwise identity for a WHOLE power-series launch (helper module of tests/test_series_bounds.py and
tests/test_gpu_series_bounds.py; not a test module).  tests/rounding_bounds.py holds ONE application of a step's term
operator to its bound; this module holds what is specific to k terms in one launch -- the resident series
(series_res / series_res_h, povar_kernels_res.hpp) or the replayed graph of per-term kernels -- where only the last term
x_k and the sum S_k can be read back.

The identity.  Let T be the step's term operator (step 1: B^-1 E0; step 2: B^-1 N_c^T sigma E0 sigma N_c) and let the
device compute x_i = T x_{i-1} + eps_i with |eps_i| <= tb(x_{i-1}) (the one-term bound: step 1
|B^-1| bound_E0 + gamma_13 |B^-1| |y|, as test_gpu_e0_bounds.test_terms_and_increment_within_bound; step 2 evaluate_joint's
own bound) and S_k = fl(sum_{i<=k} x_i) = sum x_i + delta, |delta| <= gamma_k sum |x_i| (k additions, one per term:
povar_kernels_res.hpp:253-255, :336-338).  Summing x_i = T x_{i-1} + eps_i over i = 1..k gives, from the final state alone,

    R := (S_k - x_0) - T_ref(S_k) + T_ref(x_k)  =  sum_{i=1..k} eps_i + delta - T delta
    |R| <= sum_{i=1..k} tb(x_{i-1}) + gamma_k sum |x_i| + |T|_abs (gamma_k sum |x_i|)          (componentwise)

T_ref(S_k) and T_ref(x_k) are two long-double evaluations of rounding_bounds' reference on the device's own fp64 vectors
(exact inputs).  |T|_abs v is the magnitude chain the bound modules already compute (step 1: |B^-1| times evaluate's "Ym";
step 2: evaluate_joint's "tm").  The magnitudes |x_i| inside tb and the sum come from the long-double reference series
T_ref^i x_0, which is built from x_0 alone -- never from the code under test.  Swapping them for an independent fp64 run's
own terms changes the bound by less than 1e-9 of itself on the edge graphs (test_series_bounds.py measures it): first order,
inside the (1 + 1e-6) the bound modules apply.  An error eps_j made at ANY term j enters R undamped, and the bound is
dominated by tb(x_0): a stale block, a dropped record or a sum that was not re-zeroed at term j is seen with a margin that
falls only like |x_{j-1}| / |x_0|, where a 2-norm of the increment loses it by rho^j and by the hubs' weight.

Not used: a bound carried from x_0 term by term, e_i = tb(x_{i-1}) + |T|_abs e_{i-1}.  |B^-1| reaches 1 / lambda on
under-determined cameras and |T|_abs has none of the cancellation that makes T a contraction: on the edge graphs the
carried bound grows by orders of magnitude per term (test_series_bounds.test_a_bound_carried_term_by_term_is_vacuous
prints the medians) and says nothing from the third term on.

Rounding counts of the resident body against the per-term kernels' models (povar_kernels_res.hpp):
  obs_forward    ResPose :216-218 calls ck_obs_forward, ResJoint :304-306 ckh_obs_forward<ROBUST, STRIDE>: the "fp64" and
                 "ckh" counts KF / t, e, kv.  The landmark's sum: LDS adds in arrival order, gamma_{n_l} (all observations of a
                 landmark are in ONE workgroup: res_layout.hpp).
  landmark_step  ResPose :220-225: three 3-term dots with the record's G (KG = 3, dG = 2 u64: the record of prepare_lpl);
                 ResJoint :308-310: ckh_landmark_step<STRIDE> unchanged (klm = 8, gamma_7 on the way back).
  obs_backward   :228-231 ck_obs_backward, :313-315 ckh_obs_backward: KB / the "ckh" counts; X_j q_m is an FMA into y.
  camera sum     the lane's rows, the segmented scan, one LDS add per run (:548-558), the workgroup's record (:563-564, an
                 exact copy), the owner's five groups and their sum (:584-594): one tree over the camera's n_c contributions
                 and zeros, gamma_{n_c}; yl * sigma (:595): the u64 sigma Ym of evaluate / the u y12m of evaluate_joint.
  solve          ResPose :238-256: a 12-term dot from 0 (inside gamma_13), the sum's one addition, z = s sigma (dZ = u64);
                 ResJoint :323-341: nt_apply (gamma_15), binv_row11 (gamma_11), nc_z_entry (gamma_15): cam_binv_axpy_h's.
  weights        the ONE difference: both steps read the weight the linearisation stored (:442-447) instead of recomputing
                 it.  Step 2's model already describes the stored weight (s * s and its sqrt: rel / 4 + 3.5 u <= rel / 4 +
                 gamma_4).  Step 1's "fp64" model describes ck_huber_w's recomputation; the stored one has three counts
                 more (rounding_bounds.py, rho_i "stored"): model "fp64_stored_w", used for series_res with HUBER.  With NONE
                 and CAUCHY the two models give the same bound.
"""
import numpy as np

import rounding_bounds as RB

LD = RB.LD
F = np.float64


def is_joint(prob):
    return isinstance(prob, RB.Step2)


def dim(prob):
    return 11 if is_joint(prob) else 12


def resident_model(prob):
    """The rounding model of the resident series of prob's step (module docstring: rounding counts)."""
    return RB.MODELS_H["ckh"] if is_joint(prob) else RB.MODELS["fp64_stored_w"]


def apply_ref(prob, binv, x, model):
    """(T_ref x in long double, tb(x), |T|_abs of the chain's input magnitude) for the fp64 vector x; binv: step 1's
    [n_cams, 12, 12] B^-1 (step 2 carries its own in prob)."""
    if is_joint(prob):
        t, tb, parts = RB.evaluate_joint(prob, x, model, want_parts=True)
        return t, tb, parts["tm"]
    y, by, parts = RB.evaluate(prob, x, model, want_parts=True)
    bi, ba = binv.astype(LD), np.abs(binv)
    yr = y.reshape(-1, 12)
    t = np.einsum("cij,cj->ci", bi, yr).reshape(-1)
    mul = lambda v: np.einsum("cij,cj->ci", ba, v.reshape(-1, 12)).reshape(-1)
    tb = mul(by) + float(RB.gam(13, RB.U64)) * mul(np.abs(yr.astype(F)))
    return t, tb, mul(parts["Ym"])


def reference_series(prob, binv, x0, k, model=None):
    """The long-double series x_i = T_ref x_{i-1} from the fp64 x_0 (each term rounded to fp64 where it enters the next
    evaluation: magnitudes and norms only): dict of x [k + 1] (long double), tb [k] (tb[i] = tb(x_i)), xn [k + 1] = |x_i|_2,
    sn [k + 1] = |S_i|_2, zeta [k + 1] = i |x_i| / |S_i| (the reference's q-test, LPV:209) and rel [k + 1] = |x_i| / |x_0|."""
    model = model or resident_model(prob)
    xs, tbs = [np.asarray(x0, dtype=F).astype(LD)], []
    for _ in range(k):
        t, tb, _ = apply_ref(prob, binv, xs[-1].astype(F), model)
        xs.append(t)
        tbs.append(tb)
    S = np.cumsum(np.stack(xs), axis=0)
    xn = np.array([float(np.sqrt((x * x).sum())) for x in xs])
    sn = np.array([float(np.sqrt((s * s).sum())) for s in S])
    return dict(x=xs, tb=tbs, xn=xn, sn=sn, zeta=np.arange(k + 1) * xn / sn, rel=xn / xn[0], model=model)


def expected_exit(ref, m, q_tol, r_tol):
    """(iterations, converged) of the reference's loop (oracle/povar_oracle.c: orc_solve_pose) on the reference series."""
    for i in range(1, m + 1):
        if q_tol > 0 and ref["zeta"][i] < q_tol:
            return i, True
        if r_tol > 0 and ref["rel"][i] < r_tol:
            return i, True
    return m, False


def launch_identity(prob, binv, x0, xk, Sk, k, model=None, ref=None):
    """(R, bound) of the module docstring for one launch of k terms: x0, xk, Sk are the device's fp64 vectors (start, last
    term, sum).  ref: reference_series(prob, binv, x0, >= k, model) where the caller has it already."""
    model = model or resident_model(prob)
    if ref is None:
        ref = reference_series(prob, binv, x0, k, model)
    assert len(ref["tb"]) >= k and ref["model"] is model
    tS, _, _ = apply_ref(prob, binv, np.asarray(Sk, dtype=F), model)
    tx, _, _ = apply_ref(prob, binv, np.asarray(xk, dtype=F), model)
    R = (np.asarray(Sk, dtype=F).astype(LD) - np.asarray(x0, dtype=F).astype(LD)) - tS + tx
    mag = np.sum([np.abs(x.astype(F)) for x in ref["x"][:k + 1]], axis=0)
    d = float(RB.gam(k, RB.U64)) * mag
    _, _, td = apply_ref(prob, binv, d, model)
    bound = np.sum(ref["tb"][:k], axis=0) + d + td
    return R, bound


def check(R, bound):
    """(worst |R| / bound, its index, entries over their bound)."""
    return RB.check(R, np.zeros(R.shape, dtype=LD), bound)


# ---- step 1 on the CPU: B^-1 and x_0 from the closed form (a context gives BUF_B_INV and get_term())
def _pose_rows(prob):
    """Per observation in fp64: (w, C [n, 3, 3], h~ [n, 4], P3 [n, 3, 3], A^T r [n, 3]) of the module docstring of
    rounding_bounds (C-form) at the linearisation point."""
    c, lm = prob.cam_idx, np.repeat(np.arange(len(prob.n_l)), prob.n_l)
    P = prob.cams[c].reshape(-1, 3, 4)
    h = np.concatenate([prob.lms[lm], np.ones((len(lm), 1))], 1)
    u, v = prob.obs[:, 0], prob.obs[:, 1]
    sb2, sa2 = 1.0 - prob.alpha, prob.alpha
    p = np.einsum("nij,nj->ni", P, h)
    a, b, cc, e = p[:, 0] - u * p[:, 2], p[:, 1] - v * p[:, 2], p[:, 0] - u, p[:, 1] - v
    r2 = sb2 * (a * a + b * b) + sa2 * (cc * cc + e * e)
    w = np.where(r2 < prob.huber ** 2, 1.0, prob.huber / np.sqrt(np.maximum(r2, 1e-300))) if prob.robust == "HUBER" else np.ones(len(u))
    C = np.zeros((len(u), 3, 3))
    C[:, 0, 0] = C[:, 1, 1] = 1.0
    C[:, 0, 2] = C[:, 2, 0] = -sb2 * u
    C[:, 1, 2] = C[:, 2, 1] = -sb2 * v
    C[:, 2, 2] = sb2 * (u * u + v * v)
    atr = np.stack([sb2 * a + sa2 * cc, sb2 * b + sa2 * e, -sb2 * (u * a + v * b)], 1)  # A^T r of the unweighted residual
    return w, C, h, P[:, :, :3], atr, c, lm


def pose_closed_form(prob, lam):
    """(B^-1 [n_cams, 12, 12], x_0 = B^-1 (-b)) of a Step1 in fp64: B_c = sigma (sum_i w_i C_i (x) h~ h~^T) sigma + lambda I
    (Jp^T Jp of the rows sqrt(w) A (x) h~^T, A^T A = C) and b = sigma Jp^T (r - Jl G Jl^T r), G = S Hll^-1 S."""
    w, C, h, P3, atr, c, lm = _pose_rows(prob)
    blocks = np.einsum("n,nab,ni,nj->naibj", w, C, h, h).reshape(-1, 12, 12)
    A = np.zeros((prob.n_cams, 12, 12))
    np.add.at(A, c, blocks)
    sg = prob.sigma.reshape(-1, 12)
    B = sg[:, :, None] * A * sg[:, None, :] + lam * np.eye(12)[None]
    binv = np.linalg.inv(B)
    jr = np.zeros((len(prob.n_l), 3))
    np.add.at(jr, lm, w[:, None] * np.einsum("nka,nk->na", P3, atr))
    g = np.einsum("lab,lb->la", prob.G.astype(F), jr)
    q = w[:, None] * (atr - np.einsum("nab,nb->na", C, np.einsum("nka,na->nk", P3, g[lm])))
    b = np.zeros((prob.n_cams, 12))
    np.add.at(b, c, (q[:, :, None] * h[:, None, :]).reshape(-1, 12))
    x0 = -np.einsum("cij,cj->ci", binv, sg * b).reshape(-1)
    return binv, x0


# ---- vectorised fp64 emulations of k terms with shuffled sums and mutation hooks
class _Pose:
    """One term of step 1 in the resident body's order (every product rounds: NumPy does not contract to FMAs)."""
    nco = 3

    def __init__(self, prob, binv):
        self.prob, self.binv = prob, np.asarray(binv, dtype=F)
        w, C, h, P3, _, self.c, self.lm = _pose_rows(prob)
        self.w, self.h, self.P3 = w, h, P3
        self.cu, self.cv, self.cuv = -C[:, 0, 2], -C[:, 1, 2], C[:, 2, 2]
        self.G = prob.G.astype(F)
        self.sig = prob.sigma.reshape(-1, 12)

    def z_of(self, x):
        return self.sig * np.asarray(x, dtype=F).reshape(-1, 12)

    def _wc(self, d):
        w, cu, cv, cuv = self.w, self.cu, self.cv, self.cuv
        return np.stack([w * (d[0] - cu * d[2]), w * (d[1] - cv * d[2]), w * (cuv * d[2] - cu * d[0] - cv * d[1])], 1)

    def forward(self, z):
        Z, h = z[self.c], self.h
        d = [h[:, 0] * Z[:, 4 * r] + h[:, 1] * Z[:, 4 * r + 1] + h[:, 2] * Z[:, 4 * r + 2] + Z[:, 4 * r + 3] for r in range(3)]
        a = self._wc(d)
        P3 = self.P3
        return np.stack([P3[:, 0, m] * a[:, 0] + P3[:, 1, m] * a[:, 1] + P3[:, 2, m] * a[:, 2] for m in range(3)], 1)

    def middle(self, u):
        G = self.G
        return np.stack([G[:, m, 0] * u[:, 0] + G[:, m, 1] * u[:, 1] + G[:, m, 2] * u[:, 2] for m in range(3)], 1)

    def backward(self, g):
        gl, P3, h = g[self.lm], self.P3, self.h
        e = [P3[:, k, 0] * gl[:, 0] + P3[:, k, 1] * gl[:, 1] + P3[:, k, 2] * gl[:, 2] for k in range(3)]
        q = self._wc(e)
        return (q[:, :, None] * h[:, None, :]).reshape(-1, 12)

    def tail(self, Y):
        yl = Y * self.sig
        out = np.zeros_like(yl)
        for j in range(12):
            out += self.binv[:, :, j] * yl[:, j:j + 1]
        return out.reshape(-1)


class _Joint:
    """One term of step 2: rounding_bounds.emulate_joint's "ambient" form (e0_ck_h's operator, the resident body's) in stages."""
    nco = 4

    def __init__(self, prob, binv=None):
        self.prob = prob
        c, lm = prob.cam_idx, prob.lm
        self.c, self.lm = c, lm
        P, X = prob.cams[c], prob.lms[lm]
        self.Pr = [P[:, 4 * r:4 * r + 4] for r in range(3)]
        self.X = X
        px, py, pz = (RB._dot(self.Pr[r], X) for r in range(3))
        if prob.robust == "HUBER":
            r0, r1 = px / pz - prob.obs[:, 0], py / pz - prob.obs[:, 1]
            r2 = r0 * r0 + r1 * r1
            self.sw = np.sqrt(np.where(r2 < prob.huber * prob.huber, 1.0, prob.huber / np.sqrt(np.maximum(r2, 1e-300))))
        else:
            self.sw = np.ones(len(c))
        self.D00 = 1 / pz
        iz2 = self.D00 * self.D00
        self.D02, self.D12 = -px * iz2, -py * iz2
        self.lw, self.lb = RB.house4(prob.lms)

    def z_of(self, x):
        p = self.prob
        x = np.asarray(x, dtype=F).reshape(-1, 11)
        wc, bc = p.ncw[:, :12], p.ncw[:, 12]
        wt = RB._dot(wc[:, 1:], x)
        return (np.concatenate([np.zeros((p.n_cams, 1)), x], 1) - (bc * wt)[:, None] * wc) * p.sigma

    def _q(self, s0, s1):
        sw, D00, D02, D12 = self.sw, self.D00, self.D02, self.D12
        return [sw * D00 * s0, sw * D00 * s1, sw * (D02 * s0 + D12 * s1)]

    def _t(self, d):
        sw, D00, D02, D12 = self.sw, self.D00, self.D02, self.D12
        return sw * (D00 * d[0] + D02 * d[2]), sw * (D00 * d[1] + D12 * d[2])

    def forward(self, z):
        Z = z[self.c]
        t0, t1 = self._t([RB._dot(self.X, Z[:, 4 * r:4 * r + 4]) for r in range(3)])
        e = self._q(t0, t1)
        return self.Pr[0] * e[0][:, None] + self.Pr[1] * e[1][:, None] + self.Pr[2] * e[2][:, None]

    def middle(self, U):
        p, lw, lb = self.prob, self.lw, self.lb
        hi = p.hi
        H = [hi[:, 0, 0], hi[:, 0, 1], hi[:, 0, 2], hi[:, 1, 1], hi[:, 1, 2], hi[:, 2, 2]]
        a = p.s * U
        u3 = a[:, 1:] - (lb * RB._dot(a, lw))[:, None] * lw[:, 1:]
        g3 = np.stack([H[0] * u3[:, 0] + H[1] * u3[:, 1] + H[2] * u3[:, 2], H[1] * u3[:, 0] + H[3] * u3[:, 1] + H[4] * u3[:, 2],
                       H[2] * u3[:, 0] + H[4] * u3[:, 1] + H[5] * u3[:, 2]], 1)
        gw = lb * RB._dot(lw[:, 1:], g3)
        return p.s * (np.concatenate([np.zeros((len(lb), 1)), g3], 1) - gw[:, None] * lw)

    def backward(self, G4):
        G = G4[self.lm]
        s0, s1 = self._t([RB._dot(self.Pr[r], G) for r in range(3)])
        q = self._q(s0, s1)
        return np.stack([self.X[:, j] * q[m] for m in range(3) for j in range(4)], 1)

    def tail(self, Y):
        p = self.prob
        wc, bc = p.ncw[:, :12], p.ncw[:, 12]
        y12 = Y * p.sigma
        y11 = y12[:, 1:] - (bc[:, None] * wc[:, 1:]) * RB._dot(wc, y12)[:, None]
        out = np.zeros((p.n_cams, 11))
        for j in range(11):
            out += p.binv[:, :, j] * y11[:, j:j + 1]
        return out.reshape(-1)


MUTATIONS = ("stale_z", "drop_obs", "drop_record", "no_rezero", "stale_record")


def emulate_series(prob, binv, x0, k, seed=0, mutate=None, prior=None):
    """k terms from x_0 in fp64, the landmark sums and the camera sums each in a seeded random order (np.add.at adds in
    index order, one rounding per add).  Returns dict(xk, Sk, terms [k + 1], state); state = what the launch leaves behind
    (z table, landmark slots, per-observation backward contributions of the last term): pass it as `prior` to a second run
    and a mutation at term 1 finds what a REPLAYED launch would find there.

    mutate: dict(kind=..., term=j, ...) -- one defect of a resident launch at term j (1 <= j <= k):
      stale_z       cam: the z block of camera `cam` that term j reads is the one of term j - 1 (from x_{j-2}; at j = 1 the
                    table's content before the launch: prior's z, or zeros)
      drop_obs      obs: the backward contribution of observation `obs` does not reach its camera's sum
      drop_record   cam, lms=(l0, l1): every contribution of `cam` from landmarks l0 <= l < l1 is missing (one workgroup's
                    partial record)
      stale_record  cam, lms: those contributions are term j - 1's (the record slot was not overwritten)
      no_rezero     the landmark slots were not zeroed after term j - 1: its sums start from what the slots held, g of term
                    j - 1 (landmark_step overwrites u with g in place, povar_kernels_res.hpp:220-225, :308-310)."""
    emu = (_Joint if is_joint(prob) else _Pose)(prob, binv)
    rng = np.random.default_rng(seed)
    c, lm = emu.c, emu.lm
    n_l = len(prob.n_l)
    x = np.asarray(x0, dtype=F).copy()
    S = x.copy()
    zs = [prior["z"] if prior else np.zeros((prob.n_cams, 12)), emu.z_of(x)]
    g_prev = prior["g"] if prior else None
    y_prev = prior["y"] if prior else None
    terms = [x]
    for i in range(1, k + 1):
        m = mutate if mutate and mutate["term"] == i else None
        kind = m["kind"] if m else None
        assert kind is None or kind in MUTATIONS
        z = zs[i]
        if kind == "stale_z":
            z = z.copy()
            z[m["cam"]] = zs[i - 1][m["cam"]]
        v = emu.forward(z)
        u = np.zeros((n_l, emu.nco)) if kind != "no_rezero" else g_prev.copy()
        order = rng.permutation(len(c))
        np.add.at(u, lm[order], v[order])
        g = emu.middle(u)
        y = emu.backward(g)
        ym = y
        if kind == "drop_obs":
            ym = y.copy()
            ym[m["obs"]] = 0
        elif kind in ("drop_record", "stale_record"):
            rows = (c == m["cam"]) & (lm >= m["lms"][0]) & (lm < m["lms"][1])
            assert rows.any()
            ym = y.copy()
            ym[rows] = 0 if kind == "drop_record" else y_prev[rows]
        Y = np.zeros((prob.n_cams, 12))
        order = rng.permutation(len(c))
        np.add.at(Y, c[order], ym[order])
        x = emu.tail(Y)
        S = S + x
        zs.append(emu.z_of(x))
        g_prev, y_prev = g, y
        terms.append(x)
    return dict(xk=x, Sk=S, terms=terms, state=dict(z=zs[-1], g=g_prev, y=y_prev))
