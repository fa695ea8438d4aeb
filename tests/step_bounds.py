"""Componentwise rounding-error bounds for the two ENDS of an LM iteration: the cost (error_pose, error_homogeneous) and the
applied step (apply_pose with either solver type, apply_joint, normalize_joint) -- a long-double reference of every number
these stages leave behind and, from the same chain run on absolute values, a bound on |dev - ref| for EVERY camera entry,
every landmark coordinate and every scalar (helper module of tests/test_step_bounds.py and tests/test_gpu_step_bounds.py; not
a test module).  operand_bounds.py holds what linearise and prepare hand on, rounding_bounds.py the E0 kernels; the normwise
tests against the oracle see the cost as one relative scalar and the new landmarks as a relative 2-norm that the
ill-conditioned landmarks carry.  Conventions as in operand_bounds.py: LD, gam, first-order bounds with every gamma rounded
up (u = 2^-53; an FMA rounds once, so every count is an upper one) and a final factor 1 + 1e-6 (Ref.put).

Inputs are only what the caller set: graph, image points, cameras, landmarks, alpha, lambda, robust norm and threshold, eps,
solver type, Jl scaling (operand_bounds.Pose / Joint) and the increment handed to apply_*.  sigma, the Jl column scale, the
weights with their rho and the camera reflectors are the reference's own long-double values (operand_bounds.pose_operands /
joint_operands, rounding_bounds.weights / weights_joint / house4, operand_bounds.house12) and enter with their bounds E(.)
as operand perturbations; no device value is read.  No exception is made.

COST (both steps).  e = error_weight(r2) (povar_kernels.hpp:235-247) per observation, summed.
  r, step 1   pose_residual (povar_kernels.hpp:264-277): m = sb (P0j - P2j u) (the product, the difference, sb: 3), dot4 with
              h (4): seven roundings, and sb = sqrt(1 - alpha), sa = sqrt(alpha) in fp64 (set_alpha, povar_lm.hip:200-203:
              gamma_2): err(r_k) <= gamma_9 rm_k, rm_k = sb (|P0| + |u| |P2|) . |h| (rows 2, 3: sa (|P0| . |h| + |u|), fewer
              roundings).  OpError :745-765 and lpl_pass<1> (povar_kernels_lpl.hpp:477-556) share it.
  r, step 2   hom_project (povar_kernels_joint.hpp:25-35): r0 = x / z - u with rounding_bounds.weights_joint's err(x / z):
              err(r0) <= gamma_4 xm / |z| + |x / z| (gamma_4 zm / |z| + 2 u) + u |u|.  OpErrorH :86-101, lpl_pass_h<1> (povar_kernels_lpl.hpp:565-634).
  r2          a sum of four (two) squares: E(r2) = 2 sum |r_k| err(r_k) + gamma_4 r2 (gamma_3 in step 2).
  NONE        e = 0.5 r2: exact scaling.
  HUBER       w = r2 < t^2 ? 1 : t / sqrt(r2), e = 0.5 (2 - w) w r2 = t sqrt(r2) - t^2 / 2 on the outlier branch: continuous
              with de / dr2 = w / 2 <= 1 / 2.  Inlier: 0.5 * 1 * 1 * r2 is exact.  Outlier: t t (1; only in the comparison),
              the root and the division (w: 2, entering e through r2 (1 - w) dw <= 2 e gamma_2), 2 - w (1), three products
              (3): gamma_8 e.  Where |r2 - t^2| <= E(r2) the device may take the other branch: there the derivative is taken
              as 1 / 2, gamma_8 e is charged, and the difference of the two branches at the device's r2,
              0.5 (sqrt(r2') - t)^2 <= 0.5 (E(r2) / t)^2, is added.
  CAUCHY      e = log(1.0 + r2): the rounding of 1 + r2 is an absolute term u (1 + r2) on the argument, so
              E(e) = (E(r2) + u (1 + r2)) / (1 + r2) + gamma_2 |e| (the device's log is taken as accurate to two roundings of
              its result: the one assumption about a library function).
  |r|         sqrt(r2): E = E(r2) / (2 sqrt(r2)) + u sqrt(r2).
  the sums    per lane, block_sum, reduce_partials / launch_reduce (povar_lm.hip:46-50): n_obs summands in some tree:
              sum_i E(e_i) + gamma_{n_obs} sum |e_i| for all_error and *_residual_sum alike.  Counts are exact.
  valid_*     the observations with |z| >= 1e-5 (hom_project :33).  err(z) = gamma_4 zm; the helper asserts that no
              observation has ||z| - 1e-5| <= err(z), so the classification follows from the inputs.

APPLIED STEP, step 1, POWER_VARPROJ (OpBackVarproj povar_kernels.hpp:1462-1524, backsub_lpl = backsub_lpl_body
povar_kernels_lpl.hpp:853-901 with LplPose :324-388, cam_apply_inc mode 0 povar_kernels.hpp:1931-1945).
  cameras     s = inc sigma (1), P_new = P + s (1): E(P_new) = |inc| E(sigma) + u |inc sigma| + u |P_new|.
  inc'        (inc sigma) (1 / sigma): inc itself in exact arithmetic whatever sigma is; three roundings: gamma_3 |inc|.
  rows        pose_jl with scale 1 and s = 1 at P_new (:280-295): a = P0j - u P2j carries E(P_new) through
              Ea = E(P0j) + |u| E(P2j), am = |P0j| + |u| |P2j|; cb = sb 1.0, cb a, times 1.0 and sb's gamma_2: at most six
              roundings: ejl = sb (Ea + gamma_6 am) (rows 2, 3: sa (E(P0j) + gamma_6 |P0j|)).  The residual at (P_new, x):
              err(r_k) = sb (E(P0) + |u| E(P2)) . |h| + gamma_9 rm_k.
  H, g        H = sum jl^T jl, g = sum jl^T r over the 4 n_l rows in any order (registers, seg_reduce_steps :348, lm_long):
              E(H)_ab = sum (|jl_a| ejl_b + |jl_b| ejl_a) + gamma_{4 n_l + 1} sum |jl_a| |jl_b|, E(g) alike with err(r).
  x_new       delta = -inv3(H) g through operand_bounds.inv3_bound: E(delta) = |Hi| E(g) + E(Hi) |g| + gamma_3 |Hi| |g|;
              x_new = x + delta: E = E(delta) + u |x_new|.  The bound scales with each landmark's own cancellation; no
              condition number appears and no landmark is left out.  inv3_bound's first-order condition is asserted at P_new.
  l_diff      - sum ji (0.5 ji + r_i), ji = Jp_fresh inc' + Jl_stored delta: the reference's mixture of scaled and unscaled
              quantities, as the kernels state it: Jp_fresh = pose_jp_x (:298-305) at the landmark BEFORE
              the update with scale 1 (unweighted): d_k = h . inc'_k (E = |h| . E(inc') + gamma_4 dm), t = sb (d0 - u d2)
              (gamma_6 with sb); Jl_stored = the weighted, column-scaled rows of the linearisation point with ejl of
              operand_bounds (gamma_8 + rho + E(s) / s); r_i = sqrt(w) res at the linearisation point ((gamma_10 + rho) rm).
              ji: three products and three sums: gamma_4; v = 0.5 ji + r (1), ji v (1).  The sum of the 4 n_obs terms in
              any tree: sum E(term) + gamma_{4 n_obs} sum |term|.
              The update's error enters ji as jl . d(delta), and |jl| E(delta) would charge a near-parallel landmark's
              weak direction to rows that do not see it (1e-4 of l_diff on the edge graph).  To first order
              d(delta) = -Hi dg - Hi dH delta - rho g with rho = inv3's own roundings on exact input, whose determinant
              part is a scalar factor eps of Hi (|eps| <= E0(det) / |det|, inv3_bound with E(H) = 0), so
                  |jl . d(delta)| <= |jl Hi| E(g) + |jl Hi| E(H) |delta| + |jl| (E0(Hi) - |Hi| E0(det) / |det| + gamma_3 |Hi|) |g|
                                     + (E0(det) / |det|) |jl . delta|
              with jl Hi formed in long double before the absolute value (_Solve3.row).  In step 2 jl4 . N_l d(delta3) =
              jl3 . d(delta3) with the reference's jl3, and the lift's own roundings stay entrywise.

APPLIED STEP, step 1, POWER_SCHUR_COMPLEMENT (OpBackPoba :2018-2081, cam_apply_inc modes 1 and 2).  Stored weighted, scaled
rows at the linearisation point (ejl as above).  z = sigma inc: E(z) = |inc| E(sigma) + u |z|.  jpi = pose_jp_x with scale
sqrt(w): (gamma_7 + rho) on sb sw (|d0| + |u| |d2|).  a = r + jpi (1), g = sum jl^T a, H + lambda I (E(H) as HLL_INV in
operand_bounds), delta = -inv3 g, x_new = x + s delta: E = s E(delta) + |delta| E(s) + u |s delta| + u |x_new|.  Cameras:
P + z, two roundings.  l_diff with ji = jpi + jl delta, r the stored weighted residual.

APPLIED STEP, step 2 (OpBackJoint povar_kernels_joint.hpp:231-279, backsub_lpl_h = backsub_lpl_body
povar_kernels_lpl.hpp:853-901 with LplJoint :390-453, cam_apply_inc_h povar_kernels_joint.hpp:662-677).
  z           p = N_c inc = [0; inc] - beta w (w[1:] . inc): an 11-term dot, two products, the difference: gamma_14, and the
              device's reflector against the reference's long-double one, dNc = gamma_45 (operand_bounds): E(p) =
              (gamma_14 + dNc) |N_c| |inc|; z = p sigma: E(z) = sigma E(p) + |p| E(sigma) + u |z|.  P_new = P + z: u |P_new|.
  jpi         hom_jp_x (:65-69) with scale sqrt(w): d_k = X . z_k (gamma_4), t0 = sw (D00 d0 + D02 d2) with the magnitudes A
              and errors E00, E02, E12 of operand_bounds: gamma_3 + rho on the magnitude.
  jl3, H3, g3 as HLL_INV and B_JOINT of operand_bounds (jl4 with the reference's s, N_l from long-double house4, dN =
              gamma_25), with a = r + jpi in place of r.
  X_new       delta3 = -hinv_damped(H3, lambda) g3; delta4 = N_l delta3 (delta4 :246-259: a three-term dot, two products, the
              difference: gamma_6 + dN on |N_l| |delta3|); X_new = X + s delta4 as in POWER_SCHUR_COMPLEMENT.
  l_diff      ji = jpi + jl4 . delta4 (gamma_5), two rows per observation: gamma_{2 n_obs} for the sum.

normalize_joint (:1148-1169).  X / X_w: one division per coordinate (u |X / X_w|), X_w / X_w exactly 1.  P / |P|_F: a 12-term
sum of squares (gamma_12, halved by the root), the root, the division: gamma_8 |P / |P|_F|.

Conditions, asserted here: inv3_bound's E(det) < 2^-10 |det| for every landmark where H is formed (P_new for POWER_VARPROJ);
the |z| gap above; nothing is excluded anywhere.  The margins measured on the edge graphs are recorded in
tests/test_step_bounds.py, with the slack and the detectable scales.
"""
import numpy as np

import operand_bounds as OB
import rounding_bounds as RB
from operand_bounds import LD, Joint, Pose, Ref, csum, g, gam, house12, inv3_bound, lsum, report  # noqa: F401
from rounding_bounds import house4, weights, weights_joint

F = np.float64
U64 = RB.U64
_f, _ab = OB._f, OB._ab
Z_VALID = 1e-5


def _model(u):
    return OB.FP64 if u == U64 else RB.MODELS["longdouble"]


def _with(p, **kw):
    """A copy of the problem with other cameras / landmarks (the state read back after an apply)."""
    import copy
    q = copy.copy(p)
    for k, v in kw.items():
        setattr(q, k, np.asarray(v, dtype=F).reshape(getattr(p, k).shape))
    return q


# ======== cost
def _error(robust, t, r2, Er2, u):
    """(e, E(e)) of error_weight per observation (module docstring: NONE / HUBER / CAUCHY)."""
    r2f = _f(r2)
    if robust == "HUBER":
        t = LD(t)
        t2 = t * t
        rs = np.sqrt(r2)
        inl = r2 < t2
        near = np.abs(r2f - float(t2)) <= Er2
        e = np.where(inl, LD(0.5) * r2, t * rs - LD(0.5) * t2)
        w = np.where(inl, 1.0, float(t) / np.maximum(_f(rs), 1e-300))
        Ee = 0.5 * np.where(near, 1.0, w) * Er2 + np.where(inl & ~near, 0.0, g(8, u) * _ab(e)) + np.where(near, 0.5 * (Er2 / float(t)) ** 2, 0.0)
        return e, Ee
    if robust == "CAUCHY":
        e = np.log1p(r2)
        return e, (Er2 + u * (1 + r2f)) / (1 + r2f) + g(2, u) * _ab(e)
    return LD(0.5) * r2, 0.5 * Er2


def _sums(R, names, e, Ee, rs, Ers, keep, u):
    n = int(keep.sum())
    k = lambda a: np.where(keep, a, a.dtype.type(0))
    R.put(names[0], [k(e).sum()], [k(Ee).sum() + g(max(n, 1), u) * k(_ab(e)).sum()])
    R.put(names[1], [k(rs).sum()], [k(Ers).sum() + g(max(n, 1), u) * k(_f(rs)).sum()])
    R.aux[names[2]] = n


def _pose_geometry(p, P, EP, u):
    """Per observation at the cameras P [n, 12] (long double, |dP| <= EP) and p's landmarks: the unweighted residual rows
    (r, E(r), rm) and the unweighted, unscaled Jl rows (a [4][n, 3], E(a), am) -- module docstring: r step 1, rows."""
    sb2, sa2 = LD(1) - LD(p.alpha), LD(p.alpha)
    sb, sa = np.sqrt(sb2), np.sqrt(sa2)
    fsb, fsa = float(sb), float(sa)
    X, Xa = p.lms[p.lm].astype(LD), np.abs(p.lms[p.lm])
    Pa = _ab(P)
    U, V = p.obs[:, 0].astype(LD), p.obs[:, 1].astype(LD)
    Ua, Va = np.abs(p.obs[:, 0]), np.abs(p.obs[:, 1])
    dot = lambda M, k, h: M[:, 4 * k] * h[:, 0] + M[:, 4 * k + 1] * h[:, 1] + M[:, 4 * k + 2] * h[:, 2] + M[:, 4 * k + 3]
    pk, Pm, dP = [dot(P, k, X) for k in range(3)], [dot(Pa, k, Xa) for k in range(3)], [dot(EP, k, Xa) for k in range(3)]
    r = [sb * (pk[0] - U * pk[2]), sb * (pk[1] - V * pk[2]), sa * (pk[0] - U), sa * (pk[1] - V)]
    rm = [fsb * (Pm[0] + Ua * Pm[2]), fsb * (Pm[1] + Va * Pm[2]), fsa * (Pm[0] + Ua), fsa * (Pm[1] + Va)]
    Er = [fsb * (dP[0] + Ua * dP[2]) + g(9, u) * rm[0], fsb * (dP[1] + Va * dP[2]) + g(9, u) * rm[1],
          fsa * dP[0] + g(9, u) * rm[2], fsa * dP[1] + g(9, u) * rm[3]]
    P3 = [P[:, 4 * k:4 * k + 3] for k in range(3)]
    P3a = [Pa[:, 4 * k:4 * k + 3] for k in range(3)]
    E3 = [EP[:, 4 * k:4 * k + 3] for k in range(3)]
    a = [sb * (P3[0] - U[:, None] * P3[2]), sb * (P3[1] - V[:, None] * P3[2]), sa * P3[0], sa * P3[1]]
    am = [fsb * (P3a[0] + Ua[:, None] * P3a[2]), fsb * (P3a[1] + Va[:, None] * P3a[2]), fsa * P3a[0], fsa * P3a[1]]
    Ea = [fsb * (E3[0] + Ua[:, None] * E3[2]), fsb * (E3[1] + Va[:, None] * E3[2]), fsa * E3[0], fsa * E3[1]]
    return dict(r=r, Er=Er, rm=rm, a=a, am=am, Ea=Ea, sb=sb, sa=sa, U=U, V=V, Ua=Ua, Va=Va, X=X, Xa=Xa)


def cost_pose(p, mutate=None, u=U64):
    """Ref of all_error, all_residual_sum [1] and aux all_num_obs of error_pose at p's cameras and landmarks.  mutate:
      drop_cost: observation indices left out of the sums        old_lm: (landmark indices, their old coordinates [k, 3])."""
    mutate = mutate or {}
    if "old_lm" in mutate:
        lms = p.lms.copy()
        lms[np.asarray(mutate["old_lm"][0])] = mutate["old_lm"][1]
        p = _with(p, lms=lms)
    n = len(p.cam_idx)
    G = _pose_geometry(p, p.cams[p.cam_idx].astype(LD), np.zeros((n, 12)), u)
    r2 = sum(t * t for t in G["r"])
    Er2 = 2 * sum(_ab(t) * e for t, e in zip(G["r"], G["Er"])) + g(4, u) * _f(r2)
    e, Ee = _error(p.robust, p.huber, r2, Er2, u)
    rs = np.sqrt(r2)
    Ers = Er2 / np.maximum(2 * _f(rs), 1e-300) + u * _f(rs)
    keep = np.ones(n, dtype=bool)
    if "drop_cost" in mutate:
        keep[np.asarray(mutate["drop_cost"])] = False
    R = Ref()
    _sums(R, ("all_error", "all_residual_sum", "all_num_obs"), e, Ee, rs, Ers, keep, u)
    R.aux.update(e=e, Ee=Ee)
    return R


def _hom_geometry(p, u):
    """operand_bounds.joint_operands' per-observation quantities at p's cameras and landmarks."""
    c, lm = p.cam_idx, p.lm
    g4 = g(4, u)
    P, X = p.cams[c].astype(LD), p.lms[lm].astype(LD)
    Pa, Xa = np.abs(p.cams[c]), np.abs(p.lms[lm])
    Pr, Par = [P[:, 4 * r:4 * r + 4] for r in range(3)], [Pa[:, 4 * r:4 * r + 4] for r in range(3)]
    px, py, pz = ((Pr[r] * X).sum(1) for r in range(3))
    xm, ym, zm = ((Par[r] * Xa).sum(1) for r in range(3))
    az = _ab(pz)
    gap = np.abs(az - Z_VALID)
    assert (gap > g4 * zm).all(), ("an observation's |z| is within err(z) of 1e-5", float((gap / (g4 * zm)).min()))
    ezr = g4 * zm / az
    D = [1 / pz, -px / (pz * pz), -py / (pz * pz)]
    A = [1 / az, _ab(px) / az ** 2, _ab(py) / az ** 2]
    E = [A[0] * (ezr + u), A[1] * (2 * ezr + 2 * u) + g4 * xm / az ** 2, A[2] * (2 * ezr + 2 * u) + g4 * ym / az ** 2]
    uv = p.obs.astype(LD)
    qx, qy = px / pz, py / pz
    r = [qx - uv[:, 0], qy - uv[:, 1]]
    e0 = [g4 * xm / az + _ab(qx) * (ezr + 2 * u) + u * np.abs(p.obs[:, 0]), g4 * ym / az + _ab(qy) * (ezr + 2 * u) + u * np.abs(p.obs[:, 1])]
    return dict(P=P, X=X, Pa=Pa, Xa=Xa, Pr=Pr, Par=Par, px=px, py=py, pz=pz, xm=xm, ym=ym, zm=zm, az=az, D=D, A=A, E=E, r=r, e0=e0,
                z_gap=float((gap / (g4 * zm)).min()))


def cost_joint(p, mutate=None, u=U64):
    """Ref of all_error, all_residual_sum, valid_error, valid_residual_sum [1] and aux all_num_obs, valid_num_obs, z_gap of
    error_homogeneous at p's cameras and homogeneous landmarks.  mutate: as cost_pose."""
    mutate = mutate or {}
    if "old_lm" in mutate:
        lms = p.lms.copy()
        lms[np.asarray(mutate["old_lm"][0])] = mutate["old_lm"][1]
        p = _with(p, lms=lms)
    n = len(p.cam_idx)
    G = _hom_geometry(p, u)
    r2 = G["r"][0] * G["r"][0] + G["r"][1] * G["r"][1]
    Er2 = 2 * (_ab(G["r"][0]) * G["e0"][0] + _ab(G["r"][1]) * G["e0"][1]) + g(3, u) * _f(r2)
    e, Ee = _error(p.robust, p.huber, r2, Er2, u)
    rs = np.sqrt(r2)
    Ers = Er2 / np.maximum(2 * _f(rs), 1e-300) + u * _f(rs)
    keep = np.ones(n, dtype=bool)
    if "drop_cost" in mutate:
        keep[np.asarray(mutate["drop_cost"])] = False
    R = Ref()
    _sums(R, ("all_error", "all_residual_sum", "all_num_obs"), e, Ee, rs, Ers, keep, u)
    _sums(R, ("valid_error", "valid_residual_sum", "valid_num_obs"), e, Ee, rs, Ers, keep & (G["az"] >= Z_VALID), u)
    R.aux.update(e=e, Ee=Ee, z_gap=G["z_gap"])
    return R


COST_FIELDS = {1: ("all_error", "all_residual_sum"), 2: ("all_error", "all_residual_sum", "valid_error", "valid_residual_sum")}
COUNT_FIELDS = {1: ("all_num_obs",), 2: ("all_num_obs", "valid_num_obs")}


def cost(p, mutate=None, u=U64):
    return cost_joint(p, mutate, u) if isinstance(p, Joint) else cost_pose(p, mutate, u)


def cost_check(R, ri, step):
    """[(field, err / bound, over)] of a ResidualInfo-like object (attributes) against R; the counts must match exactly."""
    out = []
    for k in COUNT_FIELDS[step]:
        assert int(getattr(ri, k)) == R.aux[k], (k, int(getattr(ri, k)), R.aux[k])
    if step == 1:
        assert int(ri.valid_num_obs) == R.aux["all_num_obs"]
    for k in COST_FIELDS[step]:
        r, _, over = RB.check(np.array([getattr(ri, k)]), R.ref[k], R.bound[k])
        out.append((k, r, over))
    return out


# ======== the applied step
class _Solve3:
    """delta = -inv3(H + lam I) g per landmark with its entrywise bound E(delta) (module docstring: x_new), and row(jl): a
    bound on |jl . (delta_dev - delta)| per observation row that keeps the structure of the error (module docstring:
    l_diff).  The first-order condition is asserted by inv3_bound."""

    def __init__(self, p, H, EH, Hm, gl, Eg, gm, lam, u):
        if lam:
            H = H + LD(lam) * np.eye(3, dtype=LD)[None]
            EH = EH + u * (Hm + lam) * np.eye(3)[None]
        Hi, EHi, self.ratio = inv3_bound(H, EH, u)
        _, EHi0, ratio0 = inv3_bound(H, np.zeros_like(EH), u)
        Hia, ga = _ab(Hi), _ab(gl)
        self.d = -np.einsum("lab,lb->la", Hi, gl)
        self.Ed = np.einsum("lab,lb->la", Hia, Eg) + np.einsum("lab,lb->la", EHi, ga) + g(3, u) * np.einsum("lab,lb->la", Hia, ga)
        self.lm, self.Hi, self.EH, self.Eg, self.ga, self.ratio0 = p.lm, Hi, EH, Eg, ga, ratio0
        # inv3's own roundings on exact input: the determinant's part is a scalar factor of Hi, the rest is entrywise
        self.Eun = np.maximum(EHi0 - Hia * ratio0[:, None, None], 0.0) + g(3, u) * Hia

    def row(self, jl):
        lm = self.lm
        jH = _ab(np.einsum("na,nab->nb", jl, self.Hi[lm]))
        return ((jH * self.Eg[lm]).sum(1) + np.einsum("na,nab,nb->n", jH, self.EH[lm], _ab(self.d)[lm])
                + np.einsum("na,nab,nb->n", _ab(jl), self.Eun[lm], self.ga[lm]) + self.ratio0[lm] * _ab((jl * self.d[lm]).sum(1)))


def _gram(p, jl, ejl, rr, Err, nrow, u, drop_g=None):
    """H, E(H), |H| sums, g, E(g), |g| sums of the rows jl [k][n, 3] with right-hand rows rr [k][n] (module docstring: H, g)."""
    jla, ra = [_ab(t) for t in jl], [_ab(t) for t in rr]
    cnt = g(nrow * p.n_l + 1, u)
    H = lsum(p, sum(t[:, :, None] * t[:, None, :] for t in jl))
    Hm = lsum(p, sum(t[:, :, None] * t[:, None, :] for t in jla))
    EH = lsum(p, sum(t[:, :, None] * e[:, None, :] + e[:, :, None] * t[:, None, :] for t, e in zip(jla, ejl))) + cnt[:, None, None] * Hm
    kg = np.ones(len(p.cam_idx), dtype=bool)
    if drop_g is not None:
        kg[np.asarray(drop_g)] = False
    gl = lsum(p, np.where(kg[:, None], sum(j * t[:, None] for j, t in zip(jl, rr)), LD(0)))
    gm = lsum(p, sum(j * t[:, None] for j, t in zip(jla, ra)))
    Eg = lsum(p, sum(j * e[:, None] + ej * t[:, None] for j, e, ej, t in zip(jla, Err, ejl, ra))) + cnt[:, None] * gm
    return H, EH, Hm, gl, Eg, gm


def _ldiff(R, p, parts, rr, Err, nrow, kj, u, drop_l=None):
    """l_diff = -sum ji (0.5 ji + r): parts = [(jpi_k, E(jpi_k), jl_k [n, m], ejl_k, delta [n, m], E(jl_k . d delta) [n])] per
    row of the observations."""
    tot, Et, ta = LD(0), 0.0, 0.0
    keep = np.ones(len(p.cam_idx), dtype=bool)
    if drop_l is not None:
        keep[np.isin(p.lm, np.asarray(drop_l))] = False
    terms, Eterms = [], []
    for (jp, Ejp, jl, ejl, d, Ejd), r, Er in zip(parts, rr, Err):
        ji = jp + (jl * d).sum(1)
        Eji = Ejp + Ejd + (ejl * _ab(d)).sum(1) + g(kj, u) * (_ab(jp) + (_ab(jl) * _ab(d)).sum(1))
        v = LD(0.5) * ji + r
        Ev = 0.5 * Eji + Er + u * (0.5 * _ab(ji) + _ab(r))
        t = ji * v
        Eterms.append(_ab(ji) * Ev + _ab(v) * Eji + u * _ab(t))
        terms.append(np.where(keep, t, LD(0)))
        tot = tot + terms[-1].sum()
        Et += Eterms[-1].sum()
        ta += _ab(t).sum()
    R.put("L_DIFF", [-tot], [Et + g(nrow * len(p.cam_idx), u) * ta])
    R.aux["ldiff_terms"], R.aux["ldiff_Eterms"] = -sum(terms), sum(Eterms)


def _stored_pose(p, R0, G, mutate, u):
    """The stored (weighted, column-scaled) Jl rows and weighted residual of the linearisation point with their bounds."""
    P = p.cams[p.cam_idx].astype(LD)
    X = G["X"]
    w, rho = weights(p, P, [X[:, 0], X[:, 1], X[:, 2]], p.obs.astype(LD), G["sb"] ** 2, G["sa"] ** 2, _model(u))
    if "w_one" in mutate:
        w = w.copy()
        w[np.asarray(mutate["w_one"])] = 1
    sw, swa = np.sqrt(w), _f(np.sqrt(w))
    s = R0.ref["JL_COL_SCALE"].reshape(-1, 3)
    Es = R0.bound["JL_COL_SCALE"].reshape(-1, 3)
    sl, sla, ds = s[p.lm], _f(s)[p.lm], (Es / _f(s))[p.lm]
    jl = [sw[:, None] * a * sl for a in G["a"]]
    ejl = [swa[:, None] * am * sla * (g(8, u) + rho[:, None] + ds) for am in G["am"]]
    rr = [sw * t for t in G["r"]]
    Err = [(g(10, u) + rho) * swa * t for t in G["rm"]]
    return dict(sw=sw, swa=swa, rho=rho, s=s, Es=Es, jl=jl, ejl=ejl, rr=rr, Err=Err)


def _jp_x_pose(G, zc, Ezc, scale, scale_a, krel, u):
    """pose_jp_x (povar_kernels.hpp:298-305): t [4][n], E(t) for the per-observation camera vector zc [n, 12], |dz| <= Ezc."""
    fsb, fsa = float(G["sb"]), float(G["sa"])
    h = np.concatenate([G["X"], np.ones((len(zc), 1), dtype=LD)], 1)
    ha = np.concatenate([G["Xa"], np.ones((len(zc), 1))], 1)
    d = [(h * zc[:, 4 * k:4 * k + 4]).sum(1) for k in range(3)]
    dm = [(ha * _ab(zc[:, 4 * k:4 * k + 4])).sum(1) for k in range(3)]
    Ed = [(ha * Ezc[:, 4 * k:4 * k + 4]).sum(1) + g(4, u) * dm[k] for k in range(3)]
    da = [_ab(t) for t in d]
    U, V, Ua, Va = G["U"], G["V"], G["Ua"], G["Va"]
    t = [G["sb"] * scale * (d[0] - U * d[2]), G["sb"] * scale * (d[1] - V * d[2]), G["sa"] * scale * d[0], G["sa"] * scale * d[1]]
    Et = [fsb * scale_a * (Ed[0] + Ua * Ed[2] + krel * (da[0] + Ua * da[2])), fsb * scale_a * (Ed[1] + Va * Ed[2] + krel * (da[1] + Va * da[2])),
          fsa * scale_a * (Ed[0] + krel * da[0]), fsa * scale_a * (Ed[1] + krel * da[1])]
    return t, Et


def apply_pose(p, inc, mutate=None, u=U64, R0=None):
    """Ref of CAMERAS [12 n_cams], LANDMARKS [3 n_lms], L_DIFF [1] after apply_pose(p.solver, alpha, inc) at p's state; aux
    det_ratio.  R0: operand_bounds.pose_operands(p) when the caller has it.  mutate (test hooks on the reference's chain):
      drop_g: observation indices left out of g                 lin_cam: cameras whose rows are taken at P instead of P_new
      no_scale: (landmark, coordinate) updated without s        w_one: observation indices whose stored weight is taken as 1
      drop_ldiff: landmarks whose terms are left out of l_diff."""
    mutate = mutate or {}
    R0 = R0 or OB.pose_operands(p, u=u)
    R = Ref()
    n, c = len(p.cam_idx), p.cam_idx
    incL = np.asarray(inc, dtype=F).reshape(-1, 12).astype(LD)
    inca = _ab(incL)
    sig, Esig = R0.ref["SIGMA"].reshape(-1, 12), R0.bound["SIGMA"].reshape(-1, 12)
    z = sig * incL
    Ez = inca * Esig + u * _ab(z)
    Pn = p.cams.astype(LD) + z
    EPn = Ez + u * _ab(Pn)
    R.put("CAMERAS", Pn.reshape(-1), EPn.reshape(-1))
    R.aux["sigma"], R.aux["Esigma"] = sig, Esig
    G0 = _pose_geometry(p, p.cams[c].astype(LD), np.zeros((n, 12)), u)
    S = _stored_pose(p, R0, G0, mutate, u)
    X = p.lms.astype(LD)
    if p.solver == "POWER_VARPROJ":
        Pc, EPc = Pn[c], EPn[c]
        if "lin_cam" in mutate:
            m = np.isin(c, np.asarray(mutate["lin_cam"]))
            Pc, EPc = np.where(m[:, None], p.cams[c].astype(LD), Pc), np.where(m[:, None], 0.0, EPc)
        G1 = _pose_geometry(p, Pc, EPc, u)
        ejl = [e + g(6, u) * am for e, am in zip(G1["Ea"], G1["am"])]
        H, EH, Hm, gl, Eg, gm = _gram(p, G1["a"], ejl, G1["r"], G1["Er"], 4, u, mutate.get("drop_g"))
        S3 = _Solve3(p, H, EH, Hm, gl, Eg, gm, 0.0, u)
        d, Ed, ratio = S3.d, S3.Ed, S3.ratio
        xn = X + d
        R.put("LANDMARKS", xn.reshape(-1), (Ed + u * _ab(xn)).reshape(-1))
        jp, Ejp = _jp_x_pose(G0, incL[c], g(3, u) * inca[c], LD(1), 1.0, g(6, u), u)
    else:
        jp, Ejp = _jp_x_pose(G0, z[c], Ez[c], S["sw"], S["swa"], g(7, u) + S["rho"], u)
        a = [r + t for r, t in zip(S["rr"], jp)]
        Ea = [er + et + u * (_ab(r) + _ab(t)) for er, et, r, t in zip(S["Err"], Ejp, S["rr"], jp)]
        H, EH, Hm, gl, Eg, gm = _gram(p, S["jl"], S["ejl"], a, Ea, 4, u, mutate.get("drop_g"))
        S3 = _Solve3(p, H, EH, Hm, gl, Eg, gm, p.lam_lm, u)
        d, Ed, ratio = S3.d, S3.Ed, S3.ratio
        s, sf = S["s"], _f(S["s"])
        sd = s * d
        if "no_scale" in mutate:
            l, k = mutate["no_scale"]
            sd = sd.copy()
            sd[l, k] = d[l, k]
        xn = X + sd
        R.put("LANDMARKS", xn.reshape(-1), (sf * Ed + _ab(d) * S["Es"] + u * _ab(sd) + u * _ab(xn)).reshape(-1))
    R.aux["det_ratio"], R.aux["delta"], R.aux["Edelta"] = ratio, d, Ed
    dl = d[p.lm]
    _ldiff(R, p, [(jp[k], Ejp[k], S["jl"][k], S["ejl"][k], dl, S3.row(S["jl"][k])) for k in range(4)], S["rr"], S["Err"], 4, 4, u,
           mutate.get("drop_ldiff"))
    return R


def _n12(w, b, x, sign=-1):
    """N_c x = [0; x] - beta (w[1:] . x) w per camera (sign = +1 with |w|, |x|: the magnitude map)."""
    out = sign * (b * (w[:, 1:] * x).sum(1))[:, None] * w
    out[:, 1:] += x
    return out


def apply_joint(p, inc, mutate=None, u=U64, R0=None):
    """Ref of CAMERAS [12 n_cams], LANDMARKS [4 n_lms], L_DIFF [1] after apply_joint(inc) at p's state; aux det_ratio, z_gap.
    mutate: drop_g, no_scale, w_one, drop_ldiff as apply_pose."""
    mutate = mutate or {}
    R0 = R0 or OB.joint_operands(p, u=u)
    R = Ref()
    c, lm = p.cam_idx, p.lm
    g2, g3, g4 = (g(k, u) for k in (2, 3, 4))
    G = _hom_geometry(p, u)
    D, A, E, Pr, Par, X, Xa = G["D"], G["A"], G["E"], G["Pr"], G["Par"], G["X"], G["Xa"]
    # ---- cameras
    inc11 = np.asarray(inc, dtype=F).reshape(-1, 11).astype(LD)
    cw, cb = house12(p.cams.astype(LD))
    dnc = R0.aux["dnc"]
    pin = _n12(cw, cb, inc11)
    pinm = _n12(_ab(cw), _f(cb), _ab(inc11), +1)
    Epin = (g(14, u) + dnc) * pinm
    sig, Esig = R0.ref["SIGMA"].reshape(-1, 12), R0.bound["SIGMA"].reshape(-1, 12)
    z = pin * sig
    Ez = _f(sig) * Epin + _ab(pin) * Esig + u * _ab(z)
    Pn = p.cams.astype(LD) + z
    R.put("CAMERAS", Pn.reshape(-1), (Ez + u * _ab(Pn)).reshape(-1))
    R.aux["sigma"], R.aux["Esigma"], R.aux["pin"], R.aux["Epin"] = sig, Esig, pin, Epin
    # ---- the stored rows (operand_bounds.joint_operands: JL SCALE H, HLL_INV, B_JOINT)
    sw, rho = weights_joint(p, G["px"], G["py"], G["pz"], G["xm"], G["ym"], G["zm"], u)
    if "w_one" in mutate:
        sw = sw.copy()
        sw[np.asarray(mutate["w_one"])] = 1
    swa = _f(sw)
    rows = [sw[:, None] * (D[0][:, None] * Pr[k] + D[k + 1][:, None] * Pr[2]) for k in range(2)]
    jm = [swa[:, None] * (A[0][:, None] * Par[k] + A[k + 1][:, None] * Par[2]) for k in range(2)]
    ej = [swa[:, None] * (E[0][:, None] * Par[k] + E[k + 1][:, None] * Par[2]) + (g4 + rho)[:, None] * jm[k] for k in range(2)]
    s, Es = R0.ref["JL_COL_SCALE_H"].reshape(-1, 4), R0.bound["JL_COL_SCALE_H"].reshape(-1, 4)
    sl, sla, ds = s[lm], _f(s)[lm], (Es / _f(s))[lm]
    lw, lb = house4(p.lms.astype(LD))
    lwa, lba, lwo, lbo = _ab(lw)[lm], _f(lb)[lm], lw[lm], lb[lm]
    dn = g(25, u)
    jl4 = [r * sl for r in rows]
    ej4 = [e * sla + (ds + u) * _ab(j) for e, j in zip(ej, jl4)]
    jl3 = [RB._nt(lwo, lbo, j) for j in jl4]
    jl3m = [RB._nt(lwa, lba, _ab(j), +1) for j in jl4]
    ejl3 = [RB._nt(lwa, lba, e, +1) + (g(8, u) + dn) * m3 for e, m3 in zip(ej4, jl3m)]
    rr = [sw * t for t in G["r"]]
    Err = [swa * e + (rho + u) * _ab(t) for e, t in zip(G["e0"], rr)]
    # ---- jpi = hom_jp_x(z)
    zc, Ezc = z[c], Ez[c]
    d = [(X * zc[:, 4 * k:4 * k + 4]).sum(1) for k in range(3)]
    dm = [(Xa * _ab(zc[:, 4 * k:4 * k + 4])).sum(1) for k in range(3)]
    Ed = [(Xa * Ezc[:, 4 * k:4 * k + 4]).sum(1) + g4 * dm[k] for k in range(3)]
    da = [_ab(t) for t in d]
    jp = [sw * (D[0] * d[k] + D[k + 1] * d[2]) for k in range(2)]
    Ejp = [swa * (A[0] * Ed[k] + E[0] * da[k] + A[k + 1] * Ed[2] + E[k + 1] * da[2]) + (g3 + rho) * swa * (A[0] * da[k] + A[k + 1] * da[2]) for k in range(2)]
    a = [r + t for r, t in zip(rr, jp)]
    Ea = [er + et + u * (_ab(r) + _ab(t)) for er, et, r, t in zip(Err, Ejp, rr, jp)]
    H, EH, Hm, gl, Eg, gm = _gram(p, jl3, ejl3, a, Ea, 2, u, mutate.get("drop_g"))
    S3 = _Solve3(p, H, EH, Hm, gl, Eg, gm, p.lam_lm, u)
    d3, Ed3, ratio = S3.d, S3.Ed, S3.ratio
    # ---- delta4 = N_l delta3, X_new
    lwf, lbf = _ab(lw), _f(lb)
    d4 = RB._n(lw, lb, d3)
    d4m = RB._n(lwf, lbf, _ab(d3), +1)
    Ed4 = RB._n(lwf, lbf, Ed3, +1) + (g(6, u) + dn) * d4m
    sd = s * d4
    if "no_scale" in mutate:
        l, k = mutate["no_scale"]
        sd = sd.copy()
        sd[l, k] = d4[l, k]
    Xn = p.lms.astype(LD) + sd
    R.put("LANDMARKS", Xn.reshape(-1), (_f(s) * Ed4 + _ab(d4) * Es + u * _ab(sd) + u * _ab(Xn)).reshape(-1))
    R.aux["det_ratio"], R.aux["z_gap"], R.aux["delta"], R.aux["Edelta"] = ratio, G["z_gap"], d4, Ed4
    dl, lift = d4[lm], ((g(6, u) + dn) * d4m)[lm]  # jl4 . N_l d(delta3) = jl3 . d(delta3): the lift's own roundings are separate
    _ldiff(R, p, [(jp[k], Ejp[k], jl4[k], ej4[k], dl, S3.row(jl3[k]) + (_ab(jl4[k]) * lift).sum(1)) for k in range(2)], rr, Err, 2, 5, u,
           mutate.get("drop_ldiff"))
    return R


def applied(p, inc, mutate=None, u=U64, R0=None):
    return apply_joint(p, inc, mutate, u, R0) if isinstance(p, Joint) else apply_pose(p, inc, mutate, u, R0)


def normalize_joint(cams, lms_h, u=U64):
    """Ref of CAMERAS [12 n_cams], LANDMARKS [4 n_lms] after normalize_joint at the given state (module docstring)."""
    R = Ref()
    P, X = np.asarray(cams, dtype=F).reshape(-1, 12).astype(LD), np.asarray(lms_h, dtype=F).reshape(-1, 4).astype(LD)
    Pn = P / np.sqrt((P * P).sum(1))[:, None]
    Xn = X / X[:, 3:4]
    EX = u * _ab(Xn)
    EX[:, 3] = 0.0
    R.put("CAMERAS", Pn.reshape(-1), (g(8, u) * _ab(Pn)).reshape(-1))
    R.put("LANDMARKS", Xn.reshape(-1), EX.reshape(-1))
    return R


def unobserved_moved(p, R, cams_dev, inc_amb):
    """The cameras without observations moved by exactly sigma * inc with sigma = 1 / eps to gamma_3: (|dev - P - inc / eps|,
    its bound) per entry; inc_amb: the ambient increment per entry ([n_cams, 12]: inc in step 1, N_c inc in step 2)."""
    c0 = np.flatnonzero(p.n_c == 0)
    mv = np.asarray(inc_amb, dtype=LD).reshape(-1, 12)[c0] / LD(p.eps)
    ref = p.cams[c0].astype(LD) + mv
    dev = np.asarray(cams_dev, dtype=F).reshape(-1, 12)[c0]
    extra = R.aux["Epin"][c0] / p.eps if "Epin" in R.aux else 0.0
    return _f(np.abs(dev.astype(LD) - ref)), (g(3) * _ab(mv) + extra + U64 * _ab(mv) + U64 * _ab(ref)) * (1 + 1e-6), c0


# ======== fp64 NumPy emulations in the kernels' operation order, with the two summation orders
def _osum(idx, n, a, order, off):
    """Per-landmark sums of the rows of a.  order "obs": in row order, one rounding per add (the per-observation kernels'
    scan over a landmark's lanes); "lpl": the lane-per-landmark form: every landmark's rows dealt to lanes of four
    consecutive rows, summed per lane, then a segmented tree over the lanes (seg_reduce_steps)."""
    if order == "obs":
        return OB._add_at(n, idx, a)
    out = np.zeros((n,) + a.shape[1:])
    for l in range(n):
        rows = a[off[l]:off[l + 1]]
        part = []
        for t in (rows[i:i + 4] for i in range(0, len(rows), 4)):
            acc = t[0].copy()
            for r in t[1:]:
                acc = acc + r
            part.append(acc)
        while len(part) > 1:
            part = [part[i] + part[i + 1] if i + 1 < len(part) else part[i] for i in range(0, len(part), 2)]
        out[l] = part[0]
    return out


def _tsum(a, order):
    """A global sum: "obs" front to back, "lpl" pairwise (per-workgroup partials, then reduce_partials)."""
    if order == "obs":
        return float(np.cumsum(a)[-1]) if len(a) else 0.0
    return float(np.sum(a))


class Info:
    pass


def _error_f(p, r2):
    if p.robust == "HUBER":
        w = np.where(r2 < p.huber * p.huber, 1.0, p.huber / np.sqrt(np.maximum(r2, 1e-300)))
        return 0.5 * (2 - w) * w * r2, w
    if p.robust == "CAUCHY":
        return np.log(1.0 + r2), np.ones(len(r2))
    return 0.5 * r2, np.ones(len(r2))


def _pose_residual_f(p, P, X):
    sa, sb = np.sqrt(p.alpha), np.sqrt(1.0 - p.alpha)
    U, V = p.obs[:, 0], p.obs[:, 1]
    h = np.concatenate([X, np.ones((len(X), 1))], 1)
    Pr = [P[:, 4 * k:4 * k + 4] for k in range(3)]
    m0, m1 = sb * (Pr[0] - Pr[2] * U[:, None]), sb * (Pr[1] - Pr[2] * V[:, None])
    return [RB._dot(m0, h), RB._dot(m1, h), RB._dot(sa * Pr[0], h) - sa * U, RB._dot(sa * Pr[1], h) - sa * V]


def _pose_jl_f(p, P, scale, s):
    sa, sb = np.sqrt(p.alpha), np.sqrt(1.0 - p.alpha)
    U, V = p.obs[:, 0], p.obs[:, 1]
    cb, ca = (sb * scale)[:, None], (sa * scale)[:, None]
    P0, P1, P2 = P[:, 0:3], P[:, 4:7], P[:, 8:11]
    return [cb * (P0 - P2 * U[:, None]) * s, cb * (P1 - P2 * V[:, None]) * s, ca * P0 * s, ca * P1 * s]


def _pose_jp_x_f(p, X, scale, zc):
    sa, sb = np.sqrt(p.alpha), np.sqrt(1.0 - p.alpha)
    U, V = p.obs[:, 0], p.obs[:, 1]
    h = np.concatenate([X, np.ones((len(X), 1))], 1)
    d = [RB._dot(h, zc[:, 4 * k:4 * k + 4]) for k in range(3)]
    return [sb * scale * (d[0] - U * d[2]), sb * scale * (d[1] - V * d[2]), sa * scale * d[0], sa * scale * d[1]]


def emulate_cost(p, order):
    """error_pose / error_homogeneous in fp64 (an Info with the ResidualInfo fields)."""
    ri = Info()
    n = len(p.cam_idx)
    if isinstance(p, Joint):
        P, X = p.cams[p.cam_idx], p.lms[p.lm]
        px, py, pz = (RB._dot(P[:, 4 * k:4 * k + 4], X) for k in range(3))
        r0, r1 = px / pz - p.obs[:, 0], py / pz - p.obs[:, 1]
        r2 = r0 * r0 + r1 * r1
        valid = np.abs(pz) >= Z_VALID
    else:
        res = _pose_residual_f(p, p.cams[p.cam_idx], p.lms[p.lm])
        r2 = res[0] * res[0] + res[1] * res[1] + res[2] * res[2] + res[3] * res[3]
        valid = np.ones(n, dtype=bool)
    e, _ = _error_f(p, r2)
    rs = np.sqrt(r2)
    ri.all_error, ri.all_residual_sum, ri.all_num_obs = _tsum(e, order), _tsum(rs, order), n
    ri.valid_error, ri.valid_residual_sum, ri.valid_num_obs = _tsum(e[valid], order), _tsum(rs[valid], order), int(valid.sum())
    return ri


def _inv3_delta_f(tot, lam):
    Hm = np.stack([tot[:, 0], tot[:, 1], tot[:, 2], tot[:, 1], tot[:, 3], tot[:, 4], tot[:, 2], tot[:, 4], tot[:, 5]], 1)
    Hm[:, [0, 4, 8]] += lam
    Hi = OB._inv3_f(Hm)
    return np.stack([-(Hi[:, 3 * a] * tot[:, 6] + Hi[:, 3 * a + 1] * tot[:, 7] + Hi[:, 3 * a + 2] * tot[:, 8]) for a in range(3)], 1)


_IDX6 = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def _red9(jl, rr):
    red = np.zeros((len(rr[0]), 9))
    for k in range(len(jl)):
        for t, (a, b) in enumerate(_IDX6):
            red[:, t] = red[:, t] + jl[k][:, a] * jl[k][:, b]
        for a in range(3):
            red[:, 6 + a] = red[:, 6 + a] + jl[k][:, a] * rr[k]
    return red


def emulate_apply_pose(p, inc, order):
    """(cameras, landmarks, l_diff) of apply_pose in fp64: OpBackVarproj / backsub_lpl or OpBackPoba with cam_apply_inc,
    sigma, the Jl scale and the weights from operand_bounds.emulate_pose."""
    c, lm = p.cam_idx, p.lm
    em = OB.emulate_pose(p, "obs" if order == "obs" else "lpl")
    sg = em["SIGMA"].reshape(-1, 12)
    s = em["JL_COL_SCALE"].reshape(-1, 3)
    inc = np.asarray(inc, dtype=F).reshape(-1, 12)
    P, X = p.cams[c], p.lms[lm]
    res = _pose_residual_f(p, P, X)
    r2 = res[0] * res[0] + res[1] * res[1] + res[2] * res[2] + res[3] * res[3]
    w = _error_f(p, r2)[1] if p.robust == "HUBER" else np.ones(len(c))
    sw = np.sqrt(w)
    rr = [sw * t for t in res]
    jls = _pose_jl_f(p, P, sw, s[lm])
    sv = inc * sg
    cams = p.cams + sv
    if p.solver == "POWER_VARPROJ":
        inc2 = sv * (1.0 / sg)
        Pn = cams[c]
        red = _red9(_pose_jl_f(p, Pn, np.ones(len(c)), np.ones((len(c), 3))), _pose_residual_f(p, Pn, X))
        dl = _inv3_delta_f(_osum(lm, p.n_lms, red, order, p.lm_off), 0.0)
        lms = p.lms + dl
        jp = _pose_jp_x_f(p, X, 1.0, inc2[c])
    else:
        jp = _pose_jp_x_f(p, X, sw, sv[c])
        red = _red9(jls, [r + t for r, t in zip(rr, jp)])
        dl = _inv3_delta_f(_osum(lm, p.n_lms, red, order, p.lm_off), p.lam_lm)
        lms = p.lms + dl * s
    d = dl[lm]
    sc = np.zeros(len(c))
    for k in range(4):
        ji = jp[k] + (jls[k][:, 0] * d[:, 0] + jls[k][:, 1] * d[:, 1] + jls[k][:, 2] * d[:, 2])
        sc = sc - ji * (0.5 * ji + rr[k])
    return cams, lms, _tsum(sc, order)


def emulate_apply_joint(p, inc, order):
    """(cameras, landmarks, l_diff) of apply_joint in fp64: OpBackJoint / backsub_lpl_h with cam_apply_inc_h."""
    c, lm = p.cam_idx, p.lm
    em = OB.emulate_joint(p)
    sg = em["SIGMA"].reshape(-1, 12)
    s = em["JL_COL_SCALE_H"].reshape(-1, 4)
    ncw = em["NC_HOUSEHOLDER"].reshape(-1, 13)
    cw, cb = ncw[:, :12], ncw[:, 12]
    x = np.asarray(inc, dtype=F).reshape(-1, 11)
    wt = np.zeros(p.n_cams)
    for j in range(11):
        wt = wt + cw[:, j + 1] * x[:, j]
    pin = np.concatenate([np.zeros((p.n_cams, 1)), x], 1) - (cb[:, None] * cw) * wt[:, None]
    z = pin * sg
    cams = p.cams + z
    P, X = p.cams[c], p.lms[lm]
    Pr = [P[:, 4 * k:4 * k + 4] for k in range(3)]
    px, py, pz = (RB._dot(Pr[k], X) for k in range(3))
    r0, r1 = px / pz - p.obs[:, 0], py / pz - p.obs[:, 1]
    D00, D02, D12 = 1 / pz, -px / (pz * pz), -py / (pz * pz)
    w = _error_f(p, r0 * r0 + r1 * r1)[1] if p.robust == "HUBER" else np.ones(len(c))
    sw = np.sqrt(w)
    sl = s[lm]
    jl4 = [sw[:, None] * (D00[:, None] * Pr[0] + D02[:, None] * Pr[2]) * sl, sw[:, None] * (D00[:, None] * Pr[1] + D12[:, None] * Pr[2]) * sl]
    lw, lb = house4(p.lms)
    wl, bl = lw[lm], lb[lm]
    jl3 = [j[:, 1:] - (bl * RB._dot(j, wl))[:, None] * wl[:, 1:] for j in jl4]
    rr = [sw * r0, sw * r1]
    zc = z[c]
    d = [RB._dot(X, zc[:, 4 * k:4 * k + 4]) for k in range(3)]
    jp = [sw * (D00 * d[0] + D02 * d[2]), sw * (D00 * d[1] + D12 * d[2])]
    red = np.zeros((len(c), 9))
    for k in range(2):
        for t, (a, b) in enumerate(_IDX6):
            red[:, t] = red[:, t] + jl3[k][:, a] * jl3[k][:, b]
    a0, a1 = rr[0] + jp[0], rr[1] + jp[1]
    for m in range(3):
        red[:, 6 + m] = jl3[0][:, m] * a0 + jl3[1][:, m] * a1
    d3 = _inv3_delta_f(_osum(lm, p.n_lms, red, order, p.lm_off), p.lam_lm)
    wd = lw[:, 1] * d3[:, 0] + lw[:, 2] * d3[:, 1] + lw[:, 3] * d3[:, 2]
    d4 = np.concatenate([np.zeros((p.n_lms, 1)), d3], 1) - (lb[:, None] * lw) * wd[:, None]
    lms = p.lms + d4 * s
    dd = d4[lm]
    sc = np.zeros(len(c))
    for k in range(2):
        ji = jp[k] + (jl4[k][:, 0] * dd[:, 0] + jl4[k][:, 1] * dd[:, 1] + jl4[k][:, 2] * dd[:, 2] + jl4[k][:, 3] * dd[:, 3])
        sc = sc - ji * (0.5 * ji + rr[k])
    return cams, lms, _tsum(sc, order)


def emulate_apply(p, inc, order):
    return emulate_apply_joint(p, inc, order) if isinstance(p, Joint) else emulate_apply_pose(p, inc, order)


def emulate_normalize(cams, lms_h):
    P, X = np.array(cams, dtype=F).reshape(-1, 12), np.array(lms_h, dtype=F).reshape(-1, 4)
    s = np.zeros(len(P))
    for k in range(12):
        s = s + P[:, k] * P[:, k]
    return P / np.sqrt(s)[:, None], X / X[:, 3:4]


# ======== shared by the CPU and the GPU tests
def seeded_increment(p, seed=5, scale=1e-3):
    """The increment handed to apply_*: a seeded vector, not a solve result, so the reference depends on inputs only.  The
    camera move is sigma * inc: 1e-3 of a well-observed camera's entries and less on the hubs."""
    return scale * np.random.default_rng(seed).normal(size=(12 if not isinstance(p, Joint) else 11) * p.n_cams)


def ambient_increment(p, inc):
    """[n_cams, 12] in long double: inc (step 1) or N_c inc (step 2, the reference's reflector)."""
    if isinstance(p, Joint):
        cw, cb = house12(p.cams.astype(LD))
        return _n12(cw, cb, np.asarray(inc, dtype=F).reshape(-1, 11).astype(LD))
    return np.asarray(inc, dtype=F).reshape(-1, 12).astype(LD)


def apply_check(p, R, cams, lms, l_diff):
    """[(quantity, err / bound, entries over, report line)] of a new state against R."""
    per = p.lms.shape[1]
    out = []
    for name, blk, dev, cnt in (("CAMERAS", 12, cams, p.n_c), ("LANDMARKS", per, lms, p.n_l), ("L_DIFF", 1, [l_diff], [len(p.cam_idx)])):
        r, over, line = report(name, blk, np.asarray(dev, dtype=F).reshape(-1), R.ref[name], R.bound[name], cnt)
        out.append((name, r, over, line))
    return out


def flagged(dev, ref, bound, per):
    return OB.flagged(dev, ref, bound, per)


def detectable(R, name, i):
    return OB.entry_scale(R, name, i)
