"""Componentwise, condition-free bounds for the rows of povar_observation_hat_pose / _joint (obs_hat, povar_kernels_cov.hpp) on
the device's own C and Sigma_l, in the manner of the OBSERVATION stage of tests/cov_bounds.py, whose conventions, operands and
Syy_i these are (helper module of tests/test_hat_reference.py and tests/test_gpu_observation_hat.py; not a test module).

Everything up to Syy_i is obs_cov's walk: syy_reference restates cov_bounds.observation_reference up to
    Syy_i = K_ii - R_i L_i^T - L_i R_i^T + L_i Sigma_l L_i^T    with its bound E(Syy) and Sa = |Syy| + E(Syy)
(the same expressions, the same operation counts: one body on the device, one derivation here).  The new row, lane 0 of the
group (ObsHatRow::write, Step::jac_a), from the caller's cameras, points and image points and the reference chain of
operand_bounds (sw to rho, w to 2 rho; y = P h a four-term dot: E(y) = g(4) |P| |h| =: g(4) ym):

Step 1 (ScdPose::jac_a).  sb = sqrt(1 - alpha), sa = sqrt(alpha) in fp64 (operand_bounds: dsb = g(2) each).
    wb = sw sb, wa = sw sa                      one product: relative rw = rho + g(3)
    A  = [[wb, 0, -(wb u)], [0, wb, -(wb v)], [wa, 0, 0], [0, wa, 0]]:   E(A) = |A| rw, one more u on the two products with u, v
    r0 = wb (y0 - u y2), r1 alike               the dot (4), the product u y2 and the difference (2), wb (3 and rho), the product (1):
                                                E(r) = (g(10) + rho) |wb| (ym0 + |u| ym2)
    r2 = wa (y0 - u), r3 alike                  the dot (4), the difference (1), wa (3 and rho), the product (1):
                                                E(r) = (g(9) + rho) |wa| (ym0 + |u|)
Step 2 (ScdJoint::jac_a).
    iz = 1 / y2                                 relative rz = E(y2) / |y2| + u                              (as cov_bounds' J)
    px = y0 iz                                  E(px) = E(y0) |iz| + |px| (rz + u)
    wz = sw iz                                  relative rho + rz + u
    A  = [[wz, 0, -(wz px)], [0, wz, -(wz py)]]:  E(A_k2) = |wz| E(px) + |wz px| (rho + rz + 2 u)
    r0 = sw (px - u)                            E(r) = |sw| E(px) + (rho + g(2)) |sw| (|px| + |u|)
A small |y2| inflates every step-2 bound through rz, as everywhere in the project; no condition number appears.

The block (ObsHatRow::write): T = A Syy and P = T A^T, three-term dots (3 roundings each), upper triangle:
    E(T) = |A| E(Syy) + E(A) Sa + g(3) |A| Sa
    E(P) = E(T) |A|^T + (|A| Sa) E(A)^T + g(3) |A| Sa |A|^T
plus the long-double reference's own rounding (20 ULD on the last magnitude).  Given C this is condition-free.
Exact: a landmark requested twice returns the same bits.
"""
import numpy as np

import cov_bounds as CB
import sc_bounds as SB
from operand_bounds import F, LD, _ab, _f, g
from rounding_bounds import ULD
from sc_bounds import ONE


def syy_reference(sy, Cs, ids=None):
    """Per requested landmark (Syy [k, 3, 3] long double, E(Syy), Sa) -- cov_bounds.observation_reference up to its Syy, on the
    symmetric C of cov_at's reads."""
    p, q, dim, u = sy.p, sy.q, sy.dim, sy.u
    ids = np.arange(p.n_lms) if ids is None else np.asarray(ids)
    o = CB.observation_operands(sy)
    Sig, ESig = CB.landmark_reference(sy, Cs, None, ids)
    tK = -(-dim * dim // 16)
    kK = tK + 2 + (2 if dim == 12 else 0)
    Cl, Ca = np.asarray(Cs, dtype=F).astype(LD), np.abs(np.asarray(Cs, dtype=F))
    T = lambda A: A.transpose(0, 2, 1)
    mm = lambda A, B: np.einsum("ixz,izy->ixy", A, B)
    out = []
    for t, l in enumerate(ids):
        a, b, rows, _ = SB._lm_index(p, int(l), dim)
        k = b - a
        ix = np.ix_(rows, rows)
        X, Xa = Cl[ix].reshape(k, dim, k * dim), Ca[ix].reshape(k, dim, k * dim)
        U, Um, EU = q.U[a:b], q.Um[a:b], q.EU[a:b]
        G, Gm, EG = q.G[a:b], q.Gm[a:b], q.EG[a:b]
        right = lambda Y, V: np.einsum("iajc,jbc->ijab", Y.reshape(k, 3, k, dim), V)
        K = right(U @ X, U)
        UmX = Um @ Xa
        Km = right(UmX, Um)
        EK = right(EU @ Xa, Um) + right(UmX, EU)
        R = np.einsum("ijab,jbm->iam", K, G)
        Rm = np.einsum("ijab,jbm->iam", Km, Gm)
        ER = np.einsum("ijab,jbm->iam", EK, Gm) + np.einsum("ijab,jbm->iam", Km, EG) + g(kK + 7 + k, u) * Rm
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
        RmL = mm(Rm, T(La))
        ESyy = ESyy + (k * (dim + 3) + 20) * ULD * (Kiim + RmL + T(RmL) + LSLa)
        out.append((Syy, ESyy, _ab(Syy) + ESyy))
    return out


class HatOperands:
    """Per observation, long double with magnitudes and operand errors: A [n, d, 3], r [n, d]."""


def hat_operands(sy):
    """What lane 0 of obs_hat forms (module docstring).  Computed once per system."""
    if hasattr(sy, "_hat_operands"):
        return sy._hat_operands
    p, u, ch = sy.p, sy.u, sy.R.aux["chain"]
    o = CB.observation_operands(sy)
    c = p.cam_idx
    n = len(c)
    Pa = np.abs(p.cams[c].reshape(n, 3, 4))
    ym = np.einsum("nxk,nk->nx", Pa, _ab(sy.q.h))
    uv, uva = p.obs.astype(LD), np.abs(p.obs)
    rho = ch["rho"]
    h = HatOperands()
    if sy.dim == 12:
        sw = np.sqrt(ch["w"])
        sb, sa = np.sqrt(LD(1) - LD(p.alpha)), np.sqrt(LD(p.alpha))
        wb, wa = sw * sb, sw * sa
        rw = rho + g(3, u)
        A = np.zeros((n, 4, 3), dtype=LD)
        A[:, 0, 0] = A[:, 1, 1] = wb
        A[:, 0, 2], A[:, 1, 2] = -(wb * uv[:, 0]), -(wb * uv[:, 1])
        A[:, 2, 0] = A[:, 3, 1] = wa
        h.A, h.Aa = A, _ab(A)
        h.EA = h.Aa * rw[:, None, None]
        h.EA[:, :2, 2] += u * h.Aa[:, :2, 2]
        y = o.y
        h.r = np.stack([wb * (y[:, 0] - uv[:, 0] * y[:, 2]), wb * (y[:, 1] - uv[:, 1] * y[:, 2]),
                        wa * (y[:, 0] - uv[:, 0]), wa * (y[:, 1] - uv[:, 1])], 1)
        wba, waa = _f(wb), _f(wa)
        h.Er = np.stack([(g(10, u) + rho) * wba * (ym[:, 0] + uva[:, 0] * ym[:, 2]), (g(10, u) + rho) * wba * (ym[:, 1] + uva[:, 1] * ym[:, 2]),
                         (g(9, u) + rho) * waa * (ym[:, 0] + uva[:, 0]), (g(9, u) + rho) * waa * (ym[:, 1] + uva[:, 1])], 1)
    else:
        sw, swa = ch["sw"], _f(ch["sw"])
        y, Ey = o.y, o.Ey
        iz = 1 / y[:, 2]
        iza = _f(_ab(iz))
        rz = Ey[:, 2] * iza + u
        wz = sw * iz
        wza = _f(_ab(wz))
        A, EA = np.zeros((n, 2, 3), dtype=LD), np.zeros((n, 2, 3))
        r, Er = np.zeros((n, 2), dtype=LD), np.zeros((n, 2))
        for k in range(2):
            px = y[:, k] * iz
            pxa = _f(_ab(px))
            Epx = Ey[:, k] * iza + pxa * (rz + u)
            A[:, k, k], A[:, k, 2] = wz, -(wz * px)
            EA[:, k, k] = wza * (rho + rz + u)
            EA[:, k, 2] = wza * Epx + wza * pxa * (rho + rz + 2 * u)
            r[:, k] = sw * (px - uv[:, k])
            Er[:, k] = swa * Epx + (rho + g(2, u)) * swa * (pxa + uva[:, k])
        h.A, h.Aa, h.EA, h.r, h.Er = A, _ab(A), EA, r, Er
    sy._hat_operands = h
    return h


def hat_reference(sy, Cs, ids=None):
    """(r [rows, d], E(r), P [rows, d, d], E(P)) long double references and bounds for the rows of one call, in its order."""
    p, u = sy.p, sy.u
    ids = np.arange(p.n_lms) if ids is None else np.asarray(ids)
    h = hat_operands(sy)
    T = lambda A: A.transpose(0, 2, 1)
    mm = lambda A, B: np.einsum("ixz,izy->ixy", A, B)
    r, Er, P, EP = [], [], [], []
    for (Syy, ESyy, Sa), l in zip(syy_reference(sy, Cs, ids), ids):
        a, b = int(p.lm_off[l]), int(p.lm_off[l + 1])
        A, Aa, EA = h.A[a:b], h.Aa[a:b], h.EA[a:b]
        AS = mm(Aa, Sa)
        ET = mm(Aa, ESyy) + mm(EA, Sa) + g(3, u) * AS
        Pm = mm(AS, T(Aa))
        P.append(mm(mm(A, Syy), T(A)))
        EP.append((mm(ET, T(Aa)) + mm(AS, T(EA)) + (g(3, u) + 20 * ULD) * Pm) * ONE)
        r.append(h.r[a:b])
        Er.append(h.Er[a:b] * ONE)
    return np.concatenate(r), np.concatenate(Er), np.concatenate(P), np.concatenate(EP)


def hat_check(sy, Cs, r, P, ids=None, ref=None):
    """{'hat_r': (err, bound) [rows, d], 'hat_p': (err, bound) [rows, d, d], 'exact': messages} for the rows of one call."""
    wr, er, wp, ep = hat_reference(sy, Cs, ids) if ref is None else ref
    r, P = np.asarray(r, dtype=F), np.asarray(P, dtype=F)
    assert r.shape == wr.shape and P.shape == wp.shape, (r.shape, wr.shape, P.shape, wp.shape)
    bad = []
    if not (np.all(np.isfinite(r)) and np.all(np.isfinite(P))):
        bad.append("non-finite entries in the hat rows")
    if not np.array_equal(P, P.transpose(0, 2, 1)):
        bad.append("a block is not symmetric")
    ids_ = np.arange(sy.p.n_lms) if ids is None else np.asarray(ids)
    start = np.r_[0, np.cumsum(sy.p.n_l[ids_])]
    first = {}
    for t, l in enumerate(ids_.tolist()):
        if l in first:
            s0, s1 = start[first[l]], start[first[l] + 1]
            if not (np.array_equal(r[start[t]:start[t + 1]], r[s0:s1]) and np.array_equal(P[start[t]:start[t + 1]], P[s0:s1])):
                bad.append(f"landmark {l} requested twice returns different bits")
        first.setdefault(l, t)
    err_r = np.where(np.isfinite(r), _f(_ab(r.astype(LD) - wr)), np.inf)
    err_p = np.where(np.isfinite(P), _f(_ab(P.astype(LD) - wp)), np.inf)
    return {"hat_r": (err_r, er), "hat_p": (err_p, ep), "exact": bad}


# ======== fp64 emulation of the row (the staged operands q and the buffers of cov_bounds.emulate_case)
def emulate_hat(p, q, inv, panel, sig, dim, ids=None):
    """obs_hat in fp64 from the staged operands q, the emulated C (inv, panel) and `sig` = Sigma_l without the gauge correction of
    the same ids: (r [rows, d], P [rows, d, d]).  The walk's own summation order is cov_bounds.emulate_observations' subject; here
    the sums are NumPy's and lane 0's expressions are the kernel's."""
    import rounding_bounds as RB
    ids = np.arange(p.n_lms) if ids is None else np.asarray(ids)
    Cs = CB.c_symmetric(np.asarray(inv), np.asarray(panel))
    Pc = p.cams.reshape(-1, 3, 4)
    if dim == 12:
        s_all = q.em["JL_COL_SCALE"].reshape(-1, 3)
        sa = np.sqrt(p.alpha)
    else:
        s_all = q.em["JL_COL_SCALE_H"].reshape(-1, 4)
        lw, lb = RB.house4(p.lms)
    rs, Ps = [], []
    for t, l in enumerate(ids.tolist()):
        a, b = int(p.lm_off[l]), int(p.lm_off[l + 1])
        k = b - a
        cams = p.cam_idx[a:b]
        idx = (dim * cams[:, None] + np.arange(dim)[None, :]).reshape(-1)
        X = Cs[np.ix_(idx, idx)].reshape(k, dim, k, dim)
        U, G = q.U[a:b], q.G[a:b]
        K = np.einsum("iar,irjc,jbc->ijab", U, X, U)
        R = np.einsum("ijab,jbm->iam", K, G)
        for i in range(k):
            o = a + i
            Pi, h, sw = Pc[cams[i]], q.h[o], q.sw[o]
            yv = ((Pi[:, 0] * h[0] + Pi[:, 1] * h[1]) + Pi[:, 2] * h[2]) + Pi[:, 3] * h[3]
            u_, v_ = p.obs[o]
            if dim == 12:
                L = Pi[:, :3] * s_all[l][None, :]
                wb, wa = sw * q.sb, sw * sa
                A = np.array([[wb, 0, -(wb * u_)], [0, wb, -(wb * v_)], [wa, 0, 0], [0, wa, 0]])
                r = np.array([wb * (yv[0] - u_ * yv[2]), wb * (yv[1] - v_ * yv[2]), wa * (yv[0] - u_), wa * (yv[1] - v_)])
            else:
                q4 = Pi * s_all[l][None, :]
                aw = ((q4[:, 0] * lw[l, 0] + q4[:, 1] * lw[l, 1]) + q4[:, 2] * lw[l, 2]) + q4[:, 3] * lw[l, 3]
                L = q4[:, 1:] - (lb[l] * aw)[:, None] * lw[l, None, 1:]
                iz = 1.0 / yv[2]
                px, py, wz = yv[0] * iz, yv[1] * iz, sw * iz
                A = np.array([[wz, 0, -(wz * px)], [0, wz, -(wz * py)]])
                r = np.array([sw * (px - u_), sw * (py - v_)])
            Syy = K[i, i] - R[i] @ L.T - L @ R[i].T + L @ (sig[t] @ L.T)
            Syy = np.triu(Syy) + np.triu(Syy, 1).T
            Pb = (A @ Syy) @ A.T
            rs.append(r)
            Ps.append(np.triu(Pb) + np.triu(Pb, 1).T)
    return np.array(rs), np.array(Ps)
