"""Componentwise, condition-free bounds for the covariance blocks of parameter pairs (povar_cov.hip: covariance_blocks;
povar_kernels_cov.hpp: pair_cc, pair_cl, pair_ll), entry by entry on the device's own C and Q (helper module of
tests/test_pair_bounds.py and tests/test_gpu_pair_bounds.py; not a test module).  The last stage of the covariance path of
tests/cov_bounds.py, with its conventions: LD, g(k) rounded up, first order, a final factor ONE, `worst` / `flagged` /
`report` from cov_bounds.  C is the symmetric matrix of cov_at's reads (cov_bounds.c_symmetric; cov_at :280-284), Q =
POVAR_BUF_COV_GAUGE (None: damped, nq = 0); the per-observation operands W_i = U_i^T G_i = E_i Hll^-1 (dim x 3; magnitudes Wm,
operand errors EW), Hll^-1 with EHi, sigma, the Jl column scales and the reflectors come from sc_bounds.pieces_pose /
pieces_joint and operand_bounds with their operand bounds, exactly as cov_bounds.landmark_reference / landmark_check take
them.  Line numbers are those of povar_kernels_cov.hpp.  chunk = 64 (step 1) or 32 (step 2); sizes(k) = the staged chunk sizes
of a track of k observations; ceil16(n) = ceil(n / 16).

pair_w (:603-608): row r of W_i on the device: Step::u's product sigma h (ScdPose::u; step 2 reads the staged U, whose arithmetic
EU carries) and the three-term dot with G (:607: three products, two additions): k_w = 4 roundings on Wm.
pair_t_add (:612-626): lane k of a group adds `tacc += qv * w` (:623) over the DIM rows of each of its ceil16(n) observations of
every chunk it is called for: one product and tt(k) = DIM sum_{n in sizes(k)} ceil16(n) additions.  pair_t_sum (:629-634): the
sixteen groups' partials in turn: 16.  So an entry of T_l = sum_i Q[c_i]^T W_i (nq x 3) carries k_t(k) = k_w + 1 + tt(k) + 16
roundings on Tm_l = sum_i |Q[c_i]|^T Wm_i and the operand error ET_l = sum_i |Q[c_i]|^T EW_i.

CAMERA-CAMERA  pair_cc (:640-683), solver coordinates: `s += qa[k] * qb[k]` (:654: g(nq)) and `cov_at - s` (:655: one rounding
          on both):   |out - (C[a, b] - Q_a Q_b^T)| <= u |C_ab| + g(nq + 1) |Q_a| |Q_b|^T.
          Damped (nq = 0) s is an exact zero and the subtraction changes nothing: the bound is ZERO, the block is C's entries
          bit for bit.  For a == b the entry (i, j), i > j, is evaluated as (j, i) (:650): symmetric bit for bit.
CAMERA-LANDMARK  pair_cl (:686-784), X = -sum_j C[c, c_j] W_j + Q_c T_l (DIM x 3).  The cameras of a track ascend, so the
          observations with c_j <= c (:717, `acc`) are a prefix of n_A and the others (:726, `accp`) the suffix of n_B.  A
          group takes every sixteenth j of a chunk (:715): at most t_A = sum over the chunks of ceil16(the chunk's share of the
          prefix) additions `acc += cv * w` (:724) per lane, or DIM t_B additions `accp += cv * w` (:732: DIM rows a j); the
          merge `acc += gl == p ? accp : 0` (:740): 1; block_sum<3 DIM, 256> (:741): 9; `v = -v` exact; then the nq additions
          of :752.  With the product cv w (1):   k_C = k_w + 1 + max(t_A, DIM t_B) + 10 + nq   on sum_j |C[c, c_j]| Wm_j,
          plus the operand term sum_j |C[c, c_j]| EW_j.  The T_l term: k_t(k), the product qc T (1) and the nq additions of
          :752:   |Q_c| ET_l + g(k_t(k) + 1 + nq) |Q_c| Tm_l.  (l, c) is the transposed store of (c, l) (`tr`, :761).
LANDMARK-LANDMARK  pair_ll (:787-902), Sigma_lm = delta_lm Hll^-1 + sum_{i in obs(l), j in obs(m)} W_i^T C[c_i, c_j] W_j - T_l^T T_m.
          Both chunk loops run in full (:807, :811): a group takes every sixteenth pair of a chunk pair (:818) and a lane
          every sixteenth entry of the DIM^2 (:823): trips(l, m) = ceil16(DIM^2) sum_{ni in sizes(k_l), nj in sizes(k_m)} ceil16(ni nj)
          additions `acc += wi * cv * wj` (:833) per lane at most, two products, block_sum<9, 256> (:838): 9, and
          `Hi + acc - tt` (:854): 2:   k_P = 2 k_w + 2 + trips(l, m) + 11,
              E(pairs) = sum_ij (EW_i^T |C_ij| Wm_j + Wm_i^T |C_ij| EW_j) + g(k_P) sum_ij Wm_i^T |C_ij| Wm_j.
          T_l is added at jc == 0 only and T_m at ic == 0 only (:816-817): each observation once.  `tt += T_l T_m` (:853: one
          product, nq additions) and the subtraction (1):
              E(T) = ET_l^T Tm_m + Tm_l^T ET_m + g(k_t(k_l) + k_t(k_m) + nq + 2) Tm_l^T Tm_m.
          Hll^-1 enters for l == m only (:854) and passes the two additions: E(Hi) + 2 u |Hi|.  For l == m the upper triangle
          stands for the lower one (:859).  (m, l), l < m, is the transposed store of (l, m) (:865).
Everywhere the magnitudes of the summands stay apart, so the cancellation of the free gauge is charged, and the long-double
reference's own rounding (its dots on the same magnitudes, in units of ULD) is added, as landmark_reference does.

PARAMETER COORDINATES (coords = 0): M_a X M_b^T with M = D (step 1) or D N_c (step 2, pair_nc :637) on a camera side and
          diag(s) or D4 N_l (house4) on a landmark side.  Per side, roundings and operand errors:
            camera, step 1     sigma: E(sigma) / sigma                                                    k = 0
            camera, step 2     pair_nc's entries (3, and the reflector's dNc) and the DIM-term dot (11)    k = 14, d = dNc
            landmark, step 1   s: E(s) / s                                                                k = 0
            landmark, step 2   N_l's entries against the long-double house4 (g(25), operand_bounds: dn),
                               the three-term dot (3)                                                     k = 3, d = g(25)
          and the scaling `s_a * v * s_b` (:681, :769, :781, :873, :895): 2.  With Lm = |M| and X^ the device's value:
              E0 = Lm_a E Lm_b^T + (g(2 + k_a + k_b) + d_a + d_b + rs_a + rs_b) Lm_a (|X| + E) Lm_b^T
          (camera_check's g(30) + 2 dNc for two camera sides, landmark_check's g(6) + 2 g(25) and g(2) for two landmark sides).

Exact facts (pair_check): every entry is finite; (b, a) is the bitwise transpose of (a, b); (a, a) is symmetric bit for bit;
a pair requested twice returns the same bits; an entry whose bound is zero is the reference's value exactly; every entry of
every block of the request is checked by exactly one of the three checks.

emulate_pairs: the three kernels in fp64 NumPy in their operation order -- lanes, groups, chunk loops, both pair_cl branches,
block_sum (a tree over the 256 threads), pair_t_sum's group order, the canonical order and `tr` --, vectorised over lanes, two
summation orders (0: ascending; 1: trips, rows, groups and dots descending, the other tree).  mutations_pairs: the defect list.
"""
import numpy as np

import cov_bounds as CB
import rounding_bounds as RB
import sc_bounds as SB
from cov_bounds import NB, _dot, _tree, flagged, report, worst  # noqa: F401  (worst / flagged / report: the cov_bounds ones)
from operand_bounds import F, LD, _ab, _f, g
from pair_covariance_reference import CAMERA, LANDMARK
from rounding_bounds import ULD
from sc_bounds import ONE

KW = 4  # pair_w: the roundings of a row of W_i on the device (module docstring)
CHECKS = ("pair_cc", "pair_cl", "pair_ll")


def chunk_of(dim):
    """SCD_CHUNK / SCDH_CHUNK (povar_kernels_sc.hpp): the staging chunk of pair_cl and pair_ll."""
    return 64 if dim == 12 else 32


def _sizes(k, chunk):
    return [min(chunk, k - a) for a in range(0, k, chunk)]


def _c16(n):
    return -(-n // 16)


def sides(dim, coords):
    """Rows of a camera side and of a landmark side of a block."""
    return {CAMERA: dim if coords == 1 else 12, LANDMARK: 3 if (coords == 1 or dim == 12) else 4}


def layout(pairs, dim, coords):
    """(shape of every block, off [n + 1]: where each starts in the flat request) -- cov_pair_request's `total` (cov_plan.hpp)."""
    sd = sides(dim, coords)
    shapes = [(sd[int(ka)], sd[int(kb)]) for ka, _, kb, _ in pairs]
    return shapes, np.r_[0, np.cumsum([r * c for r, c in shapes])].astype(np.int64)


def _kind(pair):
    ka, kb = int(pair[0]), int(pair[2])
    return "pair_cc" if ka == kb == CAMERA else "pair_ll" if ka == kb == LANDMARK else "pair_cl"


# ======== the long-double reference and its bound, solver coordinates
class _LmOps:
    """Per landmark, on demand: rows of C, W / Wm / EW stacked [k dim, 3], T_l / Tm_l / ET_l [nq, 3], k."""

    def __init__(self, sy, Q):
        self.sy, self.memo = sy, {}
        self.nq = 0 if Q is None else np.asarray(Q).shape[1]
        if self.nq:
            self.Ql, self.Qa = np.asarray(Q, dtype=F).astype(LD), np.abs(np.asarray(Q, dtype=F))

    def __call__(self, l):
        if l not in self.memo:
            sy, q, dim = self.sy, self.sy.q, self.sy.dim
            a, b, rows, _ = SB._lm_index(sy.p, int(l), dim)
            k = b - a
            o = dict(k=k, rows=rows, cams=sy.p.cam_idx[a:b], W=q.W[a:b].reshape(k * dim, 3), Wm=q.Wm[a:b].reshape(k * dim, 3),
                     EW=q.EW[a:b].reshape(k * dim, 3))
            if self.nq:
                o.update(T=self.Ql[rows].T @ o["W"], Tm=self.Qa[rows].T @ o["Wm"], ET=self.Qa[rows].T @ o["EW"])
            chunk = chunk_of(dim)
            o["kt"] = KW + 1 + dim * sum(_c16(n) for n in _sizes(k, chunk)) + 16
            self.memo[l] = o
        return self.memo[l]


def pair_reference(sy, Cs, Q, pairs):
    """[(block in long double, its bound) for every pair of the request, in request order], solver coordinates -- module
    docstring.  Cs: the symmetric C of cov_at's reads (cov_bounds.c_symmetric, [>= n, >= n]); Q: the device's gauge basis or None;
    pairs: (kind_a, id_a, kind_b, id_b) with the kinds of pair_covariance_reference."""
    dim, u, ch = sy.dim, sy.u, sy.R.aux["chain"]
    chunk = chunk_of(dim)
    Cf = np.asarray(Cs, dtype=F)[:sy.n, :sy.n]
    Cl, Ca = Cf.astype(LD), np.abs(Cf)
    ops = _LmOps(sy, Q)
    nq = ops.nq
    crow = lambda c: np.arange(dim * c, dim * c + dim)
    memo, out = {}, []

    def cc(a, b):
        ra, rb = crow(a), crow(b)
        val, e = Cl[np.ix_(ra, rb)], np.zeros((dim, dim))
        if nq:
            QQm = ops.Qa[ra] @ ops.Qa[rb].T
            val = val - ops.Ql[ra] @ ops.Ql[rb].T
            e = u * Ca[np.ix_(ra, rb)] + g(nq + 1, u) * QQm + (nq + 2) * ULD * (Ca[np.ix_(ra, rb)] + QQm)
        return val, e * ONE

    def cl(c, l):
        o, rc = ops(l), crow(c)
        ix = np.ix_(rc, o["rows"])
        n_a = int((o["cams"] <= c).sum())
        t_a = t_b = 0
        for a0, nj in zip(range(0, o["k"], chunk), _sizes(o["k"], chunk)):
            in_a = min(max(n_a - a0, 0), nj)
            t_a, t_b = t_a + _c16(in_a), t_b + _c16(nj - in_a)
        CWm = Ca[ix] @ o["Wm"]
        val = -(Cl[ix] @ o["W"])
        e = Ca[ix] @ o["EW"] + g(KW + 1 + max(t_a, dim * t_b) + 10 + nq, u) * CWm
        mag = CWm
        if nq:
            QT = ops.Qa[rc] @ o["Tm"]
            val = val + ops.Ql[rc] @ o["T"]
            e = e + ops.Qa[rc] @ o["ET"] + g(o["kt"] + 1 + nq, u) * QT
            mag = mag + QT
        return val, (e + (o["k"] * dim + nq + 8) * ULD * mag) * ONE

    def ll(l, m):
        ol, om = ops(l), ops(m)
        ix = np.ix_(ol["rows"], om["rows"])
        trips = _c16(dim * dim) * sum(_c16(ni * nj) for ni in _sizes(ol["k"], chunk) for nj in _sizes(om["k"], chunk))
        CWm = Ca[ix] @ om["Wm"]
        mag = ol["Wm"].T @ CWm
        val = ol["W"].T @ Cl[ix] @ om["W"]
        e = ol["EW"].T @ CWm + ol["Wm"].T @ (Ca[ix] @ om["EW"]) + g(2 * KW + 2 + trips + 11, u) * mag
        if l == m:
            Hi = ch["Hi"][l]
            val = val + Hi
            e = e + ch["EHi"][l] + 2 * u * _ab(Hi)
            mag = mag + _ab(Hi)
        if nq:
            TT = ol["Tm"].T @ om["Tm"]
            val = val - ol["T"].T @ om["T"]
            e = e + ol["ET"].T @ om["Tm"] + ol["Tm"].T @ om["ET"] + g(ol["kt"] + om["kt"] + nq + 2, u) * TT
            mag = mag + TT
        return val, (e + ((ol["k"] + om["k"]) * dim + nq + 8) * ULD * mag) * ONE

    for pair in pairs:
        ka, a, kb, b = (int(x) for x in pair)
        key = (ka, a, kb, b)
        if key not in memo:
            if ka == CAMERA and kb == CAMERA:
                memo[key] = cc(a, b)
            elif ka == LANDMARK and kb == LANDMARK:
                memo[key] = ll(a, b)
            elif ka == CAMERA:
                memo[key] = cl(a, b)
            else:
                v, e = cl(b, a)
                memo[key] = (v.T, e.T)
        out.append(memo[key])
    return out


# ======== the maps to parameter coordinates
def _side_maps(sy):
    """{kind: (L [n, rows, cols] long double, |L|, rs [n, rows], k, d)} -- module docstring: PARAMETER COORDINATES."""
    if hasattr(sy, "_pair_side_maps"):
        return sy._pair_side_maps
    u = sy.u
    L, Lm, rs, gmap = CB._camera_maps(sy)
    cam = (L, Lm, rs, 0, 0.0) if sy.dim == 12 else (L, Lm, rs, 14, float(sy.R.aux["dnc"]))
    if sy.dim == 12:
        s, Es = sy.R.ref["JL_COL_SCALE"].reshape(-1, 3), sy.R.bound["JL_COL_SCALE"].reshape(-1, 3)
        eye = np.eye(3, dtype=LD)[None]
        lm = (s[:, :, None] * eye, _f(s)[:, :, None] * np.eye(3)[None], Es / _f(s), 0, 0.0)
    else:
        s, Es = sy.R.ref["JL_COL_SCALE_H"].reshape(-1, 4), sy.R.bound["JL_COL_SCALE_H"].reshape(-1, 4)
        lw, lb = RB.house4(sy.p.lms.astype(LD))
        Nl = (np.eye(4, dtype=LD)[None] - lb[:, None, None] * lw[:, :, None] * lw[:, None, :])[:, :, 1:]
        Nm = (np.eye(4)[None] + _f(lb)[:, None, None] * _ab(lw)[:, :, None] * _ab(lw)[:, None, :])[:, :, 1:]
        lm = (s[:, :, None] * Nl, _f(s)[:, :, None] * Nm, Es / _f(s), 3, g(25, u))
    sy._pair_side_maps = {CAMERA: cam, LANDMARK: lm}
    return sy._pair_side_maps


def to_parameter_coords(sy, pair, val, e):
    """(M_a val M_b^T in long double, its bound) from a solver-coordinate block and its bound."""
    ka, a, kb, b = (int(x) for x in pair)
    ma, mb = _side_maps(sy)[ka], _side_maps(sy)[kb]
    (La, Lma, rsa), (k_a, d_a) = (x[a] for x in ma[:3]), ma[3:]
    (Lb, Lmb, rsb), (k_b, d_b) = (x[b] for x in mb[:3]), mb[3:]
    mag = Lma @ (_ab(val) + e) @ Lmb.T
    e0 = Lma @ e @ Lmb.T + (g(2 + k_a + k_b, sy.u) + d_a + d_b + rsa[:, None] + rsb[None, :] + 300 * ULD) * mag
    return La @ val @ Lb.T, e0 * ONE


def pair_check(sy, Cs, Q, pairs, blocks, coords=1, ref=None):
    """{'pair_cc': (err, bound), 'pair_cl': ..., 'pair_ll': ..., 'exact': messages}: every array has the length of the flat
    request (layout), zero outside the entries of its own kind, so a flagged index is an entry of the request.  blocks: what
    covariance_blocks returned for `pairs` in `coords`; ref: pair_reference's result for the same Cs, Q and pairs, when at hand."""
    pairs = [tuple(int(x) for x in pr) for pr in pairs]
    ref = pair_reference(sy, Cs, Q, pairs) if ref is None else ref
    shapes, off = layout(pairs, sy.dim, coords)
    total = int(off[-1])
    out = {k: (np.zeros(total), np.zeros(total)) for k in CHECKS}
    covered = np.zeros(total, dtype=np.int64)
    bad, first = [], {}
    assert len(blocks) == len(pairs) == len(ref)
    for t, (pair, blk) in enumerate(zip(pairs, blocks)):
        blk = np.asarray(blk, dtype=F)
        if blk.shape != shapes[t]:
            bad.append(f"pair {pair}: block of shape {blk.shape}, not {shapes[t]}")
            continue
        val, e = ref[t] if coords == 1 else to_parameter_coords(sy, pair, *ref[t])
        err = _ab(blk.astype(LD) - val)
        if not np.all(np.isfinite(blk)):
            bad.append(f"pair {pair}: non-finite entries")
            err = np.where(np.isfinite(blk), err, np.inf)
        if np.any((e == 0) & (blk.astype(LD) != val)):
            bad.append(f"pair {pair}: an entry whose bound is zero is not the reference's value")
        sl = slice(int(off[t]), int(off[t + 1]))
        k = _kind(pair)
        out[k][0][sl], out[k][1][sl] = err.reshape(-1), np.asarray(e, dtype=F).reshape(-1)
        covered[sl] += 1
        if pair in first:
            if not np.array_equal(blk, np.asarray(blocks[first[pair]])):
                bad.append(f"pair {pair} requested twice returns different bits")
            continue
        first[pair] = t
        back = (pair[2], pair[3], pair[0], pair[1])
        if back == pair:
            if not np.array_equal(blk, blk.T):
                bad.append(f"pair {pair}: not symmetric bit for bit")
        elif back in first and not np.array_equal(blk, np.asarray(blocks[first[back]]).T):
            bad.append(f"pair {pair} is not the bitwise transpose of {back}")
    if not np.all(covered == 1):
        bad.append(f"{int((covered != 1).sum())} entries of the request are not checked exactly once")
    out["exact"] = bad
    return out


# ======== fp64 emulation of the three kernels (order 0 / 1: module docstring)
class _Emu:
    """The operands the kernels read, in fp64, from the emulated staging q (sc_bounds._emu_pieces_*)."""

    def __init__(self, p, q, inv, panel, Q, dim, order):
        self.p, self.q, self.dim, self.order, self.Q = p, q, dim, order, (None if Q is None else np.asarray(Q, dtype=F))
        self.nq = 0 if Q is None else self.Q.shape[1]
        self.C = CB.c_symmetric(inv, panel)
        self.chunk = chunk_of(dim)
        self.seq = (lambda n: range(n)) if order == 0 else (lambda n: range(n - 1, -1, -1))
        self.W = self.w_rows(q.U, q.G)
        self.Hi = q.em["HLL_INV"].reshape(-1, 3, 3)
        self.sig = np.asarray(q.sig, dtype=F).reshape(-1, 12)
        if dim == 12:
            self.s = q.em["JL_COL_SCALE"].reshape(-1, 3)
        else:
            self.s = q.em["JL_COL_SCALE_H"].reshape(-1, 4)
            lw, lb = RB.house4(p.lms)
            self.Nl = np.eye(4)[None][:, :, 1:] - (lb[:, None, None] * lw[:, :, None]) * lw[:, None, 1:]  # delta(i, b + 1) - beta w_i w_{b+1}
            w, beta = q.ncw[:, :12], q.ncw[:, 12]
            self.Nc = np.eye(12)[None][:, :, 1:] - (beta[:, None, None] * w[:, :, None]) * w[:, None, 1:]  # pair_nc

    def w_rows(self, U, G):
        """pair_w for every observation: W[o, r, x] = u_0[r] G[0][x] + u_1[r] G[1][x] + u_2[r] G[2][x]."""
        t = [U[:, z, :, None] * G[:, z, None, :] for z in self.seq(3)]
        return (t[0] + t[1]) + t[2]

    def track(self, l):
        a, b = int(self.p.lm_off[l]), int(self.p.lm_off[l + 1])
        return a, b - a

    def cblock(self, ca, cb):
        """C[ca rows, cb rows] for arrays of cameras: [..., dim, dim]."""
        d = np.arange(self.dim)
        r = self.dim * np.asarray(ca)[..., None, None] + d[:, None]
        c = self.dim * np.asarray(cb)[..., None, None] + d[None, :]
        return self.C[r, c]

    def t_add(self, tacc, obs, W):
        """pair_t_add on the staged observations `obs` (global slots): tacc [16 groups, nq, 3]."""
        dim, n = self.dim, len(obs)
        cams = self.p.cam_idx[obs]
        for t in self.seq(_c16(n)):
            idx = np.arange(16 * t, min(16 * t + 16, n))
            grp = idx - 16 * t
            for r in self.seq(dim):
                tacc[grp] = tacc[grp] + self.Q[dim * cams[idx] + r][:, :, None] * W[obs[idx], r][:, None, :]

    def t_sum(self, tacc, skip=None):
        """pair_t_sum: the sixteen groups in turn: [nq, 3]."""
        s = np.zeros(tacc.shape[1:])
        for gq in self.seq(16):
            if gq != skip:
                s = s + tacc[gq]
        return s

    def block_sum(self, acc):
        """acc [16 groups, 16 lanes, ...] -> the workgroup's sum (a tree over the 256 threads)."""
        return _tree(np.moveaxis(acc.reshape((256,) + acc.shape[2:]), 0, -1), self.order)


def _emu_cc(E, a, b, coords, mut):
    """pair_cc for the canonical pair a >= b: the block as the kernel holds it before the store (tr is the caller's)."""
    dim, same = E.dim, a == b
    T = E.cblock(a, b).copy()
    if E.nq:
        qa = E.Q[dim * (b if mut.get("cc_q_rows") and not same else a):][:dim]
        T = T - _dot(qa, E.Q[dim * b:dim * b + dim].T, E.order)
    if same:
        T = np.triu(T) + np.triu(T, 1).T  # (:650)
    if coords == 1:
        return T
    sa, sb = E.sig[a], E.sig[a if mut.get("cc_sigma") else b]
    if dim == 12:
        V = T
    else:
        Na, Nb = E.Nc[a], E.Nc[a if mut.get("cc_n") else b]
        V = _dot(Na, _dot(T, Nb.T, E.order), E.order)
    V = (sa[:, None] * V) * sb[None, :]
    if same and not mut.get("cc_no_swap"):
        V = np.triu(V) + np.triu(V, 1).T  # (:668)
    return V


def _emu_cl(E, cam, l, coords, mut):
    """pair_cl for (camera, landmark): [sides] before the store."""
    dim, nq, chunk = E.dim, E.nq, E.chunk
    a0, k = E.track(l)
    acc, accp = np.zeros((16, dim, dim, 3)), np.zeros((16, dim, 3))  # [group, lane, p, x], [group, lane, x]
    tacc = np.zeros((16, max(nq, 1), 3))
    for jc in range(0, k, chunk):
        nj = min(chunk, k - jc)
        obs = a0 + jc + np.arange(nj)
        if nq:
            E.t_add(tacc, obs, E.W)
        for j in E.seq(nj):
            grp, o = j % 16, obs[j]
            bc = int(E.p.cam_idx[o])
            Cb = E.cblock(cam, bc)  # [p, r]
            w = E.W[o]  # [r, x]
            if cam >= bc:
                acc[grp] = acc[grp] + Cb.T[:, :, None] * w[:, None, :]  # lane r: acc[p, x] += C[c p, c_j r] w[r][x]
            else:
                Cr = Cb.T if mut.get("cl_branch_transposed") else Cb
                for r in E.seq(dim):
                    accp[grp] = accp[grp] + Cr[:, r, None] * w[None, r, :]  # lane p: accp[x] += C[c p, c_j r] w[r][x]
    if not mut.get("cl_no_merge"):
        d = np.arange(dim)
        acc[:, d, d, :] = acc[:, d, d, :] + accp
    full = np.zeros((16, 16, dim, 3))
    full[:, :dim] = acc
    X = -E.block_sum(full)
    if nq:
        Ts = E.t_sum(tacc, 1 if mut.get("t_group_skipped") else None)
        qc = E.Q[dim * cam:dim * cam + dim]
        for kq in E.seq(nq):
            X = (X - qc[:, kq, None] * Ts[None, kq, :]) if mut.get("cl_t_sign") else (X + qc[:, kq, None] * Ts[None, kq, :])
    if coords == 1:
        return X
    sg = E.sig[cam]
    if dim == 12:
        return (sg[:, None] * X) * E.s[l][None, :]
    nl = E.Nl[l]  # [y, b]
    inner = (X[:, None, 0] * nl[None, :, 0] + X[:, None, 1] * nl[None, :, 1]) + X[:, None, 2] * nl[None, :, 2]  # [p, y]
    V = _dot(E.Nc[cam], inner, E.order)
    return (sg[:, None] * V) * E.s[l][None, :]


def _emu_ll(E, l, m, coords, mut):
    """pair_ll for the canonical pair l <= m: the block before the store."""
    dim, nq, chunk, p = E.dim, E.nq, E.chunk, E.p
    same = l == m
    (al, kl), (am, km) = E.track(l), E.track(m)
    dd = dim * dim
    tK = _c16(dd)
    e = np.arange(tK * 16)
    e1, e2 = np.minimum(e, dd - 1) // dim, np.minimum(e, dd - 1) % dim
    live_e = e < dd
    Wj = E.W
    if mut.get("ll_m_head") and not same:  # the m side staged with landmark l's Hll^-1: G_j = F_j Hi_l
        sl_ = slice(am, am + km)
        Hi = E.Hi[l]
        Fm = E.q.F[sl_]
        G = Fm[:, :, 0, None] * Hi[None, None, 0, :] + Fm[:, :, 1, None] * Hi[None, None, 1, :] + Fm[:, :, 2, None] * Hi[None, None, 2, :]
        Wj = E.W.copy()
        Wj[sl_] = E.w_rows(E.q.U[sl_], G)
    acc = np.zeros((16, 16, 3, 3))
    tl, tm = np.zeros((16, max(nq, 1), 3)), np.zeros((16, max(nq, 1), 3))
    oj = np.zeros(chunk, dtype=np.int64)
    for ic in range(0, kl, chunk):
        ni = min(chunk, kl - ic)
        oi = al + ic + np.arange(ni)
        for jc in range(0, km, chunk):
            nj = min(chunk, km - jc)
            if not (mut.get("ll_oj_stale") and ic > 0):
                oj[:nj] = am + jc + np.arange(nj)
            ojv = oj[:nj].copy()
            if nq and (jc == 0 or mut.get("ll_tl_every_jc")):
                E.t_add(tl, oi, E.W)
            if nq and (ic == 0 or mut.get("ll_tm_every_ic")):
                E.t_add(tm, ojv, Wj)
            npp = ni * nj - (1 if mut.get("ll_skip_last_pp") else 0)
            ci, cj = p.cam_idx[oi], p.cam_idx[ojv]
            for t in E.seq(_c16(npp)):
                pp = np.arange(16 * t, min(16 * t + 16, npp))
                grp = pp - 16 * t
                i, j = pp // nj, pp % nj
                Cb = E.cblock(ci[i], cj[j])  # [g, r, c]
                by_rows = (ci[i] >= cj[j])[:, None]
                r, c = np.where(by_rows, e1[None, :], e2[None, :]), np.where(by_rows, e2[None, :], e1[None, :])
                gi = np.arange(len(pp))[:, None]
                cv = np.where(live_e[None, :], Cb[gi, r, c], 0.0)
                wi, wj = E.W[oi[i][:, None], r], Wj[ojv[j][:, None], c]  # [g, e, 3]
                terms = ((wi[:, :, :, None] * cv[:, :, None, None]) * wj[:, :, None, :]).reshape(len(pp), tK, 16, 3, 3)
                for s in E.seq(tK):
                    acc[grp] = acc[grp] + terms[:, s]
    A = E.block_sum(acc)
    tt = np.zeros((3, 3))
    if nq:
        skip = 1 if mut.get("t_group_skipped") else None
        Tl, Tm = E.t_sum(tl, skip), E.t_sum(tm, skip)
        for kq in E.seq(nq):
            tt = tt + Tl[kq, :, None] * Tm[kq, None, :]
    hi = E.Hi[l] if ((same and not mut.get("ll_no_hi")) or (not same and mut.get("ll_hi_offdiag"))) else 0.0
    Sg = hi + A - tt
    if same:
        Sg = np.triu(Sg) + np.triu(Sg, 1).T
    if coords == 1:
        return Sg
    if dim == 12:
        V = (E.s[l][:, None] * Sg) * E.s[m][None, :]
    else:
        Nl, Nm = E.Nl[l], E.Nl[m]
        inner = (Sg[:, None, 0] * Nm[None, :, 0] + Sg[:, None, 1] * Nm[None, :, 1]) + Sg[:, None, 2] * Nm[None, :, 2]  # [p, j]
        t = [Nl[:, z, None] * inner[None, z, :] for z in E.seq(3)]
        V = (E.s[l][:, None] * ((t[0] + t[1]) + t[2])) * E.s[m][None, :]
    if same:
        V = np.triu(V) + np.triu(V, 1).T
    return V


def emulate_pairs(p, q, inv, panel, Q, dim, order, pairs, coords, mutate=None):
    """The blocks of covariance_blocks for `pairs` in `coords`, in request order, from the buffers inv / panel (C through cov_at)
    and Q of an emulated or a real call and the fp64 staged operands q (sc_bounds._emu_pieces_*): the host's canonical order and
    `tr` (cov_plan.hpp: cov_pair_request), then pair_cc / pair_cl / pair_ll.  mutate: the defects of mutations_pairs."""
    mut = mutate or {}
    E = _Emu(p, q, inv, panel, Q, dim, order)
    memo, out = {}, []
    for pair in pairs:
        ka, a, kb, b = (int(x) for x in pair)
        if ka == CAMERA and kb == CAMERA:
            key, tr, fn = ("cc", max(a, b), min(a, b)), a < b, _emu_cc
        elif ka == LANDMARK and kb == LANDMARK:
            key, tr, fn = ("ll", min(a, b), max(a, b)), a > b, _emu_ll
        else:
            key, tr, fn = (("cl", a, b), False, _emu_cl) if ka == CAMERA else (("cl", b, a), True, _emu_cl)
        if key not in memo:
            memo[key] = fn(E, key[1], key[2], coords, mut)
        X = memo[key]
        if tr and mut.get({"cl": "cl_tr_ignored", "ll": "ll_tr_ignored"}.get(key[0])):
            out.append(np.ascontiguousarray(X).reshape(X.shape[1], X.shape[0]).copy())  # the canonical block's bytes, untransposed
        else:
            out.append(X.T.copy() if tr else X.copy())
    return out


# ======== the cases of tests/test_pair_bounds.py and tests/test_gpu_pair_bounds.py: (name, step, robust, lambda; 0: free gauge)
PAIR_CASES = ([("small", s, "NONE", lam) for s in (1, 2) for lam in (0.0, 1e-4)] + [("small", s, "HUBER", 0.0) for s in (1, 2)] +
              [("tracks", s, "NONE", 0.0) for s in (1, 2)] + [("long", s, "NONE", 0.0) for s in (1, 2)] +
              [("medium", s, "NONE", 1.0) for s in (1, 2)])
TRACK_CAMS, TRACK_CC = (0, 5, 65), (0, 4, 5, 6, 65)


def case_pairs(name, p, step=1):
    """The request of one case (module docstring of tests/test_gpu_pair_bounds.py)."""
    import pair_covariance_reference as P
    n_cams, n_lms = p.n_cams, p.n_lms
    if name == "small":  # every pair, shuffled, with duplicates (as test_small_free_gauge_every_pair builds them)
        cc, cl, ll = P.all_pairs(n_cams, n_lms)
        pairs = cc + cl + [(kb, b, ka, a) for ka, a, kb, b in cl] + ll
        rng = np.random.default_rng(100 * step)
        pairs = pairs + [pairs[i] for i in rng.integers(0, len(pairs), size=40)]
        return [pairs[i] for i in rng.permutation(len(pairs))]
    if name == "tracks":
        ll = [(LANDMARK, l, LANDMARK, m) for l in range(10) for m in range(10)]
        cl = [(CAMERA, c, LANDMARK, l) for c in TRACK_CAMS for l in range(10)]
        cc = [(CAMERA, a, CAMERA, b) for a in TRACK_CC for b in TRACK_CC]
        return ll + cl + [(kb, b, ka, a) for ka, a, kb, b in cl] + cc
    if name == "long":
        k = p.n_l
        big, mid = np.flatnonzero(k >= 65)[:2].tolist(), np.flatnonzero((k >= 33) & (k <= 64))[:3].tolist()
        ll = [(LANDMARK, l, LANDMARK, m) for l in big for m in big]
        ll += [pr for l in mid for m in big for pr in ((LANDMARK, l, LANDMARK, m), (LANDMARK, m, LANDMARK, l))]
        cc, cl, l2 = P.sample_pairs(np.random.default_rng(31 + step), n_cams, n_lms, 100)
        return ll + cc + cl + l2
    cc, cl, ll = P.sample_pairs(np.random.default_rng(7 + step), n_cams, n_lms, 200)
    return cc + cl + ll


# ======== mutations: (name, mutate, the checks that must report it, the flat entries of the request it touches)
def _entries(off, t):
    return set(range(int(off[t]), int(off[t + 1])))


def reads_of_c(sy, pairs, mask):
    """The flat entries (solver coordinates) of the request that read an entry of C where the symmetric boolean `mask` [n, n]
    is set: pair_cc's entry reads its own C entry; an entry (p, x) of a camera-landmark block reads row p of C[c, cams(l)]; every
    entry of a landmark-landmark block reads the whole C[cams(l), cams(m)]."""
    dim, p = sy.dim, sy.p
    shapes, off = layout(pairs, dim, 1)
    crow = lambda c: np.arange(dim * c, dim * c + dim)
    lrow = lambda l: SB._lm_index(p, int(l), dim)[2]
    out = set()
    for t, (ka, a, kb, b) in enumerate(pairs):
        if ka == CAMERA and kb == CAMERA:
            hit = mask[np.ix_(crow(a), crow(b))]
        elif ka == LANDMARK and kb == LANDMARK:
            hit = np.full((3, 3), bool(mask[np.ix_(lrow(a), lrow(b))].any()))
        elif ka == CAMERA:
            hit = np.repeat(mask[np.ix_(crow(a), lrow(b))].any(1)[:, None], 3, 1)
        else:
            hit = np.repeat(mask[np.ix_(crow(b), lrow(a))].any(1)[None, :], 3, 0)
        out |= {int(off[t]) + int(i) for i in np.flatnonzero(hit.reshape(-1))}
    return out


def c_tile_of(sy, pairs):
    """(I, J), I > J: the off-diagonal tile of C whose entries cov_bounds.emulate_lauum's `c_tile` perturbs (rows 64 I, 64 I + 1,
    columns 64 J + 32 .. 64 J + 47), read by a requested camera pair -- or None."""
    dim = sy.dim
    for ka, a, kb, b in pairs:
        if ka == CAMERA and kb == CAMERA and a != b:
            hi, lo = max(a, b), min(a, b)
            for I in {(dim * hi) // NB, (dim * hi + dim - 1) // NB}:
                for J in {(dim * lo) // NB, (dim * lo + dim - 1) // NB}:
                    rows = {NB * I, NB * I + 1} & set(range(dim * hi, dim * hi + dim))
                    cols = set(range(NB * J + 32, NB * J + 48)) & set(range(dim * lo, dim * lo + dim))
                    if I > J and rows and cols:
                        return I, J
    return None


def c_tile_mask(sy, tile):
    I, J = tile
    m = np.zeros((sy.N, sy.N), dtype=bool)
    m[NB * I:NB * I + 2, NB * J + 32:NB * J + 48] = True
    return (m | m.T)[:sy.n, :sy.n]


def mutations_pairs(sy, d, pairs):
    """Plausible defects of pair_cc, pair_cl, pair_ll and pair_t_sum, applied to the emulated blocks (emulate_pairs' mutate):
    (name, mutate, the checks that must report it, the flat entries of the request it touches).  mutate["coords"] is the
    coordinate system the defect shows in (1 unless it sits in the map to parameter coordinates); "exact" among the checks: the
    exact facts report it (an ignored `tr` shows in both: the block is wrong and no longer the bitwise transpose of its mirror
    pair, where the request holds both).  A defect is listed only where the request has what it needs.  `c_tile_1e-10` is not a defect of these
    kernels but of the C they read (mutate["c_tile"] for cov_bounds.emulate_lauum): no pair_* check may report it on its own C.
      pair_cl  cl_branch_transposed  :730 reads C[c r, c_j gl] for C[c gl, c_j r]      cl_no_merge  :740 dropped
               cl_t_sign  :752 `v -=`                                                  cl_tr_ignored  :761 / :769 / :781 store untransposed
      pair_ll  ll_m_head  :814 stages the m side with landmark l's head (here: its Hll^-1, G_j = F_j Hi_l)
               ll_oj_stale  :814 not run again for ic > 0                              ll_skip_last_pp  :818 `pp < ni * nj - 1`
               ll_tl_every_jc / ll_tm_every_ic  :816 / :817 without `jc == 0` / `ic == 0` (k_m / k_l above the chunk)
               ll_hi_offdiag / ll_no_hi  :854 Hll^-1 for l != m / not for l == m       ll_tr_ignored  :865 / :877 / :900
      pair_cc  cc_q_rows  :651 `qa` from camera b's rows                               cc_sigma_a_for_b  :681 sigma of a twice
               cc_n_a_for_b  :674 `wb` from camera a (step 2)                          cc_no_same_swap  :668 missing (parameter coordinates)
      pair_t_sum  t_group_skipped  :632 leaves group 1 out"""
    p, dim = sy.p, sy.dim
    chunk = chunk_of(dim)
    nq = 0 if d["Q"] is None else d["Q"].shape[1]
    k = p.n_l
    out = []

    def touched(pred, coords):
        _, off = layout(pairs, dim, coords)
        s = set()
        for t, pr in enumerate(pairs):
            if pred(*pr):
                s |= _entries(off, t)
        return s

    def add(name, mutate, checks, pred):
        coords = mutate.get("coords", 1)
        tch = touched(pred, coords)
        if tch:
            out.append((name, mutate, checks, tch))

    is_cl = lambda ka, kb: ka != kb
    cl_of = lambda ka, a, kb, b: (a, b) if ka == CAMERA else (b, a)
    last_cam = lambda l: int(p.cam_idx[p.lm_off[l + 1] - 1])
    has_b = lambda ka, a, kb, b: is_cl(ka, kb) and last_cam(cl_of(ka, a, kb, b)[1]) > cl_of(ka, a, kb, b)[0]
    is_ll = lambda ka, kb: ka == kb == LANDMARK
    is_cc = lambda ka, kb: ka == kb == CAMERA
    add("cl_branch_transposed", {"cl_branch_transposed": True}, ("pair_cl",), has_b)
    add("cl_no_merge", {"cl_no_merge": True}, ("pair_cl",), has_b)
    add("cl_tr_ignored", {"cl_tr_ignored": True}, ("pair_cl", "exact"), lambda ka, a, kb, b: ka == LANDMARK and kb == CAMERA)
    add("ll_m_head", {"ll_m_head": True}, ("pair_ll",), lambda ka, a, kb, b: is_ll(ka, kb) and a != b)
    add("ll_oj_stale", {"ll_oj_stale": True}, ("pair_ll",), lambda ka, a, kb, b: is_ll(ka, kb) and k[a] > chunk and k[b] > chunk)
    add("ll_skip_last_pp", {"ll_skip_last_pp": True}, ("pair_ll",), lambda ka, a, kb, b: is_ll(ka, kb))
    add("ll_hi_offdiag", {"ll_hi_offdiag": True}, ("pair_ll",), lambda ka, a, kb, b: is_ll(ka, kb) and a != b)
    add("ll_no_hi", {"ll_no_hi": True}, ("pair_ll",), lambda ka, a, kb, b: is_ll(ka, kb) and a == b)
    add("ll_tr_ignored", {"ll_tr_ignored": True}, ("pair_ll", "exact"), lambda ka, a, kb, b: is_ll(ka, kb) and a > b)
    add("cc_sigma_a_for_b", {"cc_sigma": True, "coords": 0}, ("pair_cc",), lambda ka, a, kb, b: is_cc(ka, kb) and a != b)
    add("cc_no_same_swap", {"cc_no_swap": True, "coords": 0}, ("exact",), lambda ka, a, kb, b: is_cc(ka, kb) and a == b)
    if dim == 11:
        add("cc_n_a_for_b", {"cc_n": True, "coords": 0}, ("pair_cc",), lambda ka, a, kb, b: is_cc(ka, kb) and a != b)
    if nq:
        add("cl_t_sign", {"cl_t_sign": True}, ("pair_cl",), lambda ka, a, kb, b: is_cl(ka, kb))
        # (the canonical pair is (min, max): T of the smaller id is added at jc == 0, of the larger at ic == 0)
        add("ll_tl_every_jc", {"ll_tl_every_jc": True}, ("pair_ll",), lambda ka, a, kb, b: is_ll(ka, kb) and k[max(a, b)] > chunk)
        add("ll_tm_every_ic", {"ll_tm_every_ic": True}, ("pair_ll",), lambda ka, a, kb, b: is_ll(ka, kb) and k[min(a, b)] > chunk)
        add("cc_q_rows", {"cc_q_rows": True}, ("pair_cc",), lambda ka, a, kb, b: is_cc(ka, kb) and a != b)
        add("t_group_skipped", {"t_group_skipped": True}, ("pair_cl", "pair_ll"), lambda ka, a, kb, b: not is_cc(ka, kb))
    tile = c_tile_of(sy, pairs)
    if tile is not None:
        out.append(("c_tile_1e-10", {"c_tile": tile}, ("lauum",), reads_of_c(sy, pairs, c_tile_mask(sy, tile))))
    return out


def split_mutation(mutate):
    """(the coordinate system a mutation shows in, emulate_pairs' mutate without the bookkeeping keys)."""
    m = dict(mutate)
    return m.pop("coords", 1), m
