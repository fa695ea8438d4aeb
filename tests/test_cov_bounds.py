"""The bounds, emulations and mutations of tests/cov_bounds.py, without a GPU.

* Exact arithmetic on a tiny system (`small`, step 1, free gauge: n = 72, N = 128), built independently from the reference's
  formulas with tests/exact_rational.py: S, the per-observation E_i Hll^-1 and the gauge generators are exact rationals; the
  irrational stages (Gram-Schmidt, Cholesky, inverse, C, the blocks) run in 60-digit arithmetic, each from the once-rounded
  output of the one before.  All seven checks (assembly with Q Q^T, gauge, span, inverse, camera, lauum, landmark) and both
  coordinate maps admit the once-rounded results: worst err / bound assembly 0.0058, gauge 0.0089, span 1.1e-5, inverse
  0.90, camera 0.081, lauum 0.015, landmark 3.1e-4 (own coordinates: camera 0.018, landmark 5.2e-4).  Step 1 only: step 2's
  reflectors and 1 / z put irrational numbers into the operands themselves; its formulas are held by the emulations below.
* Both emulated summation orders of the whole chain (assembly, Q Q^T, factor, inverse, camera blocks, C, landmark blocks) lie
  inside every bound on every shape of tests/test_gpu_cov_bounds.py, in both coordinate systems: the bounds are satisfiable
  before a GPU sees them.  Worst err / bound over all of them: assembly 0.31, gauge 0.040, span 3.9e-4, inverse 0.98, camera
  0.54, lauum 0.16, landmark 0.013.
* Every mutation of cov_bounds.mutations is reported by its own check, on the entries it touches and on no other, and leaves
  every other check clean.
* The gap: on the same case the normwise bounds of tests/test_gpu_camera_covariance.py / test_gpu_landmark_covariance.py accept
  a tile of C perturbed by 1e-10 relative (0.11 of the landmark bound) while LAUUM rejects it at 1.4e4 times its bound.  No
  structural mutation passes the normwise bounds on that case (small, step 1, free gauge), and the perturbed tile of W misses
  the camera bound by a factor 2.4; the stage checks reject every one of them by 1e3 .. 1e14.
"""
from fractions import Fraction

import numpy as np
import pytest

import cov_bounds as CB
import sc_bounds as SB

F = np.float64
system, emulated, _report = CB.system, CB.emulated, CB.report


def _ld_fraction(x):
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - np.longdouble(hi)))


def test_exact_arithmetic_on_a_tiny_system_stays_inside_every_bound():
    """`small`, step 1, free gauge (6 cameras, 40 landmarks, n = 72, N = 128: two block columns, camera 5 across the 64-edge),
    built independently of sc_bounds and cov_bounds from the reference's formulas in exact rationals
    (exact_rational.ExactStep1: Jp, Jl, Hll^-1 per observation; the long-double sigma and Jl scale of the reference taken as
    exact numbers, as tests/test_sc_bounds.py does): S = sigma (Hpp - sum E_i Hll^-1 E_j^T) sigma, E_i Hll^-1 per observation,
    the generators of the gauge.  Roots are irrational, so from there on the chain runs in 60-digit arithmetic (mpmath), each
    stage from the once-rounded output of the stage before, as the device's stages do: Q by the call's Gram-Schmidt, R the
    Cholesky factor of S + Q Q^T, W = R^-1, C = W W^T, the camera blocks, Sigma_l = Hll^-1 + sum W_i^T C W_j - T_l^T T_l, both
    coordinate maps.  Every output, rounded once to fp64, goes through check_all: all seven checks, both coordinate systems.
    This is the least every bound must admit, and it holds the long-double formulas of cov_bounds (not only the emulations
    written beside them) to an independent reference."""
    import mpmath as mp
    import exact_rational as ER
    mp.mp.dps = 60
    sy = system("small", 1, "NONE", 0.0)
    p, n, N, dim = sy.p, sy.n, sy.N, 12
    ex = ER.ExactStep1(p.alpha, p.n_cams, p.lm_off, p.cam_idx, p.obs, p.cams, p.lms)
    sig = [[_ld_fraction(t) for t in row] for row in sy.R.aux["chain"]["sig"]]
    s = [[_ld_fraction(t) for t in row] for row in sy.R.ref["JL_COL_SCALE"].reshape(-1, 3)]
    S = [[Fraction(0)] * n for _ in range(n)]
    for c, H in enumerate(ex.hpp()):
        for i in range(12):
            for j in range(12):
                S[12 * c + i][12 * c + j] += sig[c][i] * H[i][j] * sig[c][j]
    lm_ops = []  # per landmark: (cameras, W_i = E_i Hll^-1 in the scaled landmark coordinates [k][12][3], Hll^-1 scaled)
    for l, (ob, Hi) in enumerate(ex.lm):
        E = [[[sig[c][j] * sum(ex.D2[r] * Jp0[r][j] * Jl0[r][a] for r in range(4)) for a in range(3)] for j in range(12)]
             for c, Jp0, Jl0, _ in ob]
        EH = [[[sum(Ei[j][a] * Hi[a][b] for a in range(3)) for b in range(3)] for j in range(12)] for Ei in E]
        cams = [c for c, _, _, _ in ob]
        for i, ci in enumerate(cams):
            for j, cj in enumerate(cams):
                for r in range(12):
                    for q in range(12):
                        S[12 * ci + r][12 * cj + q] -= sum(EH[i][r][b] * E[j][q][b] for b in range(3))
        lm_ops.append((cams, [[[EHi[r][b] / s[l][b] for b in range(3)] for r in range(12)] for EHi in EH],
                       [[Hi[a][b] / (s[l][a] * s[l][b]) for b in range(3)] for a in range(3)]))
    mpf = lambda f: mp.mpf(f.numerator) / f.denominator
    fl = lambda M: np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])
    mpm = lambda A: mp.matrix([[mp.mpf(float(x)) for x in row] for row in A])
    # Q: gauge_basis's generators and twice-applied Gram-Schmidt (the supports stay disjoint exactly)
    V = [[mp.mpf(0)] * n for _ in range(12)]
    for col in range(12):
        gi, gj = divmod(col, 4)
        for c in range(p.n_cams):
            for r in range(3):
                V[col][12 * c + 4 * r + gj] = -mp.mpf(float(p.cams[c, 4 * r + gi])) / mpf(sig[c][4 * r + gj])
    dot = lambda x, y: mp.fsum(a * b for a, b in zip(x, y))
    for k in range(12):
        for _ in range(2):
            for j in range(k):
                t = dot(V[j], V[k])
                V[k] = [a - t * b for a, b in zip(V[k], V[j])]
        nrm = mp.sqrt(dot(V[k], V[k]))
        V[k] = [a / nrm for a in V[k]]
    Q = np.array([[float(V[k][i]) for k in range(12)] for i in range(n)])
    Qm = mpm(Q)
    A = mp.matrix([[mpf(x) for x in row] for row in S]) + Qm * Qm.T
    R = np.eye(N)
    R[:n, :n] = fl(mp.cholesky(A).T)
    W = np.eye(N)
    W[:n, :n] = np.triu(fl(mp.inverse(mpm(R[:n, :n]))))
    Wm = mpm(W[:n, :n])
    Cm = Wm * Wm.T
    C = np.eye(N)
    C[:n, :n] = fl(Cm)
    Cr = mpm(C[:n, :n])  # what lm_cov reads: C rounded once
    inv, panel = W.copy(), np.zeros((N, 64))
    inv[64:, :64] = C[64:, :64]
    for I in range(2):
        panel[64 * I:64 * I + 64] = C[64 * I:64 * I + 64, 64 * I:64 * I + 64]
    Tc = Cm - Qm * Qm.T
    cam = np.stack([fl(Tc[12 * c:12 * c + 12, 12 * c:12 * c + 12]) for c in range(p.n_cams)])
    cam0 = np.stack([fl(mp.diag([mpf(t) for t in sig[c]]) * Tc[12 * c:12 * c + 12, 12 * c:12 * c + 12] * mp.diag([mpf(t) for t in sig[c]]))
                     for c in range(p.n_cams)])
    lm, lm0 = np.zeros((p.n_lms, 3, 3)), np.zeros((p.n_lms, 3, 3))
    for l, (cams, Wl, His) in enumerate(lm_ops):
        Wl = [mp.matrix([[mpf(x) for x in row] for row in Wi]) for Wi in Wl]
        Sg = mp.matrix([[mpf(x) for x in row] for row in His])
        Tl = mp.zeros(12, 3)
        for i, ci in enumerate(cams):
            Tl += Qm[12 * ci:12 * ci + 12, :].T * Wl[i]
            for j, cj in enumerate(cams):
                Sg += Wl[i].T * Cr[12 * ci:12 * ci + 12, 12 * cj:12 * cj + 12] * Wl[j]
        Sg -= Tl.T * Tl
        D = mp.diag([mpf(t) for t in s[l]])
        lm[l], lm0[l] = fl(Sg), fl(D * Sg * D)
    sym = lambda B: np.triu(B) + np.triu(B, 1).transpose(0, 2, 1)  # (the device mirrors the upper triangle; so does the rounding)
    d = dict(R=R, Q=Q, inv=inv, panel=panel, cam=sym(cam), lm=sym(lm))
    out, bad = CB.check_all(sy, d)
    _report("exact small step 1 free gauge", out, bad)
    assert set(out) == {"assembly", "inverse", "camera", "lauum", "landmark", "gauge", "span"}
    out0, bad0 = CB.check_all(sy, dict(d, cam=sym(cam0), lm=sym(lm0)), coords=0)
    _report("exact small step 1 free gauge, own coordinates", {k: out0[k] for k in ("camera", "landmark")}, bad0)


@pytest.mark.parametrize("name,step,robust,lam", CB.CASES, ids=[f"{n}-{s}-{r}-{lam:g}" for n, s, r, lam in CB.CASES])
def test_both_emulation_orders_stay_inside_every_bound(name, step, robust, lam):
    sy = system(name, step, robust, lam)
    # lm_cov reads camera-pair blocks that lie on one, two and four tiles of C in every case; LAUUM checks every entry of every
    # tile, from the last block row (one K step) to the first (nb steps)
    assert CB.pair_tile_counts(sy.p, sy.dim) == {1, 2, 4} and sy.N // 64 >= 2
    for order in (0, 1):
        d = emulated(name, step, robust, lam, order)
        out, bad = CB.check_all(sy, d)
        _report(f"{name} step {step} {robust} lambda {lam:g} order {order}", out, bad)
        # the maps to the parameters' own coordinates (cov_finish, lm_cov) on the same blocks
        q = d["q"]
        d0 = dict(d, cam=CB.emulate_camera_coords(d["cam"], q.sig, getattr(q, "ncw", None), sy.dim), lm=CB.emulate_landmark_coords(d["lm"], q, sy.p))
        out0, bad0 = CB.check_all(sy, d0, coords=0)
        _report(f"{name} step {step} order {order} own coordinates", {k: out0[k] for k in ("camera", "landmark")}, bad0)


MUT_CASES = [("small", 1, "NONE", 0.0), ("p24", 2, "NONE", 0.0), ("small", 2, "NONE", 1e-4)]


@pytest.mark.parametrize("name,step,robust,lam", MUT_CASES, ids=[f"{n}-{s}-{lam:g}" for n, s, r, lam in MUT_CASES])
def test_every_mutation_is_reported_on_the_entries_it_touches(name, step, robust, lam):
    sy = system(name, step, robust, lam)
    clean = emulated(name, step, robust, lam, 0)
    muts = CB.mutations(clean, sy.p)
    assert len(muts) >= 10
    for mname, mutate, check, expected in muts:
        d = CB.emulate_case(sy.p, step == 2, 0, mutate)
        out, bad = CB.check_all(sy, d)
        assert not bad, (mname, bad)
        for k, (err, bound) in out.items():
            hit = CB.flagged(err, bound)
            if k != check:
                assert not hit, f"{mname}: {k} reports {len(hit)} entries"
                continue
            assert hit, f"{mname}: not reported by {check}"
            assert hit <= expected, f"{mname}: reported outside the entries it touches: {sorted(hit - expected)[:5]}"
        print(f"MUTATION {name} step {step} {mname}: {check} reports {len(CB.flagged(*out[check]))} entries, every other check clean")
    # sigma_j in place of sigma_i in cov_finish's map
    q = clean["q"]
    c = 1
    cam0 = CB.emulate_camera_coords(clean["cam"], q.sig, getattr(q, "ncw", None), sy.dim, {"sigma_j_for_i": c})
    err, bound = CB.camera_check(clean["inv"], clean["Q"], cam0, sy.n, sy.dim, 0, sy)["camera"]
    hit = CB.flagged(err, bound)
    assert hit and hit <= {144 * c + e for e in range(144)}, "sigma_j_for_i"


def test_the_normwise_bounds_accept_what_the_stage_checks_reject():
    """small, step 1, free gauge: the final blocks of a mutated chain against the long-double inverse under the bounds of the
    end-to-end GPU tests (n u cond |A^-1| per camera block, m u cond |K^-1| per landmark block), and the stage checks on the
    same buffers."""
    import landmark_covariance_reference as L
    name, step, robust, lam = "small", 1, "NONE", 0.0
    sy = system(name, step, robust, lam)
    ref = L.reference(name, step, robust, lam, True)
    clean = emulated(name, step, robust, lam, 0)

    def normwise_accepts(d):
        el = np.linalg.norm((d["lm"].astype(np.longdouble) - ref.want(False)).astype(F), axis=(1, 2))
        ec = np.linalg.norm((d["cam"].astype(np.longdouble) - ref.cameras.blocks).astype(F), axis=(1, 2))
        return bool(np.all(el <= ref.bound) and np.all(ec <= ref.cameras.bound)), float(el.max() / ref.bound), float(ec.max() / ref.cameras.bound)

    assert normwise_accepts(clean)[0]
    accepted = []
    for mname, mutate, check, expected in CB.mutations(clean, sy.p):
        d = CB.emulate_case(sy.p, False, 0, mutate)
        ok, rl, rc = normwise_accepts(d)
        out, _ = CB.check_all(sy, d)
        rejected = bool(CB.flagged(*out[check]))
        print(f"GAP {mname}: normwise bound {'accepts' if ok else 'rejects'} (landmarks {rl:.3g}, cameras {rc:.3g} of the bound); "
              f"{check} {'rejects' if rejected else 'accepts'}, worst err / bound {CB.worst(*out[check])[0]:.3g}")
        assert rejected
        if ok:
            accepted.append(mname)
    # On this case (cond_2 about 1e5) the normwise bounds turn out tighter than on the larger ones: they accept the perturbed
    # tile of C only.  The perturbed tile of W misses the camera bound by a factor 2.4, and no structural mutation passes:
    # each of them moves some block by far more than n u cond |A^-1|.  The perturbation case is the demonstration kept.
    # (when this was written they accepted nothing else: GAP lines above)
    assert "c_tile_1e-10" in accepted, accepted
