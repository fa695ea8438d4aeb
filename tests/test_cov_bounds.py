"""The bounds, emulations and mutations of tests/cov_bounds.py, without a GPU.

* Exact arithmetic on a tiny system (`small`, step 1, free gauge: n = 72, N = 128), built independently from the reference's
  formulas with tests/exact_rational.py: S, the per-observation E_i Hll^-1 and the gauge generators are exact rationals; the
  irrational stages (Gram-Schmidt, Cholesky, inverse, C, the blocks) run in 60-digit arithmetic, each from the once-rounded
  output of the one before.  All seven checks (assembly with Q Q^T, gauge, span, inverse, camera, lauum, landmark) and both
  coordinate maps admit the once-rounded results: worst err / bound assembly 0.0058, gauge 0.0089, span 1.1e-5, inverse
  0.90, camera 0.081, lauum 0.015, landmark 3.1e-4 (own coordinates: camera 0.018, landmark 5.2e-4).  The same chain carries
  all 36 camera pairs and twenty-odd pairs of each other kind through tests/pair_bounds.py (pair_check, both coordinate
  systems): pair_cc 0.81, pair_cl 0.0012, pair_ll 1.9e-5 (own coordinates 0.024, 7.0e-4, 1.9e-5).  Step 1 only: step 2's
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
* OBSERVATION (obs_cov's rows; cov_bounds.OBS_CASES: small free / damped / HUBER, medium damped, tracks): both emulated orders
  stay inside the bound on every entry of every row, all-landmark call and id list (reversed, one landmark twice); worst
  err / bound h 0.0072, c_* 0.013 (medium, step 1, lambda 1).  In the free gauge |sum h_i - rank J| <= 6.8e-13 against a summed
  bound of 2.5e-7 .. 6.6e-6.  The new bound over the normwise one of tests/observation_covariance_reference.py on the same
  entries, median (largest), information only -- step 1: small 7.4e-4 (1.6), lambda 1e-4 6.1e-7 (2.2e-3), HUBER 7.4e-4 (1.9),
  medium 1e-4 1.3e-7 (6.3), 1 1.6e-6 (35), tracks 5.5e-5 (0.049); step 2: small 0.043 (235), lambda 1e-4 9.3e-4 (5.2), HUBER 0.039
  (213), medium 1e-4 1.6e-5 (2.1e3), 1 0.14 (7.5), tracks 1.4e-4 (6.1).  Where it is the wider one a small y2 or the charged
  cancellation of the free gauge dominates the entry.
* The nine mutations of cov_bounds.mutations_obs are reported on the rows and in the columns they touch and nowhere else.
  Seen (both steps unless said): tracks: c_tile_1e-10, iz_f32, r_f32, corrected, kii_any_chunk, skip_last_j, unmasked, stale_oj;
  small HUBER: sw_f32, r_f32, corrected, iz_f32 (step 2); small lambda 1e-4: r_f32, iz_f32 (step 2).  iz_f32 changes nothing on
  small in step 1 (the generator's cameras have y2 = 1: 1 / y2 is exact), which is why tracks' cameras have another third
  row.  err / bound on the touched rows, new | normwise: c_tile_1e-10 3.1 .. 3.8 | 2.8e-4 .. 3.2e-4; iz_f32 1.4e2 .. 7.4e5 | 0.018 ..
  4.0e2; r_f32 5.5e3 .. 1.4e5 | 0.056 .. 4.0e2; sw_f32 3.5e3 .. 4.7e4 | 12 .. 122; the structural ones 4e9 .. 2e12 | 2e5 .. 4e8.
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
    mp_ops = []  # per landmark, 60 digits: (cameras, W_i, T_l, Hll^-1) for the pair blocks below
    for l, (cams, Wl, His) in enumerate(lm_ops):
        Wl = [mp.matrix([[mpf(x) for x in row] for row in Wi]) for Wi in Wl]
        Sg = mp.matrix([[mpf(x) for x in row] for row in His])
        Tl = mp.zeros(12, 3)
        for i, ci in enumerate(cams):
            Tl += Qm[12 * ci:12 * ci + 12, :].T * Wl[i]
            for j, cj in enumerate(cams):
                Sg += Wl[i].T * Cr[12 * ci:12 * ci + 12, 12 * cj:12 * cj + 12] * Wl[j]
        Sg -= Tl.T * Tl
        mp_ops.append((cams, Wl, Tl, mp.matrix([[mpf(x) for x in row] for row in His])))
        D = mp.diag([mpf(t) for t in s[l]])
        lm[l], lm0[l] = fl(Sg), fl(D * Sg * D)
    sym = lambda B: np.triu(B) + np.triu(B, 1).transpose(0, 2, 1)  # (the device mirrors the upper triangle; so does the rounding)
    d = dict(R=R, Q=Q, inv=inv, panel=panel, cam=sym(cam), lm=sym(lm))
    out, bad = CB.check_all(sy, d)
    _report("exact small step 1 free gauge", out, bad)
    assert set(out) == {"assembly", "inverse", "camera", "lauum", "landmark", "gauge", "span"}
    out0, bad0 = CB.check_all(sy, dict(d, cam=sym(cam0), lm=sym(lm0)), coords=0)
    _report("exact small step 1 free gauge, own coordinates", {k: out0[k] for k in ("camera", "landmark")}, bad0)
    # The blocks of parameter pairs (tests/pair_bounds.py) from the same once-rounded C and Q: all 36 camera pairs, twenty-odd
    # pairs of each other kind (both orders, own pairs, camera 5 across the 64-edge), an independent check of the formulas of
    # pair_reference and of its map to parameter coordinates, as the lines above are of landmark_reference.
    import pair_bounds as PB
    CAM, LM = PB.CAMERA, PB.LANDMARK
    rng = np.random.default_rng(9)
    cl = [(CAM, int(c), LM, int(l)) for c, l in zip(rng.integers(0, p.n_cams, 14), rng.integers(0, p.n_lms, 14))] + [(CAM, 5, LM, 0), (CAM, 0, LM, 39)]
    ll = [(LM, int(a), LM, int(b)) for a, b in rng.integers(0, p.n_lms, (14, 2))] + [(LM, l, LM, l) for l in (0, 7, 39)]
    pairs = ([(CAM, a, CAM, b) for a in range(p.n_cams) for b in range(p.n_cams)] + cl + [(kb, b, ka, a) for ka, a, kb, b in cl[:6]] +
             ll + [(kb, b, ka, a) for ka, a, kb, b in ll[:4]])
    crow = lambda c: slice(12 * c, 12 * c + 12)
    dmat = {CAM: lambda c: mp.diag([mpf(t) for t in sig[c]]), LM: lambda l: mp.diag([mpf(t) for t in s[l]])}

    def canonical(ka, a, kb, b):
        if ka == CAM and kb == CAM:
            return Cr[crow(a), crow(b)] - Qm[crow(a), :] * Qm[crow(b), :].T
        if ka == CAM:
            cams, Wl, Tl, _ = mp_ops[b]
            X = Qm[crow(a), :] * Tl
            for j, cj in enumerate(cams):
                X -= Cr[crow(a), crow(cj)] * Wl[j]
            return X
        (ca, Wa, Ta, Ha), (cb, Wb, Tb, _) = mp_ops[a], mp_ops[b]
        X = (Ha if a == b else mp.zeros(3, 3)) - Ta.T * Tb
        for i, ci in enumerate(ca):
            for j, cj in enumerate(cb):
                X += Wa[i].T * Cr[crow(ci), crow(cj)] * Wb[j]
        return X

    blocks = {1: [], 0: []}
    for ka, a, kb, b in pairs:
        flip = ka == LM and kb == CAM
        X = canonical(kb, b, ka, a) if flip else canonical(ka, a, kb, b)
        X0 = (dmat[kb](b) if flip else dmat[ka](a)) * X * (dmat[ka](a) if flip else dmat[kb](b))
        for coords, Y in ((1, X), (0, X0)):
            Y = fl(Y)
            Y = np.triu(Y) + np.triu(Y, 1).T if (ka == kb and a == b) else Y  # (the device mirrors the upper triangle)
            blocks[coords].append(Y.T if flip else Y)
    Cs = CB.c_symmetric(inv, panel)
    for coords in (1, 0):
        res = PB.pair_check(sy, Cs, Q, pairs, blocks[coords], coords)
        _report(f"exact small step 1 free gauge, pairs, coords {coords}", {k: res[k] for k in PB.CHECKS}, res["exact"])
        assert all(np.any(res[k][1] > 0) for k in PB.CHECKS)


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
        d0.pop("obs", None)  # (the rows have no coordinates: checked once, above)
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
        d = CB.emulate_case(sy.p, step == 2, 0, mutate, obs=False)  # (obs_cov's own mutations: at the end of this module)
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
        d = CB.emulate_case(sy.p, False, 0, mutate, obs=False)
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


# ======== OBSERVATION: obs_cov's rows (module docstring, last item)
def _obs_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-{c[3]:g}"


def _old_reference(name, step, robust, lam):
    """The long-double Schur-route rows and the normwise bound tests/test_gpu_observation_covariance.py holds the rows to."""
    import observation_covariance_reference as OC
    return OC.reference(name, step, robust, lam, lam == 0.0)


def _id_list(p):
    """Reversed order, one landmark twice: row0 and ids index differently from the workgroup's number."""
    k = p.n_l
    pick = sorted({int(np.argmax(k)), int(np.argmin(k)), p.n_lms - 1, 0, int(np.flatnonzero(k >= 3)[0])})
    return np.array(pick[::-1] + [pick[-1]], dtype=np.int32)


def _assert_shape_reaches_the_loop_edges(name, step, sy):
    """What each shape is there for, asserted on the shape itself (obs_cov :597-648)."""
    import landmark_covariance_reference as L
    p, dim = sy.p, sy.dim
    chunk = CB.obs_chunk(dim)
    k = set(p.n_l.tolist())
    assert {1, 2, 4} <= CB.pair_tile_counts(p, dim)
    # a camera across a 64-edge in a track with another camera: all k^2 pairs are walked, so it is the i and the j of pairs
    # whose blocks lie on two tiles, and its own block on four
    strad = {c for c in range(p.n_cams) if (dim * c) // 64 != (dim * c + dim - 1) // 64}
    assert any(len(set(p.cam_idx[a:b].tolist()) & strad) and b - a >= 2 for a, b in zip(p.lm_off[:-1], p.lm_off[1:]))
    if name in ("small", "tracks"):
        assert min(k) == 2  # the shortest track the generator makes (synth._degrees)
    if name == "tracks":
        assert set(L.TRACK_EDGES) <= k and {15, 16, 17} <= k  # the pass of 16 groups (`live`)
        assert {chunk - 1, chunk, chunk + 1} <= k  # 63, 64, 65 (step 1) or 31, 32, 33 (step 2)
        assert sy.N <= 832
        assert np.any(CB.observation_operands(sy).y[:, 2] != 1)  # (1 / y2 is not exact: the rounding of iz can show in step 1 too)
        if step == 2:
            assert max(k) > 2 * chunk  # three chunks: oj is staged again in every pass, `staged` carries over from one ic to the next
    if sy.p.robust == "HUBER":
        assert np.any(CB.emulated(name, step, "HUBER", 0.0, 0)["q"].sw < 1)


@pytest.mark.parametrize("name,step,robust,lam", CB.OBS_CASES, ids=[_obs_id(c) for c in CB.OBS_CASES])
def test_observation_rows_of_both_emulation_orders_stay_inside_the_bound(name, step, robust, lam):
    """Every entry of every row, both summation orders, an id list with a duplicate; in the free gauge sum h_i = rank J inside
    the summed bound; the gain over the normwise bound of the end-to-end test (printed: information, not a threshold)."""
    sy = system(name, step, robust, lam)
    p = sy.p
    _assert_shape_reaches_the_loop_edges(name, step, sy)
    n_obs = len(p.cam_idx)
    ids = _id_list(p)
    old = _old_reference(name, step, robust, lam)
    for order in (0, 1):
        d = emulated(name, step, robust, lam, order)
        tag = f"{name} step {step} {robust} lambda {lam:g} order {order}"
        if (name, step, robust, lam) in CB.CASES:  # (every other stage of these: test_both_emulation_orders_stay_inside_every_bound)
            res = CB.observation_check(sy, CB.c_symmetric(d["inv"], d["panel"])[:sy.n, :sy.n], d["obs"])
            bad = res.pop("exact")
            out = res
        else:
            out, bad = CB.check_all(sy, d)
        assert out["observation_h"][0].shape == (n_obs,) and out["observation_c"][0].shape == (n_obs, 3)  # no entry skipped
        _report(tag, out, bad)
        if lam == 0.0:
            rank = sy.n + 3 * p.n_lms - d["Q"].shape[1]
            assert rank == old.rank
            gap, room = abs(float(d["obs"][:, 0].sum()) - rank), float(out["observation_h"][1].sum())
            print(f"OBSRANK {tag}: |sum h - {rank}| = {gap:.3g}, summed bound {room:.3g}")
            assert gap <= room
        # the id list: reversed, one landmark twice, each row against its own landmark
        sig = CB.emulate_landmarks(p, d["q"], d["inv"], d["panel"], None, sy.dim, order, ids=ids)
        rows = CB.emulate_observations(p, d["q"], d["inv"], d["panel"], sig, sy.dim, order, ids=ids)
        res = CB.observation_check(sy, CB.c_symmetric(d["inv"], d["panel"])[:sy.n, :sy.n], rows, ids)
        _report(tag + " id list", {k: v for k, v in res.items() if k != "exact"}, res["exact"])
        start = np.r_[0, np.cumsum(p.n_l[ids])]
        for t, l in enumerate(ids):  # (and the same bits as the all-landmark call: a row depends on its landmark alone)
            assert np.array_equal(rows[start[t]:start[t + 1]], d["obs"][p.lm_off[l]:p.lm_off[l + 1]])
    new = np.concatenate([out["observation_h"][1][:, None], out["observation_c"][1]], 1)
    ratio = new / old.bound
    print(f"OBSGAIN {name} step {step} {robust} lambda {lam:g}: new bound / normwise bound median {np.median(ratio):.3g}, largest {ratio.max():.3g}")


def test_a_reference_side_defect_is_reported_on_clean_rows():
    """The long-double formula of observation_reference itself: with Sigma_l taken with the gauge correction, or the cross
    term dropped, the clean emulated rows leave the bound (small, step 1, free gauge)."""
    case = ("small", 1, "NONE", 0.0)
    sy, d = system(*case), emulated(*case, 0)
    Cs = CB.c_symmetric(d["inv"], d["panel"])[:sy.n, :sy.n]
    for mutate in ({"Q": d["Q"]}, {"no_cross": True}):
        res = CB.observation_check(sy, Cs, d["obs"], ref=CB.observation_reference(sy, Cs, mutate=mutate))
        assert CB.flagged(*res["observation_h"]) and CB.flagged(*res["observation_c"]), mutate.keys()


@pytest.mark.parametrize("step", [1, 2])
def test_every_observation_mutation_is_reported_on_the_rows_it_touches(step):
    """cov_bounds.mutations_obs on `tracks` (the loop edges, a camera across a 64-edge, the free gauge), `small` with HUBER (a
    weight below 1) and `small` damped.  Each defect lives in obs_cov alone: the buffers every other check of check_all reads
    are those of the clean chain, which the test above holds inside every bound.  Reported: on the rows it touches and no
    other, in the columns it touches and no other.  Printed per case: err / bound under the new bound and under the normwise
    bound of tests/observation_covariance_reference.py (against the long-double Schur route) on the touched rows: the second
    column says what the suite could see before."""
    cases = [("tracks", step, "NONE", 0.0), ("small", step, "HUBER", 0.0), ("small", step, "NONE", 1e-4)]
    seen, unseen = {}, {}
    for name, step, robust, lam in cases:
        sy, d = system(name, step, robust, lam), emulated(name, step, robust, lam, 0)
        Cs = CB.c_symmetric(d["inv"], d["panel"])[:sy.n, :sy.n]
        ref = CB.observation_reference(sy, Cs)
        clean = CB.observation_check(sy, Cs, d["obs"], ref=ref)
        assert not clean["exact"] and not CB.flagged(*clean["observation_h"]) and not CB.flagged(*clean["observation_c"])
        old = _old_reference(name, step, robust, lam)
        for mname, mutate, checks, touched in CB.mutations_obs(sy, d):
            assert touched, mname
            rows = CB.emulate_obs_mutation(sy, d, 0, mutate)
            res = CB.observation_check(sy, Cs, rows, ref=ref)
            hit = {"observation_h": CB.flagged(*res["observation_h"]), "observation_c": {i // 3 for i in CB.flagged(*res["observation_c"])}}
            for check in hit:
                if check not in checks:
                    assert not hit[check], f"{name} step {step} {mname}: {check} reports rows {sorted(hit[check])[:5]}"
                assert hit[check] <= touched, f"{name} step {step} {mname}: {check} reports rows it does not touch: {sorted(hit[check] - touched)[:5]}"
            t = sorted(touched)
            cols = [0] if checks == ("observation_h",) else [1, 2, 3] if checks == ("observation_c",) else [0, 1, 2, 3]
            e_new = np.concatenate([res["observation_h"][0][:, None], res["observation_c"][0]], 1)[np.ix_(t, cols)]
            b_new = np.concatenate([res["observation_h"][1][:, None], res["observation_c"][1]], 1)[np.ix_(t, cols)]
            e_old = np.abs((rows.astype(np.longdouble) - old.rows).astype(F))[np.ix_(t, cols)]
            ok = all(hit[c] for c in checks)
            print(f"OBSMUTATION {name} step {step} {robust} lambda {lam:g} {mname}: err / bound new {CB.worst(e_new, b_new)[0]:.3g}, "
                  f"normwise {CB.worst(e_old, old.bound[np.ix_(t, cols)])[0]:.3g}; reported on {len(hit['observation_h'])} h rows, "
                  f"{len(hit['observation_c'])} c rows of {len(touched)} touched{'' if ok else ' -- NOT SEEN on this case'}")
            (seen if ok else unseen).setdefault(mname, []).append(name + " " + robust)
    want = {"c_tile_1e-10", "sw_f32", "iz_f32", "r_f32", "corrected", "kii_any_chunk", "skip_last_j", "unmasked", "stale_oj"}
    assert want <= set(seen) | set(unseen), "a mutation of the list found no shape"
    print(f"OBSMUTATION step {step}: seen {seen}; not seen {unseen}")
    assert want <= set(seen), f"not seen on any case of step {step}: {sorted(want - set(seen))}"
