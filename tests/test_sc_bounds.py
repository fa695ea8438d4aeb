"""The references, bounds, emulations and mutations of tests/sc_bounds.py, without a GPU.

* The long-double references of the dense S, the block diagonal and S_cc against exact rational arithmetic
  (tests/exact_rational.py) on a tiny graph, inside the bounds sc_bounds gives for the long-double arithmetic itself
  (u = 2^-64).  Step 1 only: step 2's reflectors and 1 / z are irrational; its reference is held by the oracle below and by
  the two independent chains (pair form and sixty moments) agreeing to long-double rounding.
* The oracle's get_hb_pose / get_hb_joint and block_jacobi_inverse lie inside E(S), E(b) and the PRECOND residual bound.
* Both emulated summation orders of the assembly, the emulated sixty-moment chain and the emulated blocked factorisation lie
  inside every bound, on every shape of tests/test_gpu_sc_bounds.py at lambda = 1e-4 and 1.0; the conditions the helper
  assumes are asserted there for every shape, norm and lambda the GPU module uses: S_ref positive definite (smallest
  eigenvalue above lambda / 2), inv3_bound's determinant condition, ascending cameras inside every landmark.
  Worst err / bound of the emulations over all those shapes: S 0.064, b 0.049, BLOCKDIAG 0.15, S_cc forward 0.062, PRECOND
  residual 0.032 and symmetry 0.0021, factor 0.32 (medium_problem at lambda = 1), forward 0.022, back 0.059, chains 0.029;
  of the oracle: S 0.058, b 0.038, PRECOND 0.024; of the long-double references against the exact rationals, in their own
  long-double bounds: S 0.012, B_c 0.072, S_cc 0.015.
* Every mutation is reported on the entries it touches and on no other.  Reference-side mutations (assembly): the reported
  entries are a subset of the entries whose reference value moved, and contain every entry that moved by more than twice its
  bound.  Factor-side mutations: exactly the listed entries, every other check clean.
"""
import numpy as np
import pytest

import exact_rational as ER
import operand_bounds as OB
import sc_bounds as SB
from rounding_bounds import ULD

F = np.float64
LAMS = (1e-4, 1.0)


def _synth(n_c, n_l, n_o, seed):
    from povar_amd import synth
    return synth.make_problem(n_c, n_l, n_o, seed=seed)


# (name: step, constructor) -- the shapes of tests/test_gpu_sc_bounds.py
SHAPES = {
    "pose-5": (1, lambda r, lam: SB.pose_case(_synth(5, 30, 120, 5), r, lam)),
    "pose-16": (1, lambda r, lam: SB.pose_case(_synth(16, 100, 420, 16), r, lam)),
    "pose-26": (1, lambda r, lam: SB.pose_case(_synth(26, 160, 680, 26), r, lam)),
    "pose-medium": (1, lambda r, lam: SB.pose_case(_synth(49, 300, 1230, 49), r, lam)),
    "pose-edge": (1, SB.edge_pose),
    "joint-small": (2, lambda r, lam: SB.joint_case(_synth(6, 40, 150, 3), r, lam)),
    "joint-29": (2, lambda r, lam: SB.joint_case(_synth(29, 180, 760, 29), r, lam)),
    "joint-64": (2, lambda r, lam: SB.joint_case(_synth(64, 400, 1800, 64), r, lam)),
    "joint-edge": (2, SB.edge_joint),
}
SMALL = ("pose-5", "pose-16", "joint-small")
_cache = {}


def system(name, robust="NONE", lam=SB.LAM):
    """The reference of one case, computed once and left unchanged."""
    key = (name, robust, lam)
    if key not in _cache:
        step, make = SHAPES[name]
        p = make(robust, lam)
        _cache[key] = SB.dense_system(p, step == 2)
    return _cache[key]


def _upper(n):
    return np.triu(np.ones((n, n), dtype=bool))


def _ld_fraction(x):
    hi = float(x)
    return ER.F(hi) + ER.F(float(x - np.longdouble(hi)))


def test_step1_references_against_exact_rationals():
    rng = np.random.default_rng(5)
    n_c, degs = 4, [2, 3, 4, 2, 3, 4, 2]
    cam_idx = np.concatenate([np.sort(rng.choice(n_c, k, replace=False)) for k in degs])
    lm_off = np.concatenate([[0], np.cumsum(degs)])
    cams = np.zeros((n_c, 12))
    cams[:, :8] = rng.normal(size=(n_c, 8))
    cams[:, 11] = 1.0
    X = rng.normal(size=(len(degs), 3))
    P = cams[cam_idx].reshape(-1, 3, 4)
    obs = np.einsum("nij,nj->ni", P[:, :2, :3], X[np.repeat(np.arange(len(degs)), degs)]) + P[:, :2, 3] + rng.normal(scale=0.05, size=(len(cam_idx), 2))
    p = OB.Pose(n_c, lm_off, cam_idx, obs, cams, X, SB.ALPHA, SB.LAM, scale_jl=False)
    sy = SB.dense_system(p, False, u=ULD)  # the bounds of the long-double arithmetic itself
    ex = ER.ExactStep1(SB.ALPHA, n_c, lm_off, cam_idx, obs, cams, X)
    n = 12 * n_c
    sig = [_ld_fraction(t) for t in sy.R.aux["chain"]["sig"].reshape(-1)]
    lam = ER.F(SB.LAM)
    hpp = ex.hpp()
    e0 = [ex.e0([ER.F(int(i == j)) for i in range(n)]) for j in range(n)]  # column j of E0
    worst = {"S": 0.0, "B": 0.0, "Scc": 0.0}
    for i in range(n):
        for j in range(n):
            ci, cj = i // 12, j // 12
            h = hpp[ci][i % 12][j % 12] if ci == cj else ER.F(0)
            s_ex = sig[i] * (h - e0[j][i]) * sig[j] + (lam if i == j else 0)
            err = abs(float(_ld_fraction(sy.S[i, j]) - s_ex))
            assert err <= sy.ES[i, j], (i, j, err, sy.ES[i, j])
            if sy.ES[i, j] > 0:
                worst["S"] = max(worst["S"], err / sy.ES[i, j])
            else:
                assert s_ex == 0 and sy.S[i, j] == 0  # no landmark is seen by both cameras
            if ci == cj:
                b_ex = sig[i] * h * sig[j] + (lam if i == j else 0)
                eb = abs(float(_ld_fraction(sy.B[ci, i % 12, j % 12]) - b_ex))
                es = abs(float(_ld_fraction(sy.Scc[ci, i % 12, j % 12]) - s_ex))
                assert eb <= sy.EB[ci, i % 12, j % 12] and es <= sy.EScc[ci, i % 12, j % 12], (i, j, eb, es)
                if sy.EB[ci, i % 12, j % 12] > 0:  # (a structural zero of Hpp otherwise: both are exactly 0)
                    worst["B"] = max(worst["B"], eb / sy.EB[ci, i % 12, j % 12])
                worst["Scc"] = max(worst["Scc"], es / sy.EScc[ci, i % 12, j % 12])
    print("exact rationals: worst err / long-double bound", worst)
    assert 0 < worst["S"] < 1


def _oracle_system(p, joint):
    from oracle import povar_oracle as O
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=p.robust, huber=p.huber)
    if not joint:
        st, ok = orc.linearize_pose(p.alpha, p.cams, p.lms)
        orc.scale_jp_cols_pose(st, 1.0 / (p.eps + np.sqrt(orc.jp_diag2_pose(st))))
        S, b = orc.get_hb_pose(st, p.lam)
        return S, b, orc.block_jacobi_inverse(S, 12)
    st_h, ok = orc.linearize_homogeneous(p.cams, p.lms)
    diag2 = orc.jp_diag2_homogeneous(st_h)
    orc.scale_jl_cols_homogeneous(st_h)
    orc.scale_jp_cols_joint(st_h, 1.0 / (p.eps + np.sqrt(diag2)))
    st_n = orc.linearize_nullspace(p.cams, p.lms, st_h)
    S, b = orc.get_hb_joint(st_h, st_n, p.lam)
    return S, b, orc.block_jacobi_inverse(S, 11)


@pytest.mark.parametrize("name,robust", [("pose-5", "NONE"), ("pose-16", "HUBER"), ("pose-medium", "NONE"), ("joint-small", "HUBER"),
                                         ("joint-29", "NONE"), ("pose-edge", "NONE"), ("joint-edge", "NONE")])
def test_the_oracle_lies_inside_the_bounds(name, robust):
    sy = system(name, robust)
    S, b, minv = _oracle_system(sy.p, sy.joint)
    n = sy.n
    r, i, over = SB.worst(np.abs((S - sy.S).astype(F)), sy.ES)
    assert over == 0, ("S", divmod(i, n), r)
    rb, i, over = SB.worst(np.abs((b - sy.b).astype(F)), sy.Eb)
    assert over == 0, ("b", i, rb)
    res, Rb, asym, ab = SB.precond_check(sy, minv.reshape(-1, sy.dim, sy.dim))
    rp, i, over = SB.worst(res, Rb)
    assert over == 0, ("precond", i, rp)
    assert SB.worst(asym, ab)[2] == 0
    # where no landmark is shared the oracle has exact zeros too, and lambda I on the cameras nobody observes
    assert np.all(S[(sy.cnt == 0) & (sy.Sm == 0)] == 0.0)
    for c in np.flatnonzero(sy.p.n_c == 0):
        sl = slice(sy.dim * c, sy.dim * c + sy.dim)
        assert np.array_equal(S[sl, sl], sy.p.lam * np.eye(sy.dim)) and np.all(b[sl] == 0.0)
    print(f"oracle {name} {robust}: S {r:.3g} b {rb:.3g} precond {rp:.3g}")


def _conditions(sy):
    p = sy.p
    assert float(sy.R.aux["det_ratio"].max()) < OB.DET_RATIO
    Sf = sy.S.astype(F)
    assert np.array_equal(Sf, Sf.T)
    assert np.linalg.eigvalsh(Sf)[0] > 0.5 * p.lam, "S_ref is not positive definite"
    for c in np.flatnonzero(p.n_c == 0):
        sl = slice(sy.dim * c, sy.dim * c + sy.dim)
        assert np.array_equal(Sf[sl, sl], p.lam * np.eye(sy.dim)) and np.all(sy.ES[sl, :] == 0) and np.all(sy.b[sl] == 0) and np.all(sy.Eb[sl] == 0)
    z = (sy.cnt == 0) & (sy.Sm == 0)  # no landmark is seen by both cameras: exactly 0
    assert np.all(sy.S[z] == 0) and np.all(sy.ES[z] == 0)
    assert sy.N <= 2048
    # the two reference chains (pair form, sixty moments) are one matrix to long-double rounding
    d = np.abs((SB.diag_blocks(sy.S, sy.dim) - sy.Scc).astype(F))
    assert d.max() <= 2.0 ** -50 * np.abs(sy.Scc.astype(F)).max()


def _emulation_ratios(sy, order):
    p, n, N = sy.p, sy.n, sy.N
    M, Bc, q = SB.emulate_assembly(p, sy.joint, order)
    out = {}
    out["S"] = SB.worst(np.where(_upper(n), np.abs((M[:n, :n] - sy.S).astype(F)), 0.0), sy.ES)
    out["b"] = SB.worst(np.abs((-M[:n, N] - sy.b).astype(F)), sy.Eb)
    out["blockdiag"] = SB.worst(np.abs((Bc - sy.B).astype(F)), sy.EB)
    X, A = SB.emulate_precond(p, sy.joint, q)
    res, Rb, asym, ab = SB.precond_check(sy, X)
    out["precond"], out["precond_sym"] = SB.worst(res, Rb), SB.worst(asym, ab)
    out["scc"] = SB.worst(np.abs((A - sy.Scc).astype(F)), sy.EScc)
    buf, info = SB.emulate_factor(M)
    assert info == 0
    fc = SB.factor_check(sy, buf, Bc)
    assert fc.pop("padding") == []
    out.update({k: SB.worst(*v) for k, v in fc.items()})
    assert np.all(np.isfinite(buf))
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_emulations_inside_every_bound(name):
    small = name in SMALL
    for robust in (("NONE", "HUBER") if small or name.endswith("edge") else ("NONE",)):
        for lam in LAMS:
            if name.endswith("edge") and (lam != SB.LAM or robust == "HUBER"):
                sy = SB.dense_system(SHAPES[name][1](robust, lam), SHAPES[name][0] == 2)  # (conditions only: not kept)
                _conditions(sy)
                continue
            sy = system(name, robust, lam)
            _conditions(sy)
            for order in (0, 1):
                out = _emulation_ratios(sy, order)
                bad = {k: v for k, v in out.items() if v[2]}
                assert not bad, (name, robust, lam, order, bad)
                print(f"emulation {name} {robust} lam={lam:g} order {order}: " + " ".join(f"{k}={v[0]:.3g}" for k, v in out.items()))


def test_the_shapes_reach_what_they_are_there_for():
    assert (system("pose-5").n, system("pose-5").N) == (60, 64)
    assert (system("pose-16").n, system("pose-16").N) == (192, 192)
    assert (system("pose-26").n, system("pose-26").N) == (312, 320)
    assert (system("pose-medium").n, system("pose-medium").N) == (588, 640)
    assert (system("joint-small").n, system("joint-small").N) == (66, 128)
    assert (system("joint-29").n, system("joint-29").N) == (319, 320)
    assert (system("joint-64").n, system("joint-64").N) == (704, 704)
    for name in ("pose-edge", "joint-edge"):
        p = system(name).p
        assert sorted(p.n_l.tolist())[-5:] == [33, 64, 65, 97, 140] and (p.n_l == 2).sum() >= 120 and (p.n_c == 0).sum() == 3


@pytest.mark.parametrize("name", ["pose-16", "pose-26", "joint-small", "joint-29"])
def test_every_mutation_is_reported_on_its_own_entries(name):
    sy = system(name)
    p, n, N, dim = sy.p, sy.n, sy.N, sy.dim
    M, Bc, q = SB.emulate_assembly(p, sy.joint, 0)
    X, _ = SB.emulate_precond(p, sy.joint, q)
    up = _upper(n)
    seen = []
    for mname, side, mut, check, expected in SB.mutations(sy):
        seen.append(mname)
        if side == "reference":
            sm = SB.dense_system(p, sy.joint, mutate=mut, R=sy.R)
            if check == "S":
                moved = np.where(up, np.abs((sm.S - sy.S).astype(F)), 0.0)
                touched = set(np.flatnonzero(moved.reshape(-1) > 0).tolist())
                must = set(np.flatnonzero(moved.reshape(-1) > 2 * sy.ES.reshape(-1)).tolist())
                got = SB.flagged(np.where(up, np.abs((M[:n, :n] - sm.S).astype(F)), 0.0), sm.ES)
                assert must and must <= got <= touched, (mname, len(must), len(got), len(touched))
                if expected is not None:
                    assert touched <= expected and got <= expected, mname
                assert np.array_equal(sm.Scc, sy.Scc) or mname in ("sigma_wrong_camera", "hll_undamped")
            else:
                res, Rb, _, _ = SB.precond_check(sm, X)
                got = set(np.flatnonzero((~(res <= Rb)).reshape(p.n_cams, -1).any(1)).tolist())
                assert got == expected, (mname, got, expected)
                assert np.array_equal(sm.S, sy.S)  # (the dense chain does not read the moments)
        else:
            sf, Mf, Bf = sy, M, Bc
            if mname == "subtile_skipped":  # (at lambda = 1e-4 the trailing matrix turns indefinite and chol_diag says so)
                sf = system(name, "NONE", 1.0)
                Mf, Bf, _ = SB.emulate_assembly(sf.p, sf.joint, 0)
                assert SB.emulate_factor(M, mut)[1] == 1
            buf, info = SB.emulate_factor(Mf, mut)
            fc = SB.factor_check(sf, buf, Bf)
            if check == "padding":
                assert info == 1 and fc["padding"], mname
                continue
            assert info == 0 and fc.pop("padding") == []
            for k, v in fc.items():
                if k == "chains":
                    continue
                got = SB.flagged(*v)
                assert got == (expected if k == check else set()), (mname, k, sorted(got)[:8], sorted(expected)[:8])
    want = {"pair_dropped", "pair_transposed", "sigma_wrong_camera", "moment_last_summand", "rhs_skipped", "subtile_skipped", "back_row_skipped"}
    want |= {"hll_undamped"} if sy.joint else set()
    want |= {"pad_zero"} if N > n else set()
    want -= {"subtile_skipped"} if n < (SB.CH_OB if N > SB.CH_OB else SB.CH_NB) + 48 else set()
    assert set(seen) == want, (seen, want)


def test_k_factor_and_k_back_count_what_the_blocked_code_does():
    kf, kb = SB.k_factor(640), SB.k_back(640)
    assert kf[0] == 2 and kf[63] == 3 * 63 + 2 and kf[64] == 64 + 2 + 2 and kf[256] == 256 + 2 + 2 and kf[639] == 256 + 2 * (2 + 1) + 3 * 63 + 2
    assert kb[639] == 64 + 4 and kb[0] == 64 + 2 * 9 + 4
    # exact_gram is exact on integers and reports what it leaves out
    rng = np.random.default_rng(0)
    R = np.triu(rng.integers(-2 ** 20, 2 ** 20, size=(128, 128)).astype(F))
    G, miss = SB.exact_gram(R)
    assert np.array_equal(G.astype(F), R.T @ R) and np.all(miss <= 16 * ULD * (np.abs(R).T @ np.abs(R)) * (1 + 1e-5))
