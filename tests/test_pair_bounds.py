"""The bounds, emulation and mutations of tests/pair_bounds.py (pair_cc, pair_cl, pair_ll), without a GPU.  The whole module
takes about 1 min 50 s on its own, 1 min 10 s of it the mutation cases; in a run of the whole suite the emulated chains of
cov_bounds (about 30 s of that) are those tests/test_cov_bounds.py has already built.

* Satisfiable: both emulated summation orders lie inside every bound on every entry of every block, in both coordinate
  systems, on every case of pair_bounds.PAIR_CASES; damped, the solver-coordinate camera-camera blocks are C's entries bit for
  bit (bound zero).  Worst err / bound over all of them, solver | parameter coordinates: pair_cc 0.94 | 0.19 (a single
  rounding of C against a bound of one rounding), pair_cl 0.010 | 0.011, pair_ll 0.0050 | 0.0038; the operand bounds of sigma,
  Hll^-1 and the column scales carry the last two, as they carry landmark's.
* Shapes: every request asserts on itself what it is there for (_assert_request_reaches_the_edges).
* Mutations: every defect of pair_bounds.mutations_pairs is reported by its own check on the entries it touches and on no
  other, every other check stays clean; the perturbed tile of C (c_tile_1e-10) leaves the pair checks clean against its own C
  and is reported by cov_bounds.lauum_check.  Seen: the eighteen defects, 74 reports over the five shapes: all but the following on
  every shape; the free gauge's (cl_t_sign, cc_q_rows, t_group_skipped) on the four free-gauge shapes; ll_oj_stale,
  ll_tl_every_jc, ll_tm_every_ic on tracks alone (step 1: the track of 65 with itself; step 2: 33, 64, 65 on both sides);
  cc_n_a_for_b in step 2; c_tile_1e-10 where a requested camera pair reads rows 64 I, 64 I + 1 of an off-diagonal tile (not
  tracks step 1).  An ignored `tr` and the missing `same` swap also (the latter only) break the bitwise facts.
* The gap (small, step 1, free gauge): the normwise bound of tests/test_gpu_pair_covariance.py on the blocks of every
  mutated emulation.  It accepts c_tile_1e-10 (0.11 of the bound) and the missing `same` swap (7.7e-5); pair_check against
  the clean C reports the tile at 9e5 times its bound on 648 of the 1 909 entries that read it (all 64 camera-camera entries,
  575 camera-landmark, 9 landmark-landmark) and on no other -- where the two perturbed rows of C carry less than the operand
  errors charged on the whole sum, 1e-10 of them is inside the bound.  Every structural defect moves some block by 4e7 ..
  6e9 normwise bounds and by 4e11 .. 2e16 of the new one.  New bound / normwise bound per block, median (largest): pair_cc
  1.8e-7 (9.5e-7), pair_cl 2.2e-4 (0.055), pair_ll 0.0061 (2.1).
* Exact arithmetic: tests/test_cov_bounds.py::test_exact_arithmetic_on_a_tiny_system_stays_inside_every_bound carries all
  36 camera pairs and twenty-odd pairs of each other kind through pair_check in both coordinate systems (the 60-digit chain
  is built once, there).
"""
import numpy as np
import pytest

import cov_bounds as CB
import pair_bounds as PB
import pair_covariance_reference as P

F = np.float64
CAM, LM = P.CAMERA, P.LANDMARK


def _id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-{c[3]:g}"


def _run(sy, d, order, pairs, coords, mutate=None):
    return PB.emulate_pairs(sy.p, d["q"], d["inv"], d["panel"], d["Q"], sy.dim, order, pairs, coords, mutate)


def _assert_request_reaches_the_edges(name, step, sy, pairs):
    """What each request is there for, asserted on the request itself (pair_cc :640-683, pair_cl :686-784, pair_ll :787-902)."""
    p, dim = sy.p, sy.dim
    chunk = PB.chunk_of(dim)
    k = p.n_l
    cams_of = lambda l: p.cam_idx[p.lm_off[l]:p.lm_off[l + 1]]
    strad = {c for c in range(p.n_cams) if (dim * c) // 64 != (dim * c + dim - 1) // 64}
    span = lambda c: 2 if c in strad else 1
    cc = [(a, b) for ka, a, kb, b in pairs if ka == kb == CAM]
    cl = [(a, b) if ka == CAM else (b, a) for ka, a, kb, b in pairs if ka != kb]
    ll = [(a, b) for ka, a, kb, b in pairs if ka == kb == LM]
    assert cc and cl and ll
    assert any(ka == CAM and kb == LM for ka, _, kb, _ in pairs) and any(ka == LM and kb == CAM for ka, _, kb, _ in pairs)  # `tr` of pair_cl
    # both branches of pair_cl (:717) and the camera's own observation; a camera the landmark sees and one it does not
    assert any((cams_of(l) < c).any() for c, l in cl) and any((cams_of(l) > c).any() for c, l in cl)
    assert any(c in cams_of(l) for c, l in cl) and any(c not in cams_of(l) for c, l in cl)
    # l == m, l < m (canonical), l > m (`tr`); a == b, a > b (canonical), a < b (`tr`)
    assert any(l == m for l, m in ll) and any(l < m for l, m in ll) and any(l > m for l, m in ll)
    assert any(a == b for a, b in cc) and any(a > b for a, b in cc) and any(a < b for a, b in cc)
    if name in ("small", "tracks"):
        # a camera across a 64-edge on either side of a camera pair, as the camera of a mixed pair, in the tracks of both sides
        assert any(a in strad and b not in strad for a, b in cc) and any(a not in strad and b in strad for a, b in cc)
        assert any(c in strad for c, _ in cl) and any(set(cams_of(l).tolist()) & strad for _, l in cl)
        assert any(set(cams_of(l).tolist()) & strad for l, _ in ll) and any(set(cams_of(m).tolist()) & strad for _, m in ll)
        # blocks of C on one, two and four tiles
        assert {span(a) * span(b) for a, b in cc} == {1, 2, 4}
        assert {1, 2, 4} <= {span(c) * span(int(cj)) for c, l in cl for cj in cams_of(l)}
    if name == "tracks":
        for side in (0, 1):  # track lengths on both sides of 16 and of the staging chunk, on the l side and on the m side
            ks = {int(k[pr[side]]) for pr in ll}
            assert {15, 16, 17, chunk - 1, chunk, chunk + 1} <= ks, ks
        assert {15, 16, 17, chunk - 1, chunk, chunk + 1} <= {int(k[l]) for _, l in cl}
    if name == "long" or (name == "tracks" and step == 2):
        assert any(l != m and k[l] > chunk and k[m] > chunk for l, m in ll)  # both chunk loops repeat on a rectangle
        assert any(l == m and k[l] > chunk for l, m in ll)
    if name == "small":
        assert len(cc) >= 36 and len(cl) >= 480 and len(ll) >= 1600 and len(set(pairs)) < len(pairs)  # every pair, duplicates


@pytest.mark.parametrize("name,step,robust,lam", PB.PAIR_CASES, ids=[_id(c) for c in PB.PAIR_CASES])
def test_both_emulation_orders_stay_inside_every_pair_bound(name, step, robust, lam):
    sy = CB.system(name, step, robust, lam)
    pairs = PB.case_pairs(name, sy.p, step)
    _assert_request_reaches_the_edges(name, step, sy, pairs)
    for order in (0, 1):
        d = CB.emulated(name, step, robust, lam, order)
        Cs = CB.c_symmetric(d["inv"], d["panel"])
        ref = PB.pair_reference(sy, Cs, d["Q"], pairs)
        for coords in (1, 0):
            blocks = _run(sy, d, order, pairs, coords)
            out = PB.pair_check(sy, Cs, d["Q"], pairs, blocks, coords, ref=ref)
            bad = out.pop("exact")
            total = int(PB.layout(pairs, sy.dim, coords)[1][-1])
            assert all(v[0].shape == (total,) for v in out.values())  # none skipped (and `covered` inside pair_check)
            PB.report(f"{name} step {step} {robust} lambda {lam:g} order {order} coords {coords} pairs", out, bad)
            if lam > 0 and coords == 1:  # damped: pair_cc's bound is zero, the blocks are C's entries bit for bit
                assert not np.any(out["pair_cc"][1]) and not np.any(out["pair_cc"][0])
                for (ka, a, kb, b), blk in zip(pairs, blocks):
                    if ka == kb == CAM:
                        assert np.array_equal(blk, Cs[sy.dim * a:sy.dim * a + sy.dim, sy.dim * b:sy.dim * b + sy.dim])


def mutation_request(name, sy, step):
    """A request small enough to be emulated once per defect: small: all 36 camera pairs and a seeded 150 of each other kind
    (the mixed ones in both orders) with every landmark's own pair among them; tracks: the tracks of 2, 17, 33, 64, 65 with
    each other and with cameras 0, 5, 65, the camera pairs of the case."""
    p = sy.p
    if name == "tracks":
        ls = (0, 1, 6, 8, 9)
        ll = [(LM, l, LM, m) for l in ls for m in ls]
        cl = [(CAM, c, LM, l) for c in PB.TRACK_CAMS for l in ls]
        cc = [(CAM, a, CAM, b) for a in PB.TRACK_CC for b in PB.TRACK_CC]
        return ll + cl + [(kb, b, ka, a) for ka, a, kb, b in cl] + cc
    cc = P.all_pairs(p.n_cams, 0)[0]
    _, cl, ll = P.sample_pairs(np.random.default_rng(5 + step), p.n_cams, p.n_lms, 150)
    return cc + cl + ll + [(LM, l, LM, l) for l in range(0, p.n_lms, 4)] + [(CAM, 5, LM, 0), (LM, 0, CAM, 5), (LM, 3, LM, 7), (LM, 7, LM, 3)]


MUT_CASES = [("small", 1, "NONE", 0.0), ("small", 2, "NONE", 0.0), ("small", 1, "NONE", 1e-4), ("tracks", 1, "NONE", 0.0),
             ("tracks", 2, "NONE", 0.0)]
WANT = {"cl_branch_transposed", "cl_no_merge", "cl_t_sign", "cl_tr_ignored", "ll_m_head", "ll_oj_stale", "ll_tl_every_jc",
        "ll_tm_every_ic", "ll_skip_last_pp", "ll_hi_offdiag", "ll_no_hi", "ll_tr_ignored", "cc_q_rows", "cc_sigma_a_for_b",
        "cc_n_a_for_b", "cc_no_same_swap", "t_group_skipped", "c_tile_1e-10"}


def _perturbed(sy, d, tile):
    """(inv, panel) of cov_lauum with the tile of C perturbed by 1e-10 relative (cov_bounds.emulate_lauum's c_tile)."""
    return CB.emulate_lauum(CB.upper(d["inv"]), 0, {"c_tile": tile})


def _tile_entries(sy, tile):
    I, J = tile
    return {(64 * I + r) * sy.N + 64 * J + c for r in range(2) for c in range(32, 48)}


@pytest.mark.parametrize("name,step,robust,lam", MUT_CASES, ids=[_id(c) for c in MUT_CASES])
def test_every_pair_mutation_is_reported_on_the_entries_it_touches(name, step, robust, lam):
    sy, d = CB.system(name, step, robust, lam), CB.emulated(name, step, robust, lam, 0)
    pairs = mutation_request(name, sy, step)
    Cs = CB.c_symmetric(d["inv"], d["panel"])
    ref = PB.pair_reference(sy, Cs, d["Q"], pairs)
    for coords in (1, 0):
        clean = PB.pair_check(sy, Cs, d["Q"], pairs, _run(sy, d, 0, pairs, coords), coords, ref=ref)
        assert not clean["exact"] and not any(PB.flagged(*clean[k]) for k in PB.CHECKS)
    muts = PB.mutations_pairs(sy, d, pairs)
    for mname, mutate, checks, touched in muts:
        assert touched, mname
        if mname == "c_tile_1e-10":  # not these kernels' fault: the pair checks stay clean on the perturbed C, LAUUM reports the tile
            inv2, panel2 = _perturbed(sy, d, mutate["c_tile"])
            assert not np.array_equal(CB.c_symmetric(inv2, panel2), Cs)
            d2 = dict(d, inv=inv2, panel=panel2)
            Cs2 = CB.c_symmetric(inv2, panel2)
            out = PB.pair_check(sy, Cs2, d["Q"], pairs, _run(sy, d2, 0, pairs, 1), 1)
            assert not out["exact"] and not any(PB.flagged(*out[k]) for k in PB.CHECKS), mname
            hit = CB.flagged(*CB.lauum_check(inv2, panel2)["lauum"])
            assert hit and hit <= _tile_entries(sy, mutate["c_tile"]), mname
            print(f"PAIRMUTATION {name} step {step} lambda {lam:g} {mname}: the pair checks are clean on the perturbed C, lauum reports {len(hit)} entries")
            continue
        coords, mut = PB.split_mutation(mutate)
        out = PB.pair_check(sy, Cs, d["Q"], pairs, _run(sy, d, 0, pairs, coords, mut), coords, ref=ref)
        bad = out.pop("exact")
        if "exact" in checks:
            assert bad and all(("symmetric" if mname == "cc_no_same_swap" else "transpose") in m for m in bad), (mname, bad[:3])
        else:
            assert not bad, (mname, bad[:3])
        n_hit = 0
        for k in PB.CHECKS:
            hit = PB.flagged(*out[k])
            if k not in checks:
                assert not hit, f"{mname}: {k} reports {len(hit)} entries"
                continue
            assert hit, f"{mname}: not reported by {k}"
            assert hit <= touched, f"{mname}: {k} reports entries the defect does not touch: {sorted(hit - touched)[:5]}"
            n_hit += len(hit)
        print(f"PAIRMUTATION {name} step {step} lambda {lam:g} {mname}: {'/'.join(checks)} reports {n_hit if n_hit else len(bad)} "
              f"of {len(touched)} touched entries, every other check clean")
    assert {m[0] for m in muts} <= WANT


def test_every_listed_pair_mutation_finds_a_shape():
    """Which shapes have what each defect needs (the cases above assert that every defect a shape lists is reported there)."""
    seen = {}
    for name, step, robust, lam in MUT_CASES:
        sy, d = CB.system(name, step, robust, lam), CB.emulated(name, step, robust, lam, 0)
        for m in PB.mutations_pairs(sy, d, mutation_request(name, sy, step)):
            seen.setdefault(m[0], []).append(_id((name, step, robust, lam)))
    print(f"PAIRMUTATION shapes per mutation: {seen}")
    assert WANT <= set(seen), sorted(WANT - set(seen))


def test_the_normwise_pair_bound_accepts_what_the_pair_checks_reject():
    """small, step 1, free gauge: the blocks of every mutated emulation under the bound of tests/test_gpu_pair_covariance.py
    (|got - want|_F <= PairReference.bound x scale per block, against the long-double blocks through the full matrix K), and
    pair_check on the same blocks."""
    name, step, robust, lam = "small", 1, "NONE", 0.0
    sy, d = CB.system(name, step, robust, lam), CB.emulated(name, step, robust, lam, 0)
    old = P.reference(name, step, robust, lam, True)
    pairs = mutation_request(name, sy, step)
    Cs = CB.c_symmetric(d["inv"], d["panel"])
    ref = PB.pair_reference(sy, Cs, d["Q"], pairs)

    def normwise(blocks, coords):
        r = [float(np.linalg.norm((b.astype(np.longdouble) - old.want(pr, coords == 0)).astype(F))) / (old.bound * old.scale(pr, coords == 0))
             for pr, b in zip(pairs, blocks)]
        return max(r)

    assert normwise(_run(sy, d, 0, pairs, 1), 1) <= 1 and normwise(_run(sy, d, 0, pairs, 0), 0) <= 1
    accepted = []
    for mname, mutate, checks, touched in PB.mutations_pairs(sy, d, pairs):
        coords, mut = PB.split_mutation(mutate)
        if mname == "c_tile_1e-10":
            inv2, panel2 = _perturbed(sy, d, mut["c_tile"])
            blocks = _run(sy, dict(d, inv=inv2, panel=panel2), 0, pairs, 1)
        else:
            blocks = _run(sy, d, 0, pairs, coords, mut)
        worst = normwise(blocks, coords)
        out = PB.pair_check(sy, Cs, d["Q"], pairs, blocks, coords, ref=ref)  # (against the clean C)
        bad = out.pop("exact")
        hit = set().union(*(PB.flagged(*out[k]) for k in PB.CHECKS))
        new = max(PB.worst(*out[k])[0] for k in PB.CHECKS)
        print(f"PAIRGAP {mname}: normwise bound {'accepts' if worst <= 1 else 'rejects'} ({worst:.3g} of the bound); pair_check "
              f"{'rejects' if (hit or bad) else 'accepts'}, worst err / bound {new:.3g}, {len(hit)} entries{', exact facts' if bad else ''}")
        assert hit or bad, mname
        if worst <= 1:
            accepted.append(mname)
        if mname == "c_tile_1e-10":
            # reported: only entries that read the tile; every camera-camera entry that reads it (its bound is one rounding of
            # C), and entries of both other kinds -- not all of them: where the two perturbed rows of C carry less than the
            # operand errors of W charged on the whole sum, 1e-10 of them is inside the bound
            assert not bad and hit <= touched, sorted(hit - touched)[:8]
            cc_t = {i for i in touched if out["pair_cc"][1][i] > 0}
            assert cc_t and PB.flagged(*out["pair_cc"]) == cc_t
            assert PB.flagged(*out["pair_cl"]) and PB.flagged(*out["pair_ll"])
            print(f"PAIRGAP c_tile_1e-10: reported {len(hit)} of the {len(touched)} entries that read the tile "
                  f"(pair_cc {len(cc_t)} of {len(cc_t)}, pair_cl {len(PB.flagged(*out['pair_cl']))}, pair_ll {len(PB.flagged(*out['pair_ll']))}), no other entry")
    print(f"PAIRGAP accepted by the normwise bound: {accepted}")
    assert "c_tile_1e-10" in accepted, accepted
    # the new bound over the normwise one, per block (Frobenius norm of the entrywise bound), information only
    ratio = {k: [] for k in PB.CHECKS}
    for t, pr in enumerate(pairs):
        ratio[PB._kind(pr)].append(float(np.linalg.norm(np.asarray(ref[t][1], dtype=F))) / old.bound)
    print("PAIRGAIN small step 1 free gauge, new bound / normwise bound per block, median (largest): " +
          ", ".join(f"{k} {np.median(v):.3g} ({max(v):.3g})" for k, v in ratio.items()))
