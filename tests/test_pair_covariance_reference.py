"""The mathematics behind povar_covariance_blocks_pose / _joint, on the CPU (tests/pair_covariance_reference.py), and the
declarations of the two calls.

* damped: the three formulas give the blocks of the inverse of the full damped matrix;
* free gauge: they give the blocks of K^-1 - n n^T, K = H0 + Cg Cg^T, Cg = [Q; 0], n = [Q; -F^T Q]: the covariance with the
  gauge fixed on the cameras, which is also the top-left part of [[H0, Cg], [Cg^T, 0]]^-1;
* parameter coordinates: the maps agree with those of the camera and the landmark references on the diagonal blocks;
* every case of the GPU test keeps its bound under 1e-4 of its smallest diagonal block, so the GPU test means something.
"""
import fnmatch
import os
import re

import numpy as np
import pytest

import covariance_reference as R
import landmark_covariance_reference as L
import pair_covariance_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _index(s, kind, i):
    return np.arange(s.dim * i, s.dim * i + s.dim) if kind == P.CAMERA else s.n + np.arange(3 * i, 3 * i + 3)


def _worst(ref, full):
    """Worst |block - full[rows(a), rows(b)]|_F / sqrt(|full_aa|_F |full_bb|_F) over every pair of the three kinds."""
    s = ref.sys
    worst = 0.0
    for pairs in P.all_pairs(s.n_cams, s.n_lms):
        for ka, a, kb, b in pairs:
            ia, ib = _index(s, ka, a), _index(s, kb, b)
            got = ref.block(ka, a, kb, b).astype(np.float64)
            assert got.shape == (ia.size, ib.size)
            unit = np.sqrt(np.linalg.norm(full[np.ix_(ia, ia)]) * np.linalg.norm(full[np.ix_(ib, ib)]))
            worst = max(worst, float(np.linalg.norm(got - full[np.ix_(ia, ib)]) / unit))
    return worst


@pytest.mark.parametrize("lam", [1e-4, 1.0])
@pytest.mark.parametrize("step", [1, 2])
def test_damped_blocks_are_those_of_the_full_inverse(step, lam):
    ref = P.reference("small", step, "NONE", lam, False)
    worst = _worst(ref, np.linalg.inv(ref.sys.full(lam)))
    print(f"step {step} lambda {lam:g}: worst pair against inv(H(lambda)) {worst:.2e}")
    assert worst <= 1e-9


@pytest.mark.parametrize("step", [1, 2])
def test_free_gauge_blocks_are_those_of_the_camera_fixed_gauge(step):
    ref = P.reference("small", step, "NONE", 0.0, True)
    s = ref.sys
    H0, Cg = s.full(0.0), s.gauge_border()
    K = H0 + Cg @ Cg.T
    n_vec = np.zeros_like(Cg)  # n = [Q; -F^T Q]
    n_vec[:s.n] = s.Q
    for l in range(s.n_lms):
        n_vec[s.n + 3 * l:s.n + 3 * l + 3] = -(ref.F[l].astype(np.float64).T @ s.Q[s.rows[l]])
    assert np.abs(H0 @ n_vec).max() <= 1e-9 * np.abs(H0).max()  # n spans the null space of H0
    full = np.linalg.inv(K) - n_vec @ n_vec.T
    worst = _worst(ref, full)
    print(f"step {step}: worst pair against K^-1 - n n^T {worst:.2e}")
    assert worst <= 1e-9
    m, nq = H0.shape[0], Cg.shape[1]
    B = np.zeros((m + nq, m + nq))
    B[:m, :m], B[:m, m:], B[m:, :m] = H0, Cg, Cg.T
    bordered = np.linalg.inv(B)[:m, :m]
    assert np.linalg.norm(bordered - full) <= 1e-9 * np.linalg.norm(full)


@pytest.mark.parametrize("step", [1, 2])
def test_parameter_coordinates_agree_with_the_diagonal_references(step):
    ref = P.reference("small", step, "NONE", 0.0, True)
    s = ref.sys
    cams = R.to_camera_coords(ref.ref.cameras.blocks, s.sigma, step, s.cams)
    lms = ref.ref.want(True)
    for c in range(s.n_cams):
        got = ref.want((P.CAMERA, c, P.CAMERA, c), True)
        assert got.shape == (12, 12)
        assert np.linalg.norm((got - cams[c]).astype(np.float64)) <= 1e-12 * np.linalg.norm(cams[c].astype(np.float64))
    d = 3 if step == 1 else 4
    for l in range(s.n_lms):
        got = ref.want((P.LANDMARK, l, P.LANDMARK, l), True)
        assert got.shape == (d, d)
        assert np.linalg.norm((got - lms[l]).astype(np.float64)) <= 1e-12 * np.linalg.norm(lms[l].astype(np.float64))
    cross = ref.want((P.CAMERA, 1, P.LANDMARK, 2), True)
    assert cross.shape == (12, d)
    assert np.array_equal(ref.want((P.LANDMARK, 2, P.CAMERA, 1), True), cross.T)
    assert ref.scale((P.CAMERA, 1, P.LANDMARK, 2), True) == float(s.sigma.max()) * float(s.s.max())
    assert ref.scale((P.CAMERA, 1, P.LANDMARK, 2), False) == 1.0


@pytest.mark.parametrize("step,name,norm,lam,free_gauge", P.GPU_CASES)
def test_bound_condition(step, name, norm, lam, free_gauge):
    """The GPU test's bound is at most 1e-4 sqrt(|Sigma_aa|_F |Sigma_bb|_F) for every pair: at most 1e-4 of the smallest
    diagonal block of the case."""
    ref = P.reference(name, step, norm, lam, free_gauge)
    smallest = ref.smallest_diagonal_block()
    print(f"step {step} {name} {norm} lambda {lam:g}: m {ref.ref.m} cond {ref.ref.cond:.3g} |K^-1| {ref.ref.inv_norm:.3g} "
          f"bound / min |Sigma_xx|_F = {ref.bound / smallest:.2e}")
    assert ref.bound <= 1e-4 * smallest


def test_tracks_problem_has_the_tracks_the_gpu_test_needs():
    s = L.system("tracks", 1)
    assert s.n_cams == 66 and tuple(int(k) for k in s.track[:10]) == L.TRACK_EDGES


def test_header_and_export_map_declare_the_calls():
    header = open(os.path.join(ROOT, "include", "povar_hip.h")).read()
    vmap = open(os.path.join(ROOT, "povar_amd", "csrc", "povar.map")).read()
    exported = re.search(r"global:([^}]*?)local:", vmap).group(1).replace(";", " ").split()
    for name in ("povar_covariance_blocks_pose", "povar_covariance_blocks_joint"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*povar_ctx\s*\*", header), name
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), name
    assert re.search(r"POVAR_COV_BLOCK_CAMERA\s*=\s*0\s*,\s*POVAR_COV_BLOCK_LANDMARK\s*=\s*1", header)
    text = " ".join(header.replace("*", " ").split())
    assert "a pair of landmarks of two different shards is therefore not served" in text
    from povar_amd import capi
    assert (capi.COV_BLOCK_CAMERA, capi.COV_BLOCK_LANDMARK) == (0, 1)
