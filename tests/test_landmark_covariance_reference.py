"""The mathematics behind povar_landmark_covariance_pose / _joint, on the CPU (tests/landmark_covariance_reference.py), and
the declarations of the two calls.

* free gauge: the Schur formula with S0^+ gives the landmark blocks of the covariance with the gauge fixed on the cameras
  (the top-left part of [[H0, Cg], [Cg^T, 0]]^-1, Cg = [Q; 0]) -- and not the blocks of pinv(H0), which the header says too;
* damped: the formula gives the blocks of the inverse of the full damped matrix;
* step 2, landmark coordinates: rank 3, null vector X_l / s_l, independent of the tangent bases;
* every case of the GPU test keeps its bound under 1e-4 of the smallest block, so the GPU test means something.
"""
import fnmatch
import os
import re

import numpy as np
import pytest

import landmark_covariance_reference as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel_blocks(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b, axis=(1, 2)) / np.linalg.norm(b, axis=(1, 2))


@pytest.mark.parametrize("name", ["small", "p22", "p24"])
@pytest.mark.parametrize("step", [1, 2])
def test_free_gauge_is_the_camera_fixed_gauge(step, name):
    s = L.system(name, step)
    got = L.reference(name, step, "NONE", 0.0, True).blocks
    H0, Cg = s.full(0.0), s.gauge_border()
    assert np.abs(s.reduced(0.0).astype(np.float64) @ s.Q).max() < 1e-10  # Q spans null(S0)
    m, nq = H0.shape[0], Cg.shape[1]
    B = np.zeros((m + nq, m + nq))
    B[:m, :m], B[:m, m:], B[m:, :m] = H0, Cg, Cg.T
    want = L.landmark_blocks(np.linalg.inv(B)[:m, :m], s.n, s.n_lms)
    err = _rel_blocks(got, want)
    print(f"step {step} {name}: Schur formula with S0^+ vs bordered system, worst block {err.max():.2e}")
    assert err.max() <= 1e-10
    # ... and it is not the minimum-norm covariance over cameras and landmarks together
    ev, V = np.linalg.eigh(H0)
    assert ev[nq - 1] < 1e-10 * ev[-1] < ev[nq]
    pinv = (V[:, nq:] / ev[nq:]) @ V[:, nq:].T
    diff = _rel_blocks(got, L.landmark_blocks(pinv, s.n, s.n_lms))
    print(f"step {step} {name}: against the blocks of pinv(H0): worst {diff.max():.2f}")
    assert diff.max() > 1e-2


@pytest.mark.parametrize("lam", [1e-4, 1.0])
@pytest.mark.parametrize("name", ["small", "p22", "p24"])
@pytest.mark.parametrize("step", [1, 2])
def test_damped_is_the_block_of_the_full_inverse(step, name, lam):
    s = L.system(name, step)
    got = s.sigma_blocks(lam, False)
    want = L.landmark_blocks(np.linalg.inv(s.full(lam)), s.n, s.n_lms)
    err = _rel_blocks(got, want)
    print(f"step {step} {name} lambda {lam:g}: worst block {err.max():.2e}")
    assert err.max() <= 1e-10


@pytest.mark.parametrize("free_gauge,lam", [(True, 0.0), (False, 1e-4)])
def test_step2_landmark_coordinates(free_gauge, lam):
    p = L.problem("small")
    s = L.system("small", 2)
    got = s.to_landmark_coords(s.sigma_blocks(lam, free_gauge)).astype(np.float64)
    assert got.shape == (s.n_lms, 4, 4)
    ev = np.linalg.eigvalsh(got)
    assert np.all(np.abs(ev[:, 0]) <= 1e-12 * ev[:, -1]) and np.all(ev[:, 1] > 1e-9 * ev[:, -1])  # rank 3
    x = s.lms / s.s
    resid = np.einsum("lij,lj->li", got, x)
    assert np.all(np.linalg.norm(resid, axis=1) <= 1e-12 * np.linalg.norm(got, axis=(1, 2)) * np.linalg.norm(x, axis=1))
    other = L.System(p, 2, basis="scipy")
    again = other.to_landmark_coords(other.sigma_blocks(lam, free_gauge)).astype(np.float64)
    err = np.linalg.norm(again - got, axis=(1, 2)) / np.linalg.norm(got, axis=(1, 2))
    print(f"free gauge {free_gauge}: Householder against scipy null-space bases, worst block {err.max():.2e}")
    assert err.max() <= 1e-9


def test_step1_landmark_coordinates_follow_the_column_scale():
    """D Sigma D with the Jl column scale on equals the unscaled system's Sigma (damping aside: free gauge, lambda_l = 0)."""
    p = L.problem("small")
    plain, scaled = L.System(p, 1, jl_scaling=False), L.system("small", 1)
    assert np.all(plain.s == 1.0) and scaled.s.min() < 1.0
    a = plain.to_landmark_coords(plain.sigma_blocks(0.0, True))
    b = scaled.to_landmark_coords(scaled.sigma_blocks(0.0, True))
    assert _rel_blocks(b, a).max() <= 1e-10


@pytest.mark.parametrize("step,name,norm,lam,free_gauge", L.GPU_CASES)
def test_bound_condition(step, name, norm, lam, free_gauge):
    """The GPU test's bound is at most 1e-4 of every block's norm."""
    ref = L.reference(name, step, norm, lam, free_gauge)
    norms = np.linalg.norm(ref.blocks.astype(np.float64), axis=(1, 2))
    print(f"step {step} {name} {norm} lambda {lam:g}: m {ref.m} cond {ref.cond:.3g} |K^-1| {ref.inv_norm:.3g} "
          f"bound / min |Sigma_l|_F = {ref.bound / norms.min():.2e}")
    assert np.all(ref.bound <= 1e-4 * norms)


def test_long_track_problem_has_the_tracks_the_gpu_test_needs():
    track = np.diff(L.problem("long").lm_off)
    assert np.sum(track >= 65) == 2 and np.sum((track >= 33) & (track <= 64)) == 3


def test_header_and_export_map_declare_the_calls():
    header = open(os.path.join(ROOT, "include", "povar_hip.h")).read()
    vmap = open(os.path.join(ROOT, "povar_amd", "csrc", "povar.map")).read()
    exported = re.search(r"global:([^}]*?)local:", vmap).group(1).replace(";", " ").split()
    for name in ("povar_landmark_covariance_pose", "povar_landmark_covariance_joint"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*povar_ctx\s*\*", header), name
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), name
    assert re.search(r"POVAR_COV_LANDMARK_COORDS\s*=\s*0", header)
    assert "gauge fixed on the cameras: minimum norm over the camera parameters" in " ".join(header.replace("*", " ").split())
