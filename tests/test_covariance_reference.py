"""The facts the camera covariance (povar_camera_covariance_pose / _joint) rests on, checked on the CPU oracle's dense S:
the undamped reduced systems have exactly the gauge null space (12 affine / 15 projective dimensions) on the regular
problems and more on medium_problem, the analytic bases of tests/covariance_reference.py span it, and
S0^+ = (S0 + Q Q^T)^-1 - Q Q^T.  Plus the public surface: header, binding, constants."""
import os
import re

import numpy as np
import pytest

import covariance_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _system(name, step):
    p = R.problem(name)
    if step == 1:
        S0, sigma, cams, _, _ = R.system_pose(p, 0.0)
        return S0, R.gauge_basis_pose(cams, sigma), sigma, cams
    S0, sigma, cams, _, _, _ = R.system_joint(p, 0.0)
    return S0, R.gauge_basis_joint(cams, sigma), sigma, cams


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("name", ["small", "p22", "p24", "medium"])
def test_gauge_null_space_and_pseudo_inverse(name, step):
    S0, V, sigma, cams = _system(name, step)
    assert np.all(np.isfinite(S0))
    nq = 12 if step == 1 else 15
    assert V.shape == (S0.shape[0], nq) and np.linalg.matrix_rank(V) == nq
    # the analytic basis is in the null space ...
    assert np.all(np.linalg.norm(S0 @ V, axis=0) <= 1e-12 * np.linalg.norm(V, axis=0))
    null_dim, ev = R.null_dimension(S0)
    if name in R.REGULAR:
        # ... and is all of it: the next eigenvalue is far away
        assert null_dim == nq and ev[nq] >= 1.1e-2
        Q = R.orthonormal(V)
        pinv = np.linalg.pinv(S0, rcond=1e-10, hermitian=True)
        ident = np.linalg.inv(S0 + Q @ Q.T) - Q @ Q.T
        assert np.linalg.norm(ident - pinv) <= 1e-12 * np.linalg.norm(pinv)
        # the scale 1 of Q Q^T suits the Jacobi-scaled system: a well conditioned inverse
        assert 1.0 < ev[-1] < 4.0 and np.linalg.cond(S0 + Q @ Q.T) <= 4.0 / 1.1e-2
    else:
        assert null_dim == (21 if step == 1 else 30)


def test_generators_with_a_last_row_are_not_gauge_in_step_1():
    S0, V, sigma, cams = _system("small", 1)
    gens = []
    for j in range(4):
        G = np.zeros((4, 4))
        G[3, j] = 1.0
        gens.append(G)
    X = R.gauge_basis_pose(cams, sigma, gens)
    assert np.all(np.linalg.norm(S0 @ X, axis=0) > 0.1 * np.linalg.norm(X, axis=0))


def test_longdouble_inverse_and_coordinate_maps():
    rng = np.random.default_rng(0)
    B = rng.normal(size=(40, 40))
    A = B @ B.T + 40 * np.eye(40)
    C = R.chol_inverse_longdouble(A)
    assert np.abs(C @ A.astype(np.longdouble) - np.eye(40)).max() < 1e-15
    assert np.array_equal(C, C.T) or np.abs(C - C.T).max() < 1e-19
    # step 2's map has rank 11 and annihilates h0 / sigma
    cams = rng.normal(size=(3, 12))
    sigma = 0.5 + rng.random((3, 12))
    T = rng.normal(size=(3, 11, 11))
    T = T @ T.transpose(0, 2, 1)
    K = R.to_camera_coords(T, sigma, 2, cams)
    w, beta = R.householder(cams)
    h0 = R.reflectors(w, beta)[:, :, 0]
    assert np.abs(np.einsum("cij,cj->ci", K, h0 / sigma)).max() < 1e-12 * np.abs(K).max()
    assert all(np.linalg.matrix_rank(K[c], tol=1e-10 * np.abs(K[c]).max()) == 11 for c in range(3))
    K1 = R.to_camera_coords(T[:, :, :], sigma[:, 1:], 1)
    assert np.allclose(K1, sigma[:, 1:, None] * T * sigma[:, None, 1:])


def test_public_surface_declares_the_covariance_calls():
    """Fails without the feature: the header declares both entry points and the enums, the binding has the method and the
    constants (the existing symbol test then covers the export)."""
    text = open(os.path.join(ROOT, "include", "povar_hip.h")).read()
    for name in ("povar_camera_covariance_pose", "povar_camera_covariance_joint"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*povar_ctx\s*\*[^;]*double\s+lambda[^;]*int32_t\s+gauge[^;]*int32_t\s+coords[^;]*double\s*\*\s*cov", text), name
    assert re.search(r"POVAR_COV_FREE_GAUGE\s*=\s*0\s*,\s*POVAR_COV_DAMPED\s*=\s*1", text)
    assert re.search(r"POVAR_COV_CAMERA_COORDS\s*=\s*0\s*,\s*POVAR_COV_SOLVER_COORDS\s*=\s*1", text)
    from povar_amd import capi
    assert (capi.COV_FREE_GAUGE, capi.COV_DAMPED, capi.COV_CAMERA_COORDS, capi.COV_SOLVER_COORDS) == (0, 1, 0, 1)
    assert callable(getattr(capi.Context, "camera_covariance"))
