"""What a covariance call decides before it touches the device (povar_amd/csrc/cov_plan.hpp), checked without the library or a device
by tests/cpp/cov_plan_check.cpp: (A) the rules of gauge, coords, lambda and the fixed set over all 120 combinations, with the first
failing rule where two fail; (B) the landmark request (ids to n_out, row0, rows; the 2^31 cap); (C) the pair request (three lists
in canonical order, tr, every offset, total, every refusal) -- all against tables written down in the checker -- and here (D) the
gauge basis against tests/covariance_reference.py on its "small" problem (6 cameras), both steps.

D's two tolerances are measured on the reference, not on the function under test: the generators V of gauge_basis_pose / _joint
are orthonormalised once in float64 (R.orthonormal: Householder QR) and once in np.longdouble (twice-applied modified Gram-Schmidt,
below: numpy's QR takes no long double), and the float64 run's worst entry of
    span  max |(I - Q_ld Q_ld^T) Q_64|        and        null  max |S0 Q_64| / |S0|_inf
is taken, S0 the reference's undamped system.  The function under test sums in another order and applies modified Gram-Schmidt
twice instead of QR, so its error differs by a small factor, not by an order of magnitude: 16 x the measured value is allowed for
    max |(I - Q_ref Q_ref^T) Q|  (Q_ref = R.orthonormal(V) in float64)      and      max |S0 Q| / |S0|_inf.
Measured (x86-64 long double, NumPy's LAPACK); the bounds are formed from the reference at run time, these are their values:
    step 1: span 1.42e-16 -> bound 2.28e-15 (the function: 4.00e-16);  null 1.25e-16 -> bound 1.99e-15 (the function: 1.19e-16)
    step 2: span 2.11e-16 -> bound 3.38e-15 (the function: 4.54e-16);  null 4.21e-17 -> bound 6.73e-16 (the function: 4.53e-17)
Q^T Q = I is held to the bound of tests/cov_bounds.py (GAUGE): g(n + 2 nq + 4), n = dim * 6."""
import os
import subprocess

import numpy as np
import pytest

import covariance_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "cov_plan_check")


@pytest.fixture(scope="module")
def checker():
    # (always through make: the rule lists the header, so an edited plan rebuilds the checker)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "../../build/cov_plan_check"], stdout=subprocess.DEVNULL)
    return BIN


def test_mode_rules_and_requests(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cov_plan_check: ok" in r.stdout


def _gauge_basis(checker, path, dim, P, sigma, w, beta):
    """gauge_basis of cov_plan.hpp on (P, sigma, reflectors) through a text file: Q [dim * n_cams, nq], or None: dependent."""
    n_cams = len(P)
    with open(path, "w") as f:
        f.write(f"{dim} {n_cams}\n")
        for a in (P, sigma, np.concatenate([w, beta[:, None]], axis=1)):
            f.write(" ".join(repr(float(x)) for x in np.asarray(a, dtype=np.float64).ravel()) + "\n")
    r = subprocess.run([checker, "gauge", str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    if lines[0] == "dependent":
        return None
    nq = int(lines[0].split()[1])
    Q = np.array([[float(x) for x in ln.split()] for ln in lines[1:]])
    assert Q.shape == (dim * n_cams, nq)
    return Q


def _orthonormal_longdouble(V):
    Q = np.array(V, dtype=np.longdouble)
    for k in range(Q.shape[1]):
        for _ in range(2):
            for j in range(k):
                Q[:, k] -= (Q[:, j] @ Q[:, k]) * Q[:, j]
        Q[:, k] /= np.sqrt(Q[:, k] @ Q[:, k])
    return Q


def _off_span(Q_ref, Q):
    Q_ref, Q = np.asarray(Q_ref, dtype=np.longdouble), np.asarray(Q, dtype=np.longdouble)
    return float(np.abs(Q - Q_ref @ (Q_ref.T @ Q)).max())


def _null(S0, Q):
    S0 = np.asarray(S0, dtype=np.longdouble)
    return float(np.abs(S0 @ np.asarray(Q, dtype=np.longdouble)).max() / np.abs(S0).sum(axis=1).max())


@pytest.mark.parametrize("step", [1, 2])
def test_gauge_basis_spans_the_reference_null_space(checker, tmp_path, step):
    p = R.problem("small")
    if step == 1:
        S0, sigma, cams = R.system_pose(p, 0.0)[:3]
        V, dim, nq = R.gauge_basis_pose(cams, sigma), 12, 12
    else:
        S0, sigma, cams = R.system_joint(p, 0.0)[:3]
        V, dim, nq = R.gauge_basis_joint(cams, sigma), 11, 15
    w, beta = R.householder(cams)
    Q = _gauge_basis(checker, tmp_path / "gauge.txt", dim, cams, sigma, w, beta)
    assert Q is not None and Q.shape == (dim * p.n_cams, nq)
    n = dim * p.n_cams

    Q_ref, Q_ld = R.orthonormal(V), _orthonormal_longdouble(V)
    span_ref, null_ref = _off_span(Q_ld, Q_ref), _null(S0, Q_ref)
    span, null = _off_span(Q_ref, Q), _null(S0, Q)
    gram = float(np.abs(Q.T.astype(np.longdouble) @ Q.astype(np.longdouble) - np.eye(nq)).max())
    k = n + 2 * nq + 4
    gram_bound = k * R.U / (1 - k * R.U)
    print(f"step {step}: span: reference {span_ref:.2e} -> bound {16 * span_ref:.2e}, the function {span:.2e};  "
          f"null: reference {null_ref:.2e} -> bound {16 * null_ref:.2e}, the function {null:.2e};  |Q^T Q - I| {gram:.2e} <= {gram_bound:.2e}")
    assert gram <= gram_bound
    assert span <= 16 * span_ref
    assert null <= 16 * null_ref


def test_gauge_basis_refuses_dependent_columns(checker, tmp_path):
    """The three generators of one column gj of G are the three columns of every camera's left 3 x 3 block, placed on the entries
    (r, gj).  The cameras of the "small" problem are affine (last row 0 0 0 1): row 2 of that block is zero, so ONE camera gives
    three vectors in two dimensions -- dependent in exact arithmetic -- while two cameras give three in four: independent (two
    cameras are therefore not the dependent input; the function returns a basis for them, asserted here)."""
    cams = R.problem("small").cams.reshape(-1, 12)[:2].copy()
    assert np.all(cams[:, 8:11] == 0)
    sigma, (w, beta) = np.ones_like(cams), R.householder(cams)
    assert _gauge_basis(checker, tmp_path / "two.txt", 12, cams, sigma, w, beta) is not None
    assert _gauge_basis(checker, tmp_path / "one.txt", 12, cams[:1], sigma[:1], w[:1], beta[:1]) is None
