"""CPU checks for fixed cameras (povar_set_fixed_cameras): the reference of tests/fixed_cameras_reference.py against itself,
the declarations of the C ABI and its binding, and the parsing of `bal --fixed-cameras`.  No GPU involved.

The restriction argument ("Fixed cameras"): with the blocks of B^-1 zeroed on the fixed set F every
term of the power series is zero on F, and on the free cameras it is the term of the series of S_ff = B_ff - E0_ff; the
same holds for PCG with the Schur-Jacobi inverse blocks zeroed on F.
"""
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

import covariance_reference as R
import fixed_cameras_reference as FR
from conftest import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM, M = 1e-4, 20
CASES = [("small", (1, 4)), ("small", (0, 1)), ("small", (2, 3, 5)), ("p22", (2, 3, 5)), ("p22", (0, 1))]


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("name,F", CASES)
def test_masked_series_is_the_restricted_series(name, F, step):
    """Oracle series with zero blocks of B^-1 on F == the series written out on S_ff's matrices: <= 1e-13 relative per term
    and for the sum (both are fp64 sums of the same products, in different orders: a few u times the number of terms and
    the row length; measured 8.5e-15 on small at 20 terms), and exactly zero on F."""
    p = R.problem(name)
    acc, terms, s = FR.masked_series(p, step, LAM, F, M)
    if step == 1:
        orc, st, hll, b, binv = s[:5]
        dim, E0 = 12, FR.dense_e0(lambda x: orc.right_mul_e0_pose(st, hll, x), 12 * p.n_cams)
    else:
        orc, st_h, st_n, hll, b, binv = s[:6]
        dim, E0 = 11, FR.dense_e0(lambda x: orc.right_mul_e0_joint(st_n, hll, x), 11 * p.n_cams)
    want, want_terms = FR.restricted_series(binv, E0, b, dim, F, M)
    k = FR.fixed_coords(p.n_cams, dim, F)
    assert np.all(acc[k] == 0.0) and np.all(terms[:, k] == 0.0)
    worst = max(rel(terms[i], want_terms[i]) for i in range(M + 1))
    print(f"step {step} {name} F {F}: sum {rel(acc, want):.3e}, worst term {worst:.3e}")
    assert rel(acc, want) <= 1e-13 and worst <= 1e-13
    # and the series is on its way to the restricted solve (the last term is small against the sum)
    S = np.zeros((dim * p.n_cams,) * 2)
    for c in range(p.n_cams):
        S[dim * c:dim * c + dim, dim * c:dim * c + dim] = np.linalg.inv(binv[c].reshape(dim, dim))
    S -= E0
    exact = FR.pad(np.linalg.solve(FR.restricted(S, dim, F), -b[FR.free_coords(p.n_cams, dim, F)]), p.n_cams, dim, F)
    assert rel(acc, exact) < rel(terms[0], exact)


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("name,F", CASES)
def test_masked_pcg_reaches_the_restricted_solve(name, F, step):
    """Oracle PCG with the Schur-Jacobi inverse blocks zeroed on F: the iterate is exactly zero on F and converges to
    S_ff^-1 (-b_f).  eta = 1e-12 bounds the relative change of the quadratic model, the squared energy norm of the error, so
    the iterate is within sqrt(eta) in the energy norm of S_ff and within sqrt(eta cond_2(S_ff)) in the 2-norm (measured 8e-8
    on small after 26 iterations, 9e-7 at worst; the bound is 2e-5 to 4e-5)."""
    from oracle import povar_oracle as O
    p = R.problem(name)
    sys_ = R.system_pose(p, LAM) if step == 1 else R.system_joint(p, LAM)
    S, b = sys_[0], sys_[-1]
    dim = 12 if step == 1 else 11
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    minv = FR.masked(orc.block_jacobi_inverse(S, dim), F)
    x, it, status = orc.pcg(S, b, minv, dim=dim, eta=1e-12, max_iterations=500)
    exact = FR.pad(np.linalg.solve(FR.restricted(S, dim, F), -b[FR.free_coords(p.n_cams, dim, F)]), p.n_cams, dim, F)
    ev = np.linalg.eigvalsh(FR.restricted(S, dim, F))
    bound = float(np.sqrt(1e-12 * ev[-1] / ev[0]))
    print(f"step {step} {name} F {F}: {it} iterations, status {status}, rel {rel(x, exact):.3e}, bound {bound:.3e}")
    assert status == 1 and 0 < it < 500
    assert np.all(x[FR.fixed_coords(p.n_cams, dim, F)] == 0.0)
    assert rel(x, exact) <= bound


def test_one_fixed_camera_does_not_fix_the_gauge():
    """Null dimension of S_ff(0) (covariance_reference.null_dimension): 4 with one fixed camera -- in step 1 at the pOSE start
    state of synth.make_problem (third camera row (0, 0, 0, 1)) for every choice of the camera, in step 2 at the generic
    state --, 0 with {0, 1} and {2, 3, 5}."""
    for name in ("small", "p22"):
        p = R.problem(name)
        S1, S2 = R.system_pose(p, 0.0)[0], R.system_joint(p, 0.0)[0]
        assert np.all(np.asarray(p.cams).reshape(-1, 12)[:, 8:] == [0, 0, 0, 1])
        for c in (range(p.n_cams) if name == "small" else (0,)):
            for S, dim in ((S1, 12), (S2, 11)):
                nd, ev = R.null_dimension(FR.restricted(S, dim, (c,)))
                assert nd == 4, (name, c, dim, ev[:6])
        for F in ((0, 1), (2, 3, 5)):
            for S, dim in ((S1, 12), (S2, 11)):
                nd, ev = R.null_dimension(FR.restricted(S, dim, F))
                print(f"{name} dim {dim} F {F}: eigenvalues {ev[0]:.3g} .. {ev[-1]:.3g}")
                assert nd == 0 and ev[0] > 0, (name, F, dim, ev[:3])


def test_decoupled_system_solves_the_restricted_one():
    """The matrix CHOLESKY factors (identity rows and columns on F, right-hand side 0): its solve is the zero-padded restricted
    solve, its inverse less the identity on F the zero-padded [S_ff]^-1."""
    p = R.problem("small")
    S, b = R.system_pose(p, LAM)[0], R.system_pose(p, LAM)[-1]
    F = FR.SETS["small"]
    A, rhs = FR.decoupled(S, -b, 12, F)
    x = np.linalg.solve(A, rhs)
    k, f = FR.fixed_coords(p.n_cams, 12, F), FR.free_coords(p.n_cams, 12, F)
    assert np.all(x[k] == 0.0)
    assert rel(x[f], np.linalg.solve(FR.restricted(S, 12, F), -b[f])) <= 1e-12
    C, cond, inv_norm = FR.covariance(S, 12, F)
    Ai = np.linalg.inv(A)
    Ai[k, k] -= 1.0
    assert np.all(C[k] == 0) and np.all(C[:, k] == 0)
    assert np.abs(Ai - C.astype(np.float64)).max() <= 72 * R.U * cond * inv_norm


def test_abi_declares_and_binding_mirrors_the_calls():
    from povar_amd import capi
    hdr = open(capi.HEADER).read()
    assert re.search(r"int\s+povar_set_fixed_cameras\(povar_ctx\*\s*\w*,\s*const int32_t\*\s*cam_ids,\s*int32_t\s+n_ids\)", hdr)
    assert re.search(r"int\s+povar_fixed_cameras\(povar_ctx\*\s*\w*,\s*int32_t\*\s*flags", hdr)
    m = re.search(r"enum\s*\{\s*POVAR_COV_FREE_GAUGE\s*=\s*0\s*,\s*POVAR_COV_DAMPED\s*=\s*1\s*,\s*POVAR_COV_FIXED_GAUGE\s*=\s*2\s*\}", hdr)
    assert m, "POVAR_COV_FIXED_GAUGE = 2 appended to the gauge enum"
    assert (capi.COV_FREE_GAUGE, capi.COV_DAMPED, capi.COV_FIXED_GAUGE) == (0, 1, 2)
    assert callable(capi.Context.set_fixed_cameras) and callable(capi.Context.fixed_cameras)
    # no new buffer id, no new layout field
    assert capi.BUF_COV_GAUGE == 17 and capi.LayoutInfo._fields_[-1][0] == "fp32_terms"
    # the version script exports them
    vs = open(os.path.join(ROOT, "povar_amd", "csrc", "povar.map")).read()
    glob = re.search(r"global:\s*([^;]+);", vs).group(1).split()
    for name in ("povar_set_fixed_cameras", "povar_fixed_cameras"):
        assert any(fnmatch.fnmatch(name, g) for g in glob), name
    if os.path.exists(capi.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
        assert " T povar_set_fixed_cameras" in out and " T povar_fixed_cameras" in out


@pytest.fixture(scope="module")
def binaries():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povar_amd", "csrc"), "host"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "bin", "bal"), os.path.join(ROOT, "build", "bal_oracle")


def test_bal_parses_fixed_cameras(binaries, tmp_path):
    """`bal --fixed-cameras LIST`: ids and a-b ranges; a bad token fails at the command line, an id >= the camera count once the
    problem is loaded, both before any device work; a good list is announced on stdout (what follows needs the device).
    The oracle-backed twin does not implement fixed cameras and says so instead of ignoring the option."""
    from povar_amd import synth
    bal, bal_oracle = binaries
    p = synth.make_problem(8, 150, 640, seed=5)
    f = str(tmp_path / "problem-8-150.txt")
    synth.write_data_custom(f, p)
    base = ["--input", f, "--quiet", "--log-disable-all", "--max-num-iterations-step-1", "1", "--max-num-iterations-step-2", "0"]
    assert "--fixed-cameras" in subprocess.run([bal, "--help"], capture_output=True, text=True).stdout
    for bad in ("0,x", "1-", "-1", "3-2", "0,,1", "", "1;2", "0,1,"):
        r = subprocess.run([bal] + base + ["--fixed-cameras", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "fixed-cameras" in r.stderr and "fixed cameras:" not in r.stdout, bad
    for out_of_range in ("0,8", "6-9"):
        r = subprocess.run([bal] + base + ["--fixed-cameras", out_of_range], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "out of range" in r.stderr and "fixed cameras:" not in r.stdout, out_of_range
    for good, k in (("0,1", 2), ("0,2-4,2", 4), ("7", 1), ("0-7", 8), ("--fixed-cameras=1,5", 2)):
        args = [good] if good.startswith("--") else ["--fixed-cameras", good]
        r = subprocess.run([bal] + base + args, capture_output=True, text=True, timeout=120)
        assert f"fixed cameras: {k} of 8\n" in r.stdout, (good, r.stdout[-500:], r.stderr[-500:])
    r = subprocess.run([bal_oracle] + base + ["--fixed-cameras", "0,1"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "does not implement fixed cameras" in r.stderr
    r = subprocess.run([bal_oracle] + base, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
