"""The host surface of step 2's direct solve, without a GPU: the two new entry points in the header and in the built
library, and `bal --solver-type-step-2 RICHOLESKY` in the option parser (not a value of the reference)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bal():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povar_amd", "csrc"), "host"], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "bin", "bal")


def test_entry_points_declared_and_exported():
    import ctypes
    from povar_amd import capi
    h = open(os.path.join(ROOT, "include", "povar_hip.h")).read()
    assert re.search(r"\bint povar_solve_joint_sc_method\(povar_ctx\* ctx, double lambda, int32_t method,", h)
    assert re.search(r"\bint povar_right_mul_e0_joint\(povar_ctx\* ctx, const double\* x, double\* y\);", h)
    lib = ctypes.CDLL(capi.build())
    for name in ("povar_solve_joint_sc_method", "povar_right_mul_e0_joint", "povar_solve_joint_sc"):
        assert getattr(lib, name) is not None, name
    # null context: an argument error, not a crash
    assert lib.povar_right_mul_e0_joint(None, None, None) < 0
    assert capi.SC_PCG == 0 and capi.SC_CHOLESKY == 1


def test_bal_lists_and_parses_richolesky(bal, tmp_path):
    r = subprocess.run([bal, "--help"], capture_output=True, text=True)
    assert "RICHOLESKY" in r.stdout and "not a value of the reference" in r.stdout
    missing = str(tmp_path / "missing.txt")
    r = subprocess.run([bal, "--input", missing, "--solver-type-step-2", "RICHOLESKY"], capture_output=True, text=True)
    assert r.returncode != 0 and "invalid value" not in r.stdout + r.stderr and "Could not open" in r.stdout + r.stderr
    r = subprocess.run([bal, "--input", missing, "--solver-type-step-2", "NOPE"], capture_output=True, text=True)
    assert r.returncode != 0 and "invalid value 'NOPE'" in r.stdout + r.stderr


def test_richolesky_with_gpus_2_is_refused(bal, tmp_path):
    from povar_amd import synth
    p = synth.make_problem(6, 40, 150, seed=3)
    f = str(tmp_path / "p.txt")
    synth.write_data_custom(f, p)
    r = subprocess.run([bal, "--input", f, "--quiet", "--log-disable-all", "--solver-type-step-2", "RICHOLESKY", "--gpus", "2"],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0
    assert "--gpus > 1 serves the power-series solvers" in r.stderr
