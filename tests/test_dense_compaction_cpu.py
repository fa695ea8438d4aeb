"""The compacted dense system (povar_set_dense_compaction) without a GPU: the ABI and its binding, the conditioning of every
case the GPU tests assert on, the host-only map builder under the sanitizers, and the option of `bal`."""
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

import compaction_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("povar_set_dense_compaction", "povar_dense_compaction", "povar_dense_layout")


def test_abi_and_binding():
    """The three symbols: declared in the header, matched by the version script, exported by the built library, bound in capi."""
    from povar_amd import capi
    hdr = open(os.path.join(ROOT, "include", "povar_hip.h")).read()
    assert re.search(r"int povar_set_dense_compaction\(povar_ctx\* ctx, int32_t mode\);", hdr)
    assert re.search(r"int povar_dense_compaction\(povar_ctx\* ctx\);", hdr)
    assert re.search(r"int povar_dense_layout\(povar_ctx\* ctx, int32_t\* cam_row[^)]*\);", hdr)
    vs = open(os.path.join(ROOT, "povar_amd", "csrc", "povar.map")).read()
    glob = re.search(r"global:\s*([^;]+);", vs).group(1).split()
    for name in SYMBOLS:
        assert any(fnmatch.fnmatch(name, g) for g in glob), name
    assert os.path.exists(capi.LIB_PATH), "the library is built before the tests run"
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert f" T {name}\n" in out, name
    for method in ("set_dense_compaction", "dense_compaction", "dense_layout"):
        assert callable(getattr(capi.Context, method, None)), method
    lib = capi.lib()
    for name in SYMBOLS:
        assert getattr(lib, name)


def test_expected_map_and_rows():
    """The table of the cases: the compact row counts, and the reference map's own shape."""
    for case, (name, F, n1, n2) in CR.CASES.items():
        n_cams = CR.PROBLEMS[name][0]
        for step, dim, want in ((1, 12, n1), (2, 11, n2)):
            n, rows = CR.expected_map(n_cams, dim, F, 1)
            assert n == want == CR.rows_of(case, step), (case, step, n)
            assert np.all(rows[list(F)] == -1) and np.array_equal(rows[rows >= 0], dim * np.arange(n // dim))
            n0, rows0 = CR.expected_map(n_cams, dim, F, 0)
            assert n0 == dim * n_cams and np.array_equal(rows0, dim * np.arange(n_cams))
    # what the cases are for
    assert CR.rows_of("small", 1) < 64 and 256 < CR.rows_of("p24", 1) and CR.rows_of("p24", 2) < 256
    assert min(CR.rows_of("p40", 1), CR.rows_of("p40", 2)) > 256
    free = np.setdiff1d(np.arange(40), CR.fixed_of("p40w"))
    assert (free < 32).any() and (free >= 32).any()  # both column tiles of sc_dense_ordered
    p = CR.synth_problem("p40")
    has_free = np.array([np.isin(p.cam_idx[p.lm_off[l]:p.lm_off[l + 1]], free).any() for l in range(p.n_lms)])
    print(f"p40w: {int((~has_free).sum())} of {p.n_lms} landmarks have no free camera")
    assert (~has_free).sum() == 148


@pytest.mark.parametrize("case", list(CR.CASES))
def test_conditioning(case):
    """S_ff is positive definite with cond_2 <= 1e4 in both steps, undamped and at lambda = 1e-4: no GPU assertion rests on a
    near-singular case."""
    for step in (1, 2):
        for lam in (0.0, CR.LAM):
            lo, hi = CR.conditioning(case, step, lam)
            print(f"{case} step {step} lambda {lam:g}: eigenvalues of S_ff in [{lo:.3e}, {hi:.3e}], cond_2 = {hi / lo:.3e}")
            assert lo > 0 and hi / lo <= 1e4, (case, step, lam, lo, hi)


def test_map_builder_under_sanitizers(tmp_path):
    """tests/cpp/cam_row_map_check.cpp (its own main) with -fsanitize=address,undefined, run directly."""
    exe = str(tmp_path / "cam_row_map_check")
    src = os.path.join(ROOT, "tests", "cpp", "cam_row_map_check.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "cam_row_map: ok" in r.stdout, r.stdout + r.stderr


@pytest.fixture(scope="module")
def binaries():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povar_amd", "csrc"), "host"], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "bin", "bal")


def test_bal_accepts_compact_fixed_cameras(binaries, tmp_path):
    """--compact-fixed-cameras: listed by --help, accepted as a boolean (--x / --no-x), announced with the fixed set and silent
    without one (what follows the announcement needs the device)."""
    from povar_amd import synth
    bal = binaries
    h = subprocess.run([bal, "--help"], capture_output=True, text=True).stdout
    assert "--compact-fixed-cameras" in h and h.count("compact-fixed-cameras") >= 2  # the list of booleans and its own paragraph
    r = subprocess.run([bal, "--input", str(tmp_path / "missing.txt"), "--compact-fixed-cameras"], capture_output=True, text=True)
    assert r.returncode != 0 and "unknown option" not in r.stdout + r.stderr and "Could not open" in r.stdout + r.stderr
    p = synth.make_problem(8, 150, 640, seed=5)
    f = str(tmp_path / "problem-8-150.txt")
    synth.write_data_custom(f, p)
    base = ["--input", f, "--quiet", "--log-disable-all", "--max-num-iterations-step-1", "1", "--max-num-iterations-step-2", "0"]
    r = subprocess.run([bal] + base + ["--fixed-cameras", "0,2-4", "--compact-fixed-cameras"], capture_output=True, text=True, timeout=120)
    assert "fixed cameras: 4 of 8\ndense system: compacted to the 4 free cameras\n" in r.stdout, r.stdout[-500:] + r.stderr[-500:]
    r = subprocess.run([bal] + base + ["--fixed-cameras", "0,2-4", "--compact-fixed-cameras", "--no-compact-fixed-cameras"],
                       capture_output=True, text=True, timeout=120)
    assert "fixed cameras: 4 of 8\n" in r.stdout and "dense system:" not in r.stdout
    r = subprocess.run([bal] + base + ["--compact-fixed-cameras"], capture_output=True, text=True, timeout=120)
    assert "dense system:" not in r.stdout and "unknown option" not in r.stderr
