"""bal --fp32-terms (SolverOptions::fp32_terms -> POVAR_FLAG_FP32_TERMS; not a reference option, like --deterministic) and the
flag's ABI constants, without a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def binaries():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povar_amd", "csrc"), "host"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "bin", "bal"), os.path.join(ROOT, "build", "bal_oracle")


def test_bal_accepts_fp32_terms(binaries, tmp_path):
    bal, bal_oracle = binaries
    r = subprocess.run([bal, "--help"], capture_output=True, text=True)
    assert "--fp32-terms" in r.stdout
    r = subprocess.run([bal, "--input", str(tmp_path / "missing.txt"), "--fp32-terms"], capture_output=True, text=True)
    assert r.returncode != 0 and "unknown option" not in r.stdout + r.stderr and "Could not open" in r.stdout + r.stderr
    # the oracle-backed twin shares the option parser: a whole run with the option
    from povar_amd import synth
    p = synth.make_problem(10, 300, 1300, seed=21)
    f = str(tmp_path / "p.txt")
    synth.write_data_custom(f, p)
    r = subprocess.run([bal_oracle, "--input", f, "--fp32-terms", "--no-fp32-terms", "--fp32-terms", "--quiet", "--log-log-path",
                        str(tmp_path / "log.json"), "--max-num-iterations-step-1", "2", "--max-num-iterations-step-2", "0"],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-800:]


def test_flag_constants_match_the_header():
    from povar_amd import capi
    h = open(os.path.join(ROOT, "include", "povar_hip.h")).read()
    assert re.search(r"POVAR_FLAG_FP32_TERMS = 1u << 17\b", h)
    assert capi.FLAG_FP32_TERMS == 1 << 17
    # bit 17 is free of every other switch
    for f in (capi.FLAG_DETERMINISTIC, capi.FLAG_DET_GATHER_TERMS, capi.FLAG_NO_GRAPH, capi.FLAG_NO_PACKED_ROWS, 0xF << 4, 0x3 << 8, 0x3 << 12):
        assert f & capi.FLAG_FP32_TERMS == 0
    # the new povar_layout_info field is the struct's last, as appended in the header
    assert capi.LayoutInfo._fields_[-1] == ("fp32_terms", capi.C.c_int32)
    body = h[h.index("typedef struct {\n  int32_t grid;"):h.index("} povar_layout_info;")]
    assert body.rstrip().splitlines()[-2].strip().startswith("int32_t fp32_terms;")
