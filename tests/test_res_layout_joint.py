"""Host-only invariants of the STEP-2 instance of the resident power series' layout (povar_amd/csrc/res_layout.hpp with
res_shape_step2(): the layout of series_res_h, one launch per solve_joint, sc/linearization_power_varproj.hpp:240-287)
through tests/cpp/res_layout_h_check.cpp, which this module compiles itself with plain g++ (the layout header needs no HIP
header): every observation in exactly one lane chunk of its camera, landmark slots that name its landmark inside the
workgroup and inside the compile-time stride of the LDS arrays, partial records camera-major and used once, every camera
owned by exactly one workgroup, no image points, and the LDS capacity under the step-2 formula
    64 + 64 LS T + 8 max(13 cams, 12 records) + owned (8 (121 + 12 + 13 + 11 + 11 + 12 + 2 + 60) + 16) + 4 (cams + records) + 8,
which the checker writes out a second time.  Runs without a GPU.

must_fit of the (wgs, kw) rows of tests/test_res_layout.py, derived again for this shape: the rows that must not fit
fail on LANES (workgroups x lanes x rows < 90 000 observations), which no LDS formula changes.  The three rows that must
fit have at most 300 cameras, so the region is at most 8 * 13 * 300 = 31 200 bytes (its records are (workgroup, camera)
pairs of owned cameras: 256 workgroups own two cameras at most, 256 records each at most -> 49 152; 32 workgroups own
twelve of at most 32 records -> 36 864), the owned cameras at most 12 * 1 952 = 23 424, the index lists under 4 000 and
the landmark arrays 64 * 1024 = 65 536 at either instantiated slot capacity (16 wavefronts x 1, 8 x 2): under 143 000 of
163 840 bytes.  No row changes.
"""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "res_layout_h_check.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "povar_amd", "csrc", h) for h in ("res_layout.hpp", "layout_host.hpp")]
LDS = 160 * 1024


def _build(name, flags):
    out = os.path.join(ROOT, "build", name)
    if not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(s) for s in DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17"] + flags + ["-pthread", "-o", out, SRC])
    return out


def _run(tmp_path, n_cams, lm_off, cam_idx, obs, wgs, n_waves=8, rounds=2, hmin=1, hmax=4, ls_max=2, order=-1, binary=None):
    binary = binary or _build("res_layout_h_check", ["-O1"])
    f = [str(tmp_path / n) for n in ("lm_off.bin", "cam_idx.bin", "obs.bin")]
    np.ascontiguousarray(lm_off, dtype=np.int32).tofile(f[0])
    np.ascontiguousarray(cam_idx, dtype=np.int32).tofile(f[1])
    np.ascontiguousarray(obs, dtype=np.float64).tofile(f[2])
    r = subprocess.run([binary, str(n_cams)] + f + [str(wgs), str(n_waves), str(rounds), str(hmin), str(hmax), str(ls_max), str(order)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


BIG = dict(hmin=4)  # four rows per chunk whatever the problem needs
WIDE = dict(n_waves=16, rounds=1, hmax=2, ls_max=1)  # a 1024-thread shape (the layout's side of it: series_res_h has no such instantiation)


@pytest.mark.parametrize("wgs,kw,must_fit", [(256, {}, True), (256, WIDE, True), (32, WIDE, False), (32, BIG, True), (7, BIG, False), (1, BIG, False),
                                             (90, dict(hmax=1), False), (16, dict(n_waves=8, rounds=1, hmin=8, hmax=8, ls_max=2), False)])
def test_res_layout_joint_invariants_medium(tmp_path, wgs, kw, must_fit):
    from povar_amd import synth
    p = synth.make_problem(300, 20000, 90000, seed=5)
    fits = []
    for order in (-1, 0, 1):
        s = _run(tmp_path, p.n_cams, p.lm_off, p.cam_idx, p.obs, wgs, order=order, **kw)
        assert s["ok"] == 1
        fits.append(s["fits"])
        if s["fits"]:
            assert s["lds_bytes"] <= LDS and s["W"] <= wgs
    if must_fit:
        assert all(fits)


@pytest.mark.parametrize("wgs,kw", [(1, {}), (8, {}), (40, {}), (40, WIDE)])
def test_res_layout_joint_small_problem(tmp_path, small_problem, wgs, kw):
    """Six cameras, 40 landmarks: with 40 workgroups every landmark has its own, and most workgroups own no camera."""
    p = small_problem
    s = _run(tmp_path, p.n_cams, p.lm_off, p.cam_idx, p.obs, wgs, **kw)
    assert s["ok"] == 1 and s["fits"] == 1 and s["W"] <= wgs and s["lds_bytes"] <= LDS, s
    if wgs == 40:
        assert s["W"] == 40 and s["max_lm"] == 1 and s["wg_without_owned"] == 34, s


def test_res_layout_joint_shares_step1_cut_where_it_fits(tmp_path):
    """Step 1's cut serves step 2 where its fullest workgroup fits the LDS under the step-2 formula, and only there.  2000
    cameras over 74 workgroups: 28 owned cameras and 350 records in one workgroup next to 1024 landmark slots are 164 856
    bytes under the step-2 formula (115 k under step 1's) -- not shared; a cut for 1024 slots does not exist then, one for
    512 (ls_max = 1) does.  Over 96 workgroups step 1's cut is step 2's."""
    from povar_amd import synth
    p = synth.make_problem(2000, 12000, 80000, seed=2)
    tight = _run(tmp_path, p.n_cams, p.lm_off, p.cam_idx, p.obs, 74, **BIG)
    assert tight["ok"] == 1 and tight["fits1"] == 1 and tight["lds1_h"] > LDS and tight["shared"] == 0, tight
    own = _run(tmp_path, p.n_cams, p.lm_off, p.cam_idx, p.obs, 74, ls_max=1, **BIG)
    assert own["ok"] == 1 and own["fits"] == 1 and own["LS"] == 1 and own["lds_bytes"] <= LDS, own
    roomy = _run(tmp_path, p.n_cams, p.lm_off, p.cam_idx, p.obs, 96, **BIG)
    assert roomy["ok"] == 1 and roomy["fits1"] == 1 and roomy["lds1_h"] <= LDS and roomy["shared"] == 1, roomy
    assert roomy["fits"] == 1 and roomy["lds_bytes"] <= LDS


def test_res_layout_joint_checker_under_sanitizers(tmp_path, small_problem):
    """The stand-alone checker (the layout builder with it) under AddressSanitizer and UBSan: a medium cut and the small one."""
    from povar_amd import synth
    binary = _build("res_layout_h_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    p = synth.make_problem(300, 20000, 90000, seed=5)
    s = _run(tmp_path, p.n_cams, p.lm_off, p.cam_idx, p.obs, 64, binary=binary, **BIG)
    assert s["ok"] == 1 and s["fits"] == 1
    q = small_problem
    s = _run(tmp_path, q.n_cams, q.lm_off, q.cam_idx, q.obs, 40, binary=binary)
    assert s["ok"] == 1 and s["fits"] == 1
