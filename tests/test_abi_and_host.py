"""CPU-side checks of the product: the C-ABI library loads and exports every symbol declared in
include/povar_hip.h, fails loudly without a GPU, the host-only sharding logic, and the
data_custom reader/writer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from povar_amd import capi
    capi.build()
    lib = capi.lib()
    text = open(os.path.join(ROOT, "include", "povar_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(povar_[a-z0-9_]+)\s*\(", text)))
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in povar_hip.h but not exported"


def test_buffer_ids_of_the_header_and_the_ctypes_mirror_agree():
    """POVAR_BUF_* in the header's order against capi.BUF_* (the covariance inspection ids included), and the setter that
    goes with them."""
    from povar_amd import capi
    text = open(os.path.join(ROOT, "include", "povar_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"enum\s*\{\s*(POVAR_BUF_DIAG2\b.*?)\}", text, flags=re.S).group(1)
    names = re.findall(r"\bPOVAR_(BUF_[A-Z0-9_]+)", body)
    assert len(names) == 18 and names[-4:] == ["BUF_COV_FACTOR", "BUF_COV_INVERSE", "BUF_COV_PANEL", "BUF_COV_GAUGE"]
    for k, n in enumerate(names):
        assert getattr(capi, n) == k, n
    assert hasattr(capi.lib(), "povar_set_cov_inspect") and hasattr(capi.Context, "set_cov_inspect")


def test_no_gpu_fails_loudly():
    """No CPU fallback: without a HIP device povar_create must return an error, never a context."""
    from povar_amd import capi, synth
    import subprocess, sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from povar_amd import capi, synth\n"
            "p = synth.make_problem(4, 10, 30, seed=0)\n"
            "try:\n"
            "    capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs)\n"
            "    print('CREATED')\n"
            "except capi.PovarError as e:\n"
            "    print('ERROR', e)\n") % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert "ERROR" in out.stdout and "CREATED" not in out.stdout, out.stdout + out.stderr


def test_create_rejects_bad_input():
    from povar_amd import capi
    lib = capi.lib()
    h = C.c_void_p()
    opts = capi.Options(0, 1.0, 1e-5, 0, 0)
    lm_off = np.array([0, 2, 4], dtype=np.int32)
    obs = np.zeros((4, 2))
    for cam in ([0, 1, 1, 1], [0, 5, 0, 1], [1, 0, 0, 1]):  # duplicate, out of range, not ascending
        cam_idx = np.array(cam, dtype=np.int32)
        rc = lib.povar_create(C.byref(h), 3, 2, C.c_int64(4), C.c_void_p(lm_off.ctypes.data),
                              C.c_void_p(cam_idx.ctypes.data), C.c_void_p(obs.ctypes.data), C.byref(opts))
        assert rc < 0 and lib.povar_last_error()


def test_shard_range_balances_observations():
    from povar_amd import capi, synth
    p = synth.make_problem(20, 5000, 21000, seed=2)
    for world in (1, 2, 3, 8):
        ranges = [capi.shard_range(p.lm_off, world, r) for r in range(world)]
        assert ranges[0][0] == 0 and ranges[-1][1] == p.n_lms
        assert all(ranges[i][1] == ranges[i + 1][0] for i in range(world - 1))
        counts = [int(p.lm_off[e] - p.lm_off[b]) for b, e in ranges]
        assert sum(counts) == p.n_obs and max(counts) - min(counts) <= 2 * int(np.diff(p.lm_off).max())


def test_data_custom_roundtrip(tmp_path):
    from povar_amd import synth
    p = synth.make_problem(5, 30, 100, seed=9)
    f = str(tmp_path / "problem.txt")
    synth.write_data_custom(f, p)
    q = synth.read_data_custom(f)
    assert (q.n_cams, q.n_lms, q.n_obs) == (p.n_cams, p.n_lms, p.n_obs)
    assert np.array_equal(q.lm_off, p.lm_off) and np.array_equal(q.cam_idx, p.cam_idx)
    assert np.abs(q.obs - p.obs).max() < 1e-12 and np.abs(q.cams - p.cams).max() < 1e-12
    # a duplicate (camera, landmark) pair aborts the reference loader (bal_problem.cpp:227)
    lines = open(f).read().split("\n")
    lines[2] = lines[1]
    open(f, "w").write("\n".join(lines))
    with pytest.raises(ValueError):
        synth.read_data_custom(f)


def test_bal_shapes():
    from povar_amd import synth
    p = synth.make_bal_problem("ladybug-49")
    assert (p.n_cams, p.n_lms, p.n_obs) == (49, 7776, 31843)
    k = np.diff(p.lm_off)
    assert k.min() >= 2 and k.max() <= 49
    # strictly ascending camera index inside every landmark
    same = np.repeat(np.arange(p.n_lms), k)
    assert np.all((np.diff(p.cam_idx) > 0) | (np.diff(same) > 0))


def test_read_bal_file_original_and_custom(tmp_path):
    """$POVAR_BAL_DIR support of bench.py: an original-format BAL file (9 camera parameters,
    optionally .bz2) and its data_custom twin give the same observation structure; the original one gets
    create-dataset style cameras."""
    import bz2
    from povar_amd import synth
    p = synth.make_problem(7, 60, 260, seed=4)
    lm_of = np.repeat(np.arange(p.n_lms), np.diff(p.lm_off))
    perm = np.random.default_rng(0).permutation(p.n_obs)           # BAL files are not required to be sorted
    lines = [f"{p.n_cams} {p.n_lms} {p.n_obs}"]
    lines += [f"{p.cam_idx[i]} {lm_of[i]} {p.obs[i, 0]:.6f} {-p.obs[i, 1]:.6f}" for i in perm]
    for c in range(p.n_cams):
        lines += ["0.1", "0.2", "0.3", "0", "0", "-5", "800", "0", "0"]
    lines += [f"{x:.6f}" for x in p.lms.ravel()]
    d = tmp_path / "bal"
    d.mkdir()
    name = synth.BAL_FILES["ladybug-49"]
    with bz2.open(d / (name + ".bz2"), "wt") as fh:
        fh.write("\n".join(lines) + "\n")
    found = synth.find_bal_file("ladybug-49", str(d))
    assert found and found.endswith(".bz2") and synth.find_bal_file("venice-1778", str(d)) is None
    q = synth.read_bal_file(found, seed=5)
    assert (q.n_cams, q.n_lms, q.n_obs) == (p.n_cams, p.n_lms, p.n_obs)
    assert np.array_equal(q.lm_off, p.lm_off) and np.array_equal(q.cam_idx, p.cam_idx)
    assert np.abs(q.obs - p.obs).max() < 1e-6
    assert np.allclose(q.cams[:, 8:], [0, 0, 0, 1]) and np.abs(q.cams[:, :8]).max() > 0.1
    assert np.array_equal(synth.read_bal_file(found, seed=5).cams, q.cams)
    (d / "data_custom").mkdir()
    synth.write_data_custom(str(d / "data_custom" / name), p)
    found2 = synth.find_bal_file("ladybug-49", str(d))
    assert "data_custom" in found2
    r = synth.read_bal_file(found2)
    assert np.array_equal(r.cam_idx, p.cam_idx) and np.abs(r.cams - p.cams).max() < 1e-6


def test_options_struct_mirror_and_flag_fields():
    """povar_options as the header declares it (the flags word of VERDICT r05 item 6 included) against the ctypes mirror the
    tests and bench.py pass through the ABI: same field order; the flag helpers produce the header's bit fields."""
    import re
    from povar_amd import capi
    hdr = open(capi.HEADER).read()
    body = hdr[hdr.index("/* LandmarkBlockSC::Options"):hdr.index("} povar_options;")]
    names = re.findall(r"^\s+(?:int32_t|uint32_t|double)\s+(\w+);", body, flags=re.M)
    assert names == [f[0] for f in capi.Options._fields_] == ["robust_norm", "huber_parameter", "jacobi_scaling_eps", "device", "e0_mode", "flags"]
    val = {k: int(v) for k, v in re.findall(r"(POVAR_FLAG_\w+) = 1u << (\d+)", hdr)}
    assert capi.FLAG_DETERMINISTIC == 1 << val["POVAR_FLAG_DETERMINISTIC"] and capi.FLAG_DET_GATHER_TERMS == 1 << val["POVAR_FLAG_DET_GATHER_TERMS"]
    assert capi.FLAG_NO_GRAPH == 1 << val["POVAR_FLAG_NO_GRAPH"] and capi.FLAG_NO_PACKED_ROWS == 1 << val["POVAR_FLAG_NO_PACKED_ROWS"]
    assert capi.flag_e0_kernel(-1) == 0 and capi.flag_e0_kernel(0) == 1 << 4 and capi.flag_e0_kernel(6) == 7 << 4
    assert capi.flag_series_kernel(-1) == 0 and capi.flag_series_kernel(1) == 2 << 8 and capi.flag_placement(3) == 3 << 12
