"""What povar_create makes of a table of switches (povar_options.flags x environment), on two synthetic problems: every field of
povar_layout_info that is not a time, povar_device_bytes after the creation and after layout_finalize(wait=True) -- or, for a
refused combination, the return code's message -- and, for the deterministic rows, the bits of one 20-term solve per step.  The
A/B of a change that may move none of it (the resolver of create_plan.hpp: run it with POVAR_LIB on two builds of the library;
the outputs are compared line for line -- profiles/create_plan_matrix.txt).  The rows are those of tests/cpp/create_plan_check.cpp
that a device can be asked (the CU count and the sizes are the device's and the problems').
usage: [POVAR_LIB=<library>] python3 tools/create_matrix.py"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from povar_amd import capi, synth  # noqa: E402

ALPHA, LAM, M = 0.01, 1e-4, 20
DET, F32 = capi.FLAG_DETERMINISTIC, capi.FLAG_FP32_TERMS
K, S, P = capi.flag_e0_kernel, capi.flag_series_kernel, capi.flag_placement
LDSACC = capi.E0_IMPLICIT_LDSACC

# (name, flags, environment, e0_mode, robust norm, print the bits of a solve per step)
ROWS = [
    ("defaults", 0, {}, LDSACC, "NONE", False),
    ("default E0 mode", 0, {}, capi.E0_IMPLICIT, "NONE", False),
    ("E0 mode TILES", 0, {}, capi.E0_TILES, "NONE", False),
    ("deterministic: flag", DET, {}, LDSACC, "NONE", True),
    ("deterministic: variable without the flag", 0, {"POVAR_DETERMINISTIC": "1"}, LDSACC, "NONE", False),
    ("deterministic: variable 0 over the flag", DET, {"POVAR_DETERMINISTIC": "0"}, LDSACC, "NONE", False),
    ("NO_GRAPH: flag", capi.FLAG_NO_GRAPH, {}, LDSACC, "NONE", False),
    ("NO_GRAPH: variable 0 over the flag", capi.FLAG_NO_GRAPH, {"POVAR_NO_GRAPH": "0"}, LDSACC, "NONE", False),
    ("NO_GRAPH: variable without the flag", 0, {"POVAR_NO_GRAPH": "1"}, LDSACC, "NONE", False),
    ("E0 kernel: flag 3", K(3), {}, LDSACC, "NONE", False),
    ("E0 kernel: flag 0", K(0), {}, LDSACC, "NONE", False),
    ("E0 kernel: variable 0 over flag 3", K(3), {"POVAR_E0_CK": "0"}, LDSACC, "NONE", False),
    ("E0 kernel: variable 4 over flag 0", K(0), {"POVAR_E0_CK": "4"}, LDSACC, "NONE", False),
    ("E0 kernel: variable 5", 0, {"POVAR_E0_CK": "5"}, LDSACC, "NONE", False),
    ("E0 kernel: variable 2", 0, {"POVAR_E0_CK": "2"}, LDSACC, "NONE", False),
    ("E0 kernel: variable 9 is clamped", 0, {"POVAR_E0_CK": "9"}, LDSACC, "NONE", False),
    ("E0 kernel: variable -1 over flag 2", K(2), {"POVAR_E0_CK": "-1"}, LDSACC, "NONE", False),
    ("series kernel: flag 1", S(1), {}, LDSACC, "NONE", False),
    ("series kernel: flag 0", S(0), {}, LDSACC, "NONE", False),
    ("series kernel: variable 0 over flag 1", S(1), {"POVAR_RES": "0"}, LDSACC, "NONE", False),
    ("series kernel: variable 1 over flag 0", S(0), {"POVAR_RES": "1"}, LDSACC, "NONE", False),
    ("placement: flag 1", P(1), {}, LDSACC, "NONE", False),
    ("placement: flag 2", P(2), {}, LDSACC, "NONE", False),
    ("placement: flag 3", P(3), {}, LDSACC, "NONE", False),
    ("placement: variable sync over flag 2", P(2), {"POVAR_LPL_PLACE": "sync"}, LDSACC, "NONE", False),
    ("placement: variable async over flag 1", P(1), {"POVAR_LPL_PLACE": "async"}, LDSACC, "NONE", False),
    ("placement: variable async, step 2's chunk layout early", 0, {"POVAR_LPL_PLACE": "async", "POVAR_CKH_EARLY": "1"}, LDSACC, "NONE", False),
    ("placement: variable none", 0, {"POVAR_LPL_PLACE": "none"}, LDSACC, "NONE", False),
    ("placement: an unknown word", 0, {"POVAR_LPL_PLACE": "later"}, LDSACC, "NONE", False),
    ("placement: NOPLACE alone", 0, {"POVAR_LPL_NOPLACE": "1"}, LDSACC, "NONE", False),
    ("placement: NOPLACE over flag 2", P(2), {"POVAR_LPL_NOPLACE": "1"}, LDSACC, "NONE", False),
    ("placement: NOPLACE loses to PLACE=sync", 0, {"POVAR_LPL_NOPLACE": "1", "POVAR_LPL_PLACE": "sync"}, LDSACC, "NONE", False),
    ("deterministic: kernels pinned", DET | K(2) | S(1), {"POVAR_E0_CK": "3", "POVAR_RES": "1"}, LDSACC, "NONE", True),
    ("deterministic: E0 mode TILES_LDSACC asked", DET, {}, capi.E0_TILES_LDSACC, "NONE", False),
    ("deterministic: forced sync", DET, {"POVAR_LPL_PLACE": "sync"}, LDSACC, "NONE", True),
    ("deterministic: placement flag 1", DET | P(1), {}, LDSACC, "NONE", False),
    ("deterministic: forced async", DET, {"POVAR_LPL_PLACE": "async"}, LDSACC, "NONE", False),
    ("deterministic: POVAR_DET_CK=0", DET, {"POVAR_DET_CK": "0"}, LDSACC, "NONE", True),
    ("deterministic: gather-terms flag", DET | capi.FLAG_DET_GATHER_TERMS, {}, LDSACC, "NONE", False),
    ("deterministic: POVAR_DET_CK=1 over the gather-terms flag", DET | capi.FLAG_DET_GATHER_TERMS, {"POVAR_DET_CK": "1"}, LDSACC, "NONE", False),
    ("gather-terms flag alone", capi.FLAG_DET_GATHER_TERMS, {}, LDSACC, "NONE", False),
    ("deterministic with HUBER", DET, {}, LDSACC, "HUBER", False),
    ("fp32: deterministic first", F32 | DET, {"POVAR_RES": "1", "POVAR_E0_CK": "0"}, capi.E0_IMPLICIT, "NONE", False),
    ("fp32: deterministic by variable", F32, {"POVAR_DETERMINISTIC": "1"}, LDSACC, "NONE", False),
    ("fp32: then the forced resident series", F32, {"POVAR_RES": "1", "POVAR_E0_CK": "0"}, capi.E0_IMPLICIT, "NONE", False),
    ("fp32: resident series by flag", F32 | S(1), {}, LDSACC, "NONE", False),
    ("fp32: then the forced e0_lpl", F32, {"POVAR_E0_CK": "0"}, capi.E0_IMPLICIT, "NONE", False),
    ("fp32: e0_lpl by flag", F32 | K(0), {}, LDSACC, "NONE", False),
    ("fp32: then the E0 mode", F32, {}, capi.E0_IMPLICIT, "NONE", False),
    ("fp32: by variable", 0, {"POVAR_FP32_TERMS": "1"}, capi.E0_TILES_LDSACC, "NONE", False),
    ("fp32: variable 0 over the flag", F32, {"POVAR_FP32_TERMS": "0"}, LDSACC, "NONE", False),
    ("fp32: accepted", F32, {}, LDSACC, "NONE", False),
    ("fp32: variables lift the refusing flags", F32 | S(1) | K(0), {"POVAR_RES": "0", "POVAR_E0_CK": "3"}, LDSACC, "NONE", False),
    ("fp32: POVAR_E0_V1=1, no placement asked for", F32, {"POVAR_E0_V1": "1", "POVAR_PREPARE_V1": "1", "POVAR_LPL_PLACE": "none"}, LDSACC, "NONE", False),
    ("fp32: no chunk layout", F32, {"POVAR_NO_CK": "1"}, LDSACC, "NONE", False),
    ("HUBER", 0, {}, LDSACC, "HUBER", False),
    ("CAUCHY", 0, {}, LDSACC, "CAUCHY", False),
    ("POVAR_CK_COLD_RECORDS", 0, {"POVAR_CK_COLD_RECORDS": "1"}, LDSACC, "NONE", False),
    ("POVAR_CK_HMAX=0", 0, {"POVAR_CK_HMAX": "0"}, LDSACC, "NONE", False),
    ("POVAR_CK_HMAX=99", 0, {"POVAR_CK_HMAX": "99"}, LDSACC, "NONE", False),
    ("POVAR_CK_HMAX=5", 0, {"POVAR_CK_HMAX": "5"}, LDSACC, "NONE", False),
    ("POVAR_HOT_ACC=0", 0, {"POVAR_HOT_ACC": "0"}, LDSACC, "NONE", False),
    ("POVAR_HOT_ACC=20", 0, {"POVAR_HOT_ACC": "20"}, LDSACC, "NONE", False),
    ("POVAR_HOT_ACC=20, lane per observation", 0, {"POVAR_HOT_ACC": "20", "POVAR_E0_V1": "1"}, LDSACC, "NONE", False),
    ("POVAR_HOT_ACC=9999", 0, {"POVAR_HOT_ACC": "9999"}, LDSACC, "NONE", False),
    ("POVAR_E0_WGS=0", 0, {"POVAR_E0_WGS": "0"}, LDSACC, "NONE", False),
    ("POVAR_E0_WGS=40", 0, {"POVAR_E0_WGS": "40"}, LDSACC, "NONE", False),
    ("POVAR_RES_OBS_PER_WG=10", 0, {"POVAR_RES_OBS_PER_WG": "10"}, LDSACC, "NONE", False),
    ("POVAR_RES_OBS_PER_WG=1000", 0, {"POVAR_RES_OBS_PER_WG": "1000"}, LDSACC, "NONE", False),
    ("POVAR_RES_WGS=0", 0, {"POVAR_RES_WGS": "0"}, LDSACC, "NONE", False),
    ("POVAR_RES_WGS=12", 0, {"POVAR_RES_WGS": "12"}, LDSACC, "NONE", False),
    ("POVAR_RES_WGS=9999", 0, {"POVAR_RES_WGS": "9999"}, LDSACC, "NONE", False),
    ("POVAR_RES_SPIN=0", 0, {"POVAR_RES_SPIN": "0"}, LDSACC, "NONE", False),
    ("POVAR_RES_MAX_OBS=1000", 0, {"POVAR_RES_MAX_OBS": "1000"}, LDSACC, "NONE", False),
    ("POVAR_CK_MAX_CAMS=-5", 0, {"POVAR_CK_MAX_CAMS": "-5", "POVAR_E0_V1": "0"}, LDSACC, "NONE", False),
    ("POVAR_CK_MAX_CAMS=10, rows placed on a host thread", 0, {"POVAR_CK_MAX_CAMS": "10", "POVAR_E0_V1": "0", "POVAR_LPL_PLACE": "async"}, LDSACC, "NONE", False),
    ("POVAR_CK_MAX_CAMS=1000", 0, {"POVAR_CK_MAX_CAMS": "1000", "POVAR_E0_V1": "0"}, LDSACC, "NONE", False),
    ("CU mask: not a range", 0, {"POVAR_CU_MASK": "half"}, LDSACC, "NONE", False),
    ("CU mask: one number", 0, {"POVAR_CU_MASK": "12"}, LDSACC, "NONE", False),
    ("CU mask: last before first", 0, {"POVAR_CU_MASK": "4-2"}, LDSACC, "NONE", False),
    ("CU mask: negative first", 0, {"POVAR_CU_MASK": "-1-3"}, LDSACC, "NONE", False),
    ("CU mask: past the device's CUs", 0, {"POVAR_CU_MASK": "0-100000"}, LDSACC, "NONE", False),
    ("CU mask: checked before the fp32 refusals", F32 | DET, {"POVAR_CU_MASK": "0-100000"}, LDSACC, "NONE", False),
    ("CU mask: 32 CUs", 0, {"POVAR_CU_MASK": "32-63"}, LDSACC, "NONE", False),
    ("CU mask: 32 CUs, the workgroup knobs against the range", 0, {"POVAR_CU_MASK": "0-31", "POVAR_E0_WGS": "100", "POVAR_RES_WGS": "100"}, LDSACC, "NONE", False),
    ("POVAR_NO_CK", 0, {"POVAR_NO_CK": "1"}, LDSACC, "NONE", False),
    ("POVAR_E0_V1=1", 0, {"POVAR_E0_V1": "1"}, LDSACC, "NONE", False),
    ("POVAR_E0_V1=0", 0, {"POVAR_E0_V1": "0"}, LDSACC, "NONE", False),
    ("POVAR_E0_V1=0, forced variant 4", 0, {"POVAR_E0_V1": "0", "POVAR_E0_CK": "4"}, LDSACC, "NONE", False),
    ("POVAR_E0_V1=0, HUBER", 0, {"POVAR_E0_V1": "0"}, LDSACC, "HUBER", False),
    ("POVAR_E0_V1=0, deterministic", DET, {"POVAR_E0_V1": "0"}, LDSACC, "NONE", True),
    ("POVAR_NO_ERR_MEMO, POVAR_GRAPH_COMM, POVAR_NO_FUSE", 0, {"POVAR_NO_ERR_MEMO": "1", "POVAR_GRAPH_COMM": "1", "POVAR_NO_FUSE": "1"}, LDSACC, "NONE", False),
    ("POVAR_K1_NORMAL_EQ, POVAR_PREPARE_V1", 0, {"POVAR_K1_NORMAL_EQ": "1", "POVAR_PREPARE_V1": "1"}, LDSACC, "NONE", False),
    ("POVAR_CK_NOPLACE", 0, {"POVAR_CK_NOPLACE": "1", "POVAR_E0_V1": "0"}, LDSACC, "NONE", False),
    ("POVAR_FLAG_NO_PACKED_ROWS", capi.FLAG_NO_PACKED_ROWS, {"POVAR_E0_V1": "0"}, LDSACC, "NONE", False),
    ("POVAR_COLD_Q_ROWS=0", 0, {"POVAR_COLD_Q_ROWS": "0"}, LDSACC, "NONE", False),
    ("POVAR_COLD_Q_ROWS=1", 0, {"POVAR_COLD_Q_ROWS": "1"}, LDSACC, "NONE", False),
    ("POVAR_LONG_SEPARATE", 0, {"POVAR_LONG_SEPARATE": "1"}, LDSACC, "NONE", False),
]
KNOBS = sorted({k for row in ROWS for k in row[2]})


def problems():
    """The 29-camera problem of tools/ctx_bytes.py (lane per observation by default), and one just over 65536 observations (lane per
    landmark, a chunk layout that is ready)."""
    return (("29 cameras", synth.make_problem(29, 400, 2400, seed=11, popularity="uniform")),
            ("257 cameras", synth.make_problem(257, 14000, 70000, seed=4)))


def solve_bits(ctx, p):
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(ALPHA)
    assert ctx.linearize_pose(ALPHA)
    inc, _, _, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
    assert rc == 0
    yield "step-1", hashlib.sha256(inc.tobytes()).hexdigest()
    lms = ctx.get_landmarks()
    ctx.set_landmarks_homogeneous(np.concatenate([lms, np.ones((p.n_lms, 1))], axis=1))
    ctx.normalize_joint()
    assert ctx.linearize_homogeneous()
    inc, _, _, rc = ctx.solve_joint(LAM, M)
    assert rc == 0
    yield "step-2", hashlib.sha256(inc.tobytes()).hexdigest()


def main():
    for tag, p in problems():
        for name, flags, env, e0_mode, robust, bits in ROWS:
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update(env)
            head = f"{tag} | {name}"
            try:
                ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=robust, e0_mode=e0_mode, flags=flags)
            except capi.PovarError as e:
                print(f"{head}: refused: {e}", flush=True)
                continue
            li = ctx.layout_info()
            fields = " ".join(f"{f}={getattr(li, f)}" for f, _ in capi.LayoutInfo._fields_ if not f.endswith(("_ms", "_us")))
            print(f"{head}: {fields}")
            print(f"{head}: device_bytes after create: {ctx.device_bytes()}")
            ctx.layout_finalize(wait=True)
            print(f"{head}: device_bytes after layout_finalize(wait=True): {ctx.device_bytes()}, placement {ctx.layout_info().placement}")
            if bits:
                for step, sha in solve_bits(ctx, p):
                    print(f"{head}: sha256 of the {step} increment: {sha}")
            sys.stdout.flush()
            ctx.close()
    for k in KNOBS:
        os.environ.pop(k, None)


if __name__ == "__main__":
    main()
