"""What povar_create makes of its switches, on a device: rows of the table of tests/cpp/create_plan_check.cpp (the resolver of
povar_amd/csrc/create_plan.hpp, checked there field by field without a device) held to povar_layout_info -- the environment over
the flag, what deterministic mode pins, the fp32 terms accepted and refused, the placement.  Two problems: the 29-camera one of
tools/ctx_bytes.py (2400 observations: lane per observation by default) and one of 70 000 (over 65536: lane per landmark, with a
camera-chunk layout).  The expected values are the CPU table's, read through povar_get_layout_info:
  lane_per_landmark = use_lpl;  placement = place_mode;  e0_auto = ck_auto, res_auto = (res_mode == -1), both before any timing;
  ck_ready = want_ck (every layout of these problems is one the chunk kernels can run);
  e0_kernel = 7 on a deterministic context with det_ck and a chunk layout, else the forced ck_variant where there is a chunk
  layout, else 0;  fp32_terms = 1 after a step-1 solve of an fp32 context."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALPHA, LAM, M = 0.01, 1e-4, 5
_KNOBS = ("POVAR_DETERMINISTIC", "POVAR_DET_CK", "POVAR_FP32_TERMS", "POVAR_E0_CK", "POVAR_RES", "POVAR_E0_V1", "POVAR_PREPARE_V1", "POVAR_NO_CK",
          "POVAR_NO_GRAPH", "POVAR_LPL_PLACE", "POVAR_LPL_NOPLACE", "POVAR_CK_MAX_CAMS", "POVAR_CU_MASK", "POVAR_CKH_EARLY")
REFUSED = "POVAR_FLAG_FP32_TERMS cannot be combined with "


@pytest.fixture(scope="module")
def problems():
    from povar_amd import synth
    return {"small": synth.make_problem(29, 400, 2400, seed=11, popularity="uniform"),
            "large": synth.make_problem(257, 14000, 70000, seed=4)}


def _flags(det=False, f32=False, kernel=None, series=None, placement=0):
    from povar_amd import capi
    return ((capi.FLAG_DETERMINISTIC if det else 0) | (capi.FLAG_FP32_TERMS if f32 else 0) | (0 if kernel is None else capi.flag_e0_kernel(kernel)) |
            (0 if series is None else capi.flag_series_kernel(series)) | capi.flag_placement(placement))


def _info(lpl, placement, e0_kernel, e0_auto, res_auto, ck_ready, fp32_after_solve=None):
    d = dict(lane_per_landmark=lpl, placement=placement, e0_kernel=e0_kernel, e0_auto=e0_auto, res_auto=res_auto, ck_ready=ck_ready)
    return d, fp32_after_solve


LDSACC, IMPLICIT = 2, 0
DEFAULT = {"small": _info(0, 1, 0, 1, 1, 0, 0), "large": _info(1, 1, 0, 1, 1, 1, 0)}
DET = {"small": _info(0, 0, 0, 0, 0, 0), "large": _info(1, 0, 7, 0, 0, 1)}
# (id, flags, environment, e0_mode, {problem: expected fields, or the refusal's text})
ROWS = [
    ("defaults", dict(), {}, LDSACC, DEFAULT),
    ("deterministic-variable-without-the-flag", dict(), {"POVAR_DETERMINISTIC": "1"}, LDSACC, DET),
    ("deterministic-variable-0-over-the-flag", dict(det=True), {"POVAR_DETERMINISTIC": "0"}, LDSACC, DEFAULT),
    ("deterministic-pins-the-kernels", dict(det=True, kernel=2, series=1), {"POVAR_E0_CK": "3", "POVAR_RES": "1"}, LDSACC, DET),
    ("deterministic-keeps-a-forced-sync", dict(det=True), {"POVAR_LPL_PLACE": "sync"}, LDSACC,
     {"small": _info(0, 1, 0, 0, 0, 0), "large": _info(1, 1, 7, 0, 0, 1)}),
    ("deterministic-forced-async-is-none", dict(det=True), {"POVAR_LPL_PLACE": "async"}, LDSACC, DET),
    ("deterministic-gather-terms", dict(det=True), {"POVAR_DET_CK": "0"}, LDSACC, {"small": _info(0, 0, 0, 0, 0, 0), "large": _info(1, 0, 0, 0, 0, 1)}),
    ("e0-kernel-variable-0-over-flag-3", dict(kernel=3), {"POVAR_E0_CK": "0"}, LDSACC, {"small": _info(0, 1, 0, 0, 1, 0), "large": _info(1, 1, 0, 0, 1, 1)}),
    ("e0-kernel-variable-1-over-flag-0", dict(kernel=0), {"POVAR_E0_CK": "1"}, LDSACC, {"small": _info(0, 1, 0, 0, 1, 0), "large": _info(1, 1, 1, 0, 1, 1)}),
    ("series-kernel-variable-0-over-flag-1", dict(series=1), {"POVAR_RES": "0"}, LDSACC, {"small": _info(0, 1, 0, 1, 0, 0), "large": _info(1, 1, 0, 1, 0, 1)}),
    ("placement-flag-3-is-none", dict(placement=3), {}, LDSACC, {"small": _info(0, 0, 0, 1, 1, 0), "large": _info(1, 0, 0, 1, 1, 1)}),
    ("placement-variable-async-over-flag-1", dict(placement=1), {"POVAR_LPL_PLACE": "async"}, LDSACC,
     {"small": _info(0, 2, 0, 1, 1, 0), "large": _info(1, 2, 0, 1, 1, 1)}),
    ("placement-noplace-loses-to-sync", dict(), {"POVAR_LPL_NOPLACE": "1", "POVAR_LPL_PLACE": "sync"}, LDSACC, DEFAULT),
    ("lane-per-landmark-forced-without-chunk-layout", dict(), {"POVAR_E0_V1": "0", "POVAR_NO_CK": "1"}, LDSACC,
     {"small": _info(1, 1, 0, 1, 1, 0), "large": _info(1, 1, 0, 1, 1, 0)}),
    ("fp32-accepted-whatever-POVAR_E0_V1-and-the-placement-say", dict(f32=True), {"POVAR_E0_V1": "1", "POVAR_PREPARE_V1": "1", "POVAR_LPL_PLACE": "none"}, LDSACC,
     {"small": _info(1, 1, 1, 1, 0, 1, 1), "large": _info(1, 1, 1, 1, 0, 1, 1)}),
    ("fp32-refused-deterministic-first", dict(f32=True, det=True), {"POVAR_RES": "1", "POVAR_E0_CK": "0"}, IMPLICIT,
     REFUSED + "POVAR_FLAG_DETERMINISTIC: its adds land in arrival order"),
    ("fp32-refused-then-the-resident-series", dict(f32=True), {"POVAR_RES": "1", "POVAR_E0_CK": "0"}, IMPLICIT,
     REFUSED + "POVAR_FLAG_SERIES_KERNEL(1): the resident series has no fp32 form"),
    ("fp32-refused-then-e0_lpl", dict(f32=True, kernel=0), {}, IMPLICIT, REFUSED + "POVAR_FLAG_E0_KERNEL(0): the fp32 terms are a camera-chunk kernel"),
    ("fp32-refused-then-the-e0-mode", dict(), {"POVAR_FP32_TERMS": "1"}, IMPLICIT, REFUSED + "an E0 mode other than POVAR_E0_IMPLICIT_LDSACC"),
    ("cu-mask-past-the-device", dict(), {"POVAR_CU_MASK": "0-100000"}, LDSACC, "POVAR_CU_MASK: expected <first>-<last> inside the device's CU range"),
]


@pytest.mark.parametrize("size", ["small", "large"])
@pytest.mark.parametrize("name,flags,env,e0_mode,expected", ROWS, ids=[r[0] for r in ROWS])
def test_povar_create_resolves_its_switches(problems, monkeypatch, size, name, flags, env, e0_mode, expected):
    from povar_amd import capi
    p = problems[size]
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # (undone after the test)
    create = lambda: capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, e0_mode=e0_mode, flags=_flags(**flags))  # noqa: E731
    if isinstance(expected, str):
        with pytest.raises(capi.PovarError) as e:
            create()
        assert str(e.value) == f"povar_hip rc=-1: {expected}"
        return
    fields, fp32_after_solve = expected[size]
    ctx = create()
    li = ctx.layout_info()
    got = {k: getattr(li, k) for k in fields}
    print(f"{name} / {size}: {got}")
    assert got == fields
    if fp32_after_solve is not None:
        ctx.set_cameras(p.cams)
        ctx.init_landmarks_pose(ALPHA)
        assert ctx.linearize_pose(ALPHA)
        inc, it, _, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
        assert rc == 0 and it == M and np.all(np.isfinite(inc))
        assert ctx.layout_info().fp32_terms == fp32_after_solve
    ctx.close()
