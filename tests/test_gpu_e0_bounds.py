"""Every step-1 E0 family held to the componentwise rounding-error bound of tests/rounding_bounds.py: for EVERY output entry,
|y_dev - y_ref| <= bound_i, with the long-double reference and the bound built from the context's own G (BUF_HLL_INV,
BUF_JL_COL_SCALE), sigma (BUF_POSE_SCALING), cameras and landmarks.  Unlike the relative 2-norms of the other modules this
checks a one-observation camera as hard as a hub, and it holds the fp32 terms (POVAR_FLAG_FP32_TERMS) to a bound that
scales with the conditioning of the landmark blocks instead of a normwise 1e-5 they cannot meet.

Families: e0_lpl, e0_ck, e0_ck_det, e0_ck_f32 (the C-form, lane per landmark / camera chunk), and the lane-per-observation
kernels of E0_IMPLICIT (C-form) and of the two stored-tile modes (explicit-form model) at the sizes where they run.  Each
case forces its kernel itself (environment, flags, setters) and checks that it ran.  Under an environment that pins another
kernel (POVAR_DETERMINISTIC=1: tools/forced_mode_suite.sh) the cases that would not run their kernel skip.
"""
import os

import numpy as np
import pytest

import rounding_bounds as RB
from conftest import rel

pytestmark = pytest.mark.gpu
ALPHA, LAM = 0.01, 1e-4
DET_ENV = os.environ.get("POVAR_DETERMINISTIC") == "1"
CK_VARIANTS = 6

# family: (environment, e0 mode, flags, model)
FAMILIES = {
    "e0_lpl": ({"POVAR_E0_V1": "0", "POVAR_E0_CK": "0", "POVAR_LPL_PLACE": "sync"}, "E0_IMPLICIT_LDSACC", 0, "fp64"),
    "e0_ck": ({"POVAR_E0_V1": "0", "POVAR_E0_CK": "1", "POVAR_LPL_PLACE": "sync"}, "E0_IMPLICIT_LDSACC", 0, "fp64"),
    "e0_ck_det": ({"POVAR_E0_V1": "0", "POVAR_LPL_PLACE": "sync", "POVAR_DETERMINISTIC": "1"}, "E0_IMPLICIT_LDSACC", 0, "det"),
    "e0_ck_f32": ({}, "E0_IMPLICIT_LDSACC", "FLAG_FP32_TERMS", "fp32"),
    "implicit": ({"POVAR_E0_V1": "1"}, "E0_IMPLICIT", 0, "fp64"),
    "tiles": ({"POVAR_E0_V1": "1"}, "E0_TILES", 0, "explicit"),
    "tiles_ldsacc": ({"POVAR_E0_V1": "1"}, "E0_TILES_LDSACC", 0, "explicit"),
}
C_FORM = ["e0_lpl", "e0_ck", "e0_ck_det", "e0_ck_f32"]
CHUNK = ["e0_ck", "e0_ck_det", "e0_ck_f32"]
PER_OBS = ["implicit", "tiles", "tiles_ldsacc"]


def _problem(name):
    from povar_amd import synth
    if name == "local-900":
        return synth.make_problem(900, 40000, 200000, seed=9, popularity="local")
    if name == "p257":
        return synth.make_problem(257, 12000, 60000, seed=4)
    return synth.make_bal_problem(name)


_CACHE = {}


def _cached(name):
    if name not in _CACHE:
        _CACHE.clear()  # (one problem at a time: venice is 5 M observations)
        _CACHE[name] = _problem(name)
    return _CACHE[name]


def _context(monkeypatch, fam, n_cams, lm_off, cam_idx, obs, cams, robust="NONE", huber=1.0, flags=0, lms=None):
    from povar_amd import capi
    env, mode, fl, _ = FAMILIES[fam]
    if DET_ENV and fam != "e0_ck_det":
        pytest.skip("POVAR_DETERMINISTIC=1 in the environment pins the kernel of this case")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if fam == "e0_ck_f32":
        monkeypatch.delenv("POVAR_E0_CK", raising=False)
    flags |= getattr(capi, fl) if fl else 0
    ctx = capi.Context(n_cams, lm_off, cam_idx, obs, robust_norm=robust, huber=huber, e0_mode=getattr(capi, mode), flags=flags)
    ctx.layout_finalize(True)
    ctx.set_cameras(cams)
    if lms is None:
        ctx.init_landmarks_pose(ALPHA)
    else:
        ctx.set_landmarks(lms)
    assert ctx.linearize_pose(ALPHA)
    ctx.prepare_pose(LAM)
    li = ctx.layout_info()
    if fam in ("e0_lpl", "e0_ck"):
        assert li.lane_per_landmark == 1 and li.e0_kernel == (0 if fam == "e0_lpl" else 1), (li.lane_per_landmark, li.e0_kernel)
    elif fam == "e0_ck_det":
        assert li.e0_kernel == CK_VARIANTS + 1, li.e0_kernel
    elif fam in PER_OBS:
        assert li.lane_per_landmark == 0
    return ctx


def _run(ctx, fam, obs, robust, huber, xs, label):
    """Every x against the bound; returns the worst err / bound."""
    prob = RB.Step1.from_context(ctx, obs, ALPHA, robust, huber)
    model = RB.MODELS[FAMILIES[fam][3]]
    worst = 0.0
    for what, x in xs:
        y = ctx.right_mul_e0_pose(x)
        y_ref, bound = RB.evaluate(prob, x, model)
        r, i, n_over = RB.check(y, y_ref, bound)
        print(f"E0BOUND {label} {fam} x={what} err/bound={r:.3g} rel={rel(y, y_ref.astype(np.float64)):.3g} over={n_over}")
        assert n_over == 0, (what, r, i // 12, i % 12, float(y[i]), float(y_ref[i]), float(bound[i]))
        assert np.all(np.isfinite(y))
        worst = max(worst, r)
    return worst


def _xs(n_cams, ctx=None, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=12 * n_cams)
    out = [("normal", x), ("scaled", x * np.repeat(10.0 ** rng.uniform(-4, 4, n_cams), 12))]
    if ctx is not None:
        ctx.power_series_begin()
        ctx.power_series_step()
        out.append(("term", ctx.get_term()))
    return out


SIZES = [(f, n) for n in ("ladybug-49", "trafalgar-257", "local-900") for f in C_FORM] + \
        [(f, "venice-1778") for f in CHUNK] + [(f, "ladybug-49") for f in PER_OBS]


@pytest.mark.parametrize("fam,name", SIZES)
def test_e0_within_bound_at_size(monkeypatch, fam, name):
    p = _cached(name)
    ctx = _context(monkeypatch, fam, p.n_cams, p.lm_off, p.cam_idx, p.obs, p.cams)
    xs = _xs(p.n_cams) if name == "venice-1778" else _xs(p.n_cams) + _xs(p.n_cams, ctx)[2:]
    _run(ctx, fam, p.obs, "NONE", 1.0, xs, name)
    ctx.close()


@pytest.mark.parametrize("fam", C_FORM)
@pytest.mark.parametrize("robust", ["HUBER", "CAUCHY"])
def test_e0_within_bound_robust(monkeypatch, fam, robust):
    p = _cached("trafalgar-257")
    ctx = _context(monkeypatch, fam, p.n_cams, p.lm_off, p.cam_idx, p.obs, p.cams, robust=robust)
    _run(ctx, fam, p.obs, robust, 1.0, _xs(p.n_cams) + _xs(p.n_cams, ctx)[2:], f"trafalgar-257/{robust}")
    ctx.close()


# ---- the edge graph (rounding_bounds.edge_problem) plus one camera without observations
def _edge():
    n_c, lm_off, cam_idx, obs, cams, lms = RB.edge_problem(0)
    cams = np.concatenate([cams, cams[:1] + 0.5], 0)
    return n_c + 1, lm_off, cam_idx, obs, cams


# The row stream of e0_lpl (povar_kernels_lpl.hpp).  One workgroup: the edge graph's landmarks are at least 65 tiles over 16
# wavefronts, so every wavefront takes later tiles from the counter, its prefetch cursor crosses tile boundaries three rows
# ahead and ends in "no tile left"; K0 = 2 is the shortest tile the stream's invariant allows; 8 accumulators make most
# observations cold, in both addressings of q4c.  (The default grid has more workgroups than tiles: wavefronts and workgroups
# without any tile.)
LPL_STREAM_RUNS = [("e0_lpl", r, {"POVAR_E0_WGS": "1"}, 0) for r in ("NONE", "HUBER")] + \
    [("e0_lpl", "NONE", {"POVAR_E0_WGS": "1", "POVAR_LPL_K0": "2"}, 0)] + \
    [("e0_lpl", "NONE", {"POVAR_HOT_ACC": "8", "POVAR_COLD_Q_ROWS": q}, 0) for q in ("0", "1")]
EDGE_RUNS = [(f, "NONE", {}, 0) for f in C_FORM + PER_OBS] + [(f, "HUBER", {}, 0) for f in C_FORM] + \
    [(f, "NONE", {"POVAR_HOT_ACC": "8"}, 0) for f in CHUNK] + \
    [(f, "NONE", {"POVAR_CK_NB": "3", "POVAR_CK_HMAX": "5"}, 0) for f in CHUNK] + \
    [(f, "HUBER", {"POVAR_CK_NB": "3", "POVAR_CK_HMAX": "5"}, 0) for f in CHUNK] + \
    [(f, "NONE", {}, "FLAG_NO_PACKED_ROWS") for f in ("e0_ck", "e0_ck_f32")] + \
    [("e0_ck_det", r, {"POVAR_E0_WGS": "1", "POVAR_CK_HMAX": "3"}, 0) for r in ("NONE", "HUBER")] + LPL_STREAM_RUNS
# (the two of e0_ck_det: one workgroup and chunks of at most 3 rows -- a batch of more than 16 tiles, so that a wavefront walks a
# SECOND tile and reloads its camera record between the passes and on the way back; every other edge run has 16 per batch)


@pytest.mark.parametrize("fam,robust,env,flag", EDGE_RUNS,
                         ids=[f"{f}-{r}-{'+'.join(f'{k}={v}' for k, v in e.items()) or 'default'}-{fl or 'packed'}" for f, r, e, fl in EDGE_RUNS])
def test_edge_graph_within_bound(monkeypatch, fam, robust, env, flag):
    from povar_amd import capi
    n_c, lm_off, cam_idx, obs, cams = _edge()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = _context(monkeypatch, fam, n_c, lm_off, cam_idx, obs, cams, robust=robust, huber=RB.EDGE_HUBER,
                   flags=getattr(capi, flag) if flag else 0)
    if fam in ("e0_ck", "e0_ck_f32") and not env and not flag:
        li = ctx.layout_info()
        assert li.ck_packed == 1
    if "POVAR_E0_WGS" in env and fam in CHUNK:
        assert ctx.layout_info().ck_tiles_max > 16, "no wavefront has a second tile in a batch"
    if "POVAR_E0_WGS" in env and fam == "e0_lpl":
        assert ctx.layout_info().grid == 1 and len(lm_off) - 1 > 16 * 64, "no wavefront takes a second tile from the counter"
    xs = _xs(n_c) + _xs(n_c, ctx)[2:]
    _run(ctx, fam, obs, robust, RB.EDGE_HUBER, xs, f"edge/{robust}/{env or flag or 'default'}")
    # exact zeros: the camera without observations
    for _, x in xs:
        assert np.all(ctx.right_mul_e0_pose(x)[12 * (n_c - 1):] == 0.0)
    ctx.close()


# ---- term by term: each get_term() against B^-1 E0_ref(the loop's own previous term)
@pytest.mark.parametrize("fam", ["e0_ck", "e0_ck_f32"])
@pytest.mark.parametrize("solver", ["POWER_VARPROJ", "POWER_SCHUR_COMPLEMENT"])
@pytest.mark.parametrize("robust", ["NONE", "HUBER", "CAUCHY"])
def test_terms_and_increment_within_bound(monkeypatch, fam, solver, robust):
    from povar_amd import capi
    p = _cached("p257")
    ctx = _context(monkeypatch, fam, p.n_cams, p.lm_off, p.cam_idx, p.obs, p.cams, robust=robust)
    ctx.prepare_pose(LAM, getattr(capi, solver))
    prob = RB.Step1.from_context(ctx, p.obs, ALPHA, robust, 1.0)
    model = RB.MODELS[FAMILIES[fam][3]]
    binv = ctx.get_buffer(capi.BUF_B_INV).reshape(-1, 12, 12)
    bi = binv.astype(np.longdouble)
    ba = np.abs(binv)
    ctx.power_series_begin()
    terms = [ctx.get_term()]
    worst = 0.0
    for i in range(5):
        ctx.power_series_step()
        t = ctx.get_term()
        y_ref, bound = RB.evaluate(prob, terms[-1], model)
        yr = y_ref.reshape(-1, 12)
        t_ref = np.einsum("cij,cj->ci", bi, yr).reshape(-1)
        ym = np.abs(yr.astype(np.float64))
        tb = (np.einsum("cij,cj->ci", ba, bound.reshape(-1, 12)) + float(RB.gam(13, RB.U64)) * np.einsum("cij,cj->ci", ba, ym)).reshape(-1)
        r, j, n_over = RB.check(t, t_ref, tb)
        print(f"E0BOUND p257/{robust}/{solver} {fam} term={i + 1} err/bound={r:.3g} rel={rel(t, t_ref.astype(np.float64)):.3g}")
        assert n_over == 0, (i + 1, r, j)
        worst = max(worst, r)
        terms.append(t)
    if fam == "e0_ck_f32":
        assert ctx.layout_info().fp32_terms == 1
    inc = ctx.get_increment()
    s = np.sum(terms, axis=0)
    sb = float(RB.gam(len(terms), RB.U64)) * np.sum(np.abs(terms), axis=0)
    assert np.all(np.abs(inc - s) <= sb), np.abs(inc - s).max()
    ctx.close()
