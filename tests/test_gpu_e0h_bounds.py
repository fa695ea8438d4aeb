"""Every step-2 (RIPOBA) E0 family held to the componentwise rounding-error bound of tests/rounding_bounds.py: each of the
11 n_cams entries of each power-series term satisfies |t_dev - t_ref| <= bound, with the long-double reference
B^-1 N_c^T sigma E0 sigma N_c applied to the device's OWN previous term and the bound built from the context's own operands
(cameras, homogeneous landmarks, BUF_POSE_SCALING, BUF_JL_COL_SCALE_H, BUF_HLL_INV, BUF_NC_HOUSEHOLDER, BUF_B_INV_JOINT).
The relative 2-norms of the other step-2 modules are dominated by the hub cameras; this checks a one-observation camera's
block as hard as a hub's, through either camera tail (cam_cold_sum_binv_h, or cam_cold_sum + cam_binv_axpy_h under
POVAR_NO_FUSE=1).

Families: lm_regular / lm_long<OpE0H> (lm_h), e0_lm_cached_h, e0_lpl_h (the per-observation Jl3 model), e0_ck_h at either
stride and e0_ck_h_det (the ambient U4 model, the latter with the fixed-point grid).  Each case forces its kernel itself
(environment, E0 mode, set_e0_kernel) and checks through layout_info() that it ran.  Under POVAR_DETERMINISTIC=1 in the
environment (tools/forced_mode_suite.sh) the cases of the other kernels skip.
"""
import os

import numpy as np
import pytest

import rounding_bounds as RB
from conftest import rel

pytestmark = pytest.mark.gpu
LAM, TERMS = 1e-4, 5
DET_ENV = os.environ.get("POVAR_DETERMINISTIC") == "1"
_LAYOUT_OVERRIDES = ("POVAR_CKH_ACC_CAP", "POVAR_CKH_STRIDE", "POVAR_HOT_ACC", "POVAR_CK_NB", "POVAR_LPL_K0", "POVAR_LPL_STRATEGY",
                     "POVAR_E0_WGS", "POVAR_E0_CK")

# family: (environment, e0 mode, set_e0_kernel or None, e0_kernel_h expected or None, lane_per_landmark, model)
FAMILIES = {
    "lm_h": ({"POVAR_E0_V1": "1"}, "E0_IMPLICIT", None, None, 0, "jl3"),
    "lm_cached_h": ({"POVAR_E0_V1": "1"}, "E0_IMPLICIT_LDSACC", None, None, 0, "jl3"),
    "e0_lpl_h": ({"POVAR_E0_V1": "0", "POVAR_LPL_PLACE": "sync"}, "E0_IMPLICIT_LDSACC", 0, 0, 1, "jl3"),
    "e0_ck_h": ({"POVAR_E0_V1": "0", "POVAR_E0_CK": "1", "POVAR_LPL_PLACE": "sync"}, "E0_IMPLICIT_LDSACC", None, 1, 1, "ckh"),
    "e0_ck_h_det": ({"POVAR_E0_V1": "0", "POVAR_LPL_PLACE": "sync", "POVAR_DETERMINISTIC": "1"}, "E0_IMPLICIT_LDSACC", None, 2, 1, "ckh_det"),
}
ALL = list(FAMILIES)
CHUNK = ["e0_ck_h", "e0_ck_h_det"]


def _context(monkeypatch, fam, n_cams, lm_off, cam_idx, obs, cams, lms_h, robust, huber, env=None):
    """A prepared joint system with the family's kernel forced."""
    from povar_amd import capi
    fenv, mode, kernel, kernel_h, lpl, _ = FAMILIES[fam]
    if DET_ENV and fam != "e0_ck_h_det":
        pytest.skip("POVAR_DETERMINISTIC=1 in the environment pins the kernel of this case")
    for k in _LAYOUT_OVERRIDES:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**fenv, **(env or {})}.items():
        monkeypatch.setenv(k, v)
    ctx = capi.Context(n_cams, lm_off, cam_idx, obs, robust_norm=robust, huber=huber, e0_mode=getattr(capi, mode))
    ctx.layout_finalize(True)
    ctx.set_cameras(cams)
    ctx.set_landmarks_homogeneous(lms_h)
    assert ctx.linearize_homogeneous()
    ctx.prepare_joint(LAM)
    if kernel is not None:
        ctx.set_e0_kernel(kernel)
    return ctx


def _ran(ctx, fam):
    li = ctx.layout_info()
    _, _, _, kernel_h, lpl, _ = FAMILIES[fam]
    assert li.lane_per_landmark == lpl, (fam, li.lane_per_landmark)
    if kernel_h is not None:
        assert li.e0_kernel_h == kernel_h, (fam, li.e0_kernel_h)
    return li


def _terms_within_bound(ctx, fam, obs, robust, huber, label, unobserved=()):
    """power_series_begin, TERMS steps: every entry of every term within its bound of the reference applied to the device's
    previous term; then the increment against the sum of the terms.  Returns the worst err / bound."""
    prob = RB.Step2.from_context(ctx, obs, robust, huber)
    model = RB.MODELS_H[FAMILIES[fam][5]]
    ctx.power_series_begin()
    terms = [ctx.get_term(11)]
    worst = 0.0
    for i in range(TERMS):
        ctx.power_series_step()
        t = ctx.get_term(11)
        _ran(ctx, fam)
        t_ref, bound = RB.evaluate_joint(prob, terms[-1], model)
        r, j, n_over = RB.check(t, t_ref, bound)
        print(f"E0HBOUND {label} {fam} term={i + 1} err/bound={r:.3g} rel={rel(t, t_ref.astype(np.float64)):.3g} over={n_over}")
        assert np.all(np.isfinite(t))
        assert n_over == 0, (i + 1, r, j // 11, j % 11, float(t[j]), float(t_ref[j]), float(bound[j]))
        for c in unobserved:
            assert np.all(t[11 * c:11 * c + 11] == 0.0)
        worst = max(worst, r)
        terms.append(t)
    inc = ctx.get_increment(11)
    s = np.sum(terms, axis=0)
    sb = float(RB.gam(len(terms), RB.U64)) * np.sum(np.abs(terms), axis=0)
    assert np.all(np.abs(inc - s) <= sb), np.abs(inc - s).max()
    return worst


# ---- the edge graph (rounding_bounds.edge_problem_joint): 151 cameras, one of them without observations
_EDGE = []


def _edge():
    if not _EDGE:
        _EDGE.append(RB.edge_problem_joint(0))
    return _EDGE[0]


# The row stream of e0_lpl_h (povar_kernels_lpl.hpp), as in tests/test_gpu_e0_bounds.py: one workgroup (at least 65 tiles over
# 16 wavefronts: later tiles from the counter, the prefetch cursor across tile boundaries and into "no tile left"), the shortest
# tile the stream allows (K0 = 2), and mostly cold observations in both addressings of q4c
LPL_STREAM_RUNS = [("e0_lpl_h", r, {"POVAR_E0_WGS": "1"}) for r in ("NONE", "HUBER")] + \
    [("e0_lpl_h", "NONE", {"POVAR_E0_WGS": "1", "POVAR_LPL_K0": "2"})] + \
    [("e0_lpl_h", "NONE", {"POVAR_HOT_ACC": "8", "POVAR_COLD_Q_ROWS": q}) for q in ("0", "1")]
EDGE_RUNS = [(f, "NONE", {}) for f in ALL] + [(f, r, {}) for r in ("HUBER", "CAUCHY") for f in ALL] + \
    [(f, "NONE", e) for e in ({"POVAR_HOT_ACC": "8"}, {"POVAR_CK_NB": "3"}) for f in CHUNK] + \
    [(f, "NONE", {"POVAR_NO_FUSE": "1"}) for f in ("e0_ck_h", "e0_lpl_h")] + \
    [("e0_ck_h_det", r, {"POVAR_E0_WGS": "1", "POVAR_CK_HMAX": "3"}) for r in ("NONE", "HUBER")] + LPL_STREAM_RUNS
# (the two of e0_ck_h_det: one workgroup and chunks of at most 3 rows -- more than 16 tiles in a batch, so that a wavefront walks a
# SECOND tile and reloads its camera record between the passes and on the way back; every other edge run has 16 per batch)


@pytest.mark.parametrize("fam,robust,env", EDGE_RUNS,
                         ids=[f"{f}-{r}-{'+'.join(f'{k}={v}' for k, v in e.items()) or 'default'}" for f, r, e in EDGE_RUNS])
def test_edge_graph_terms_within_bound(monkeypatch, fam, robust, env):
    n_c, lm_off, cam_idx, obs, cams, lms_h = _edge()
    ctx = _context(monkeypatch, fam, n_c, lm_off, cam_idx, obs, cams, lms_h, robust, RB.EDGE_HUBER_H, env)
    if "POVAR_E0_WGS" in env and fam == "e0_lpl_h":
        assert ctx.layout_info().grid == 1 and len(lm_off) - 1 > 16 * 64, "no wavefront takes a second tile from the counter"
    if "POVAR_E0_WGS" in env and fam in CHUNK:
        li = ctx.layout_info()
        assert li.ckh_chunks > 64 * 16 * li.ckh_batches * li.grid, "no wavefront has a second tile in a batch"
    _terms_within_bound(ctx, fam, obs, robust, RB.EDGE_HUBER_H, f"edge/{robust}/{'+'.join(f'{k}={v}' for k, v in env.items()) or 'default'}", unobserved=[n_c - 1])
    ctx.close()


# ---- problems of the other step-2 modules, with their state (tests/test_gpu_step2.py: _state)
_CACHE = {}


def _synth(name):
    from povar_amd import synth
    if name not in _CACHE:
        _CACHE.clear()
        p = synth.make_problem(257, 12000, 60000, seed=4) if name == "p257" else synth.make_problem(700, 20000, 90000, seed=6)
        rng = np.random.default_rng(11)
        cams = rng.normal(size=(p.n_cams, 12))
        cams[:, 8:11] *= 0.1
        cams[:, 11] = 5 + rng.random(p.n_cams)
        cams /= np.linalg.norm(cams, axis=1, keepdims=True)
        lms_h = np.concatenate([rng.normal(size=(p.n_lms, 3)), np.ones((p.n_lms, 1))], 1)
        _CACHE[name] = (p, cams, lms_h, p.obs / 500.0)
    return _CACHE[name]


@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
@pytest.mark.parametrize("fam", ["e0_lpl_h", "e0_ck_h", "e0_ck_h_det"])
def test_mid_size_terms_within_bound(monkeypatch, fam, robust):
    p, cams, lms_h, obs = _synth("p257")
    ctx = _context(monkeypatch, fam, p.n_cams, p.lm_off, p.cam_idx, obs, cams, lms_h, robust, 0.5)
    _terms_within_bound(ctx, fam, obs, robust, 0.5, f"p257/{robust}")
    ctx.close()


@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
@pytest.mark.parametrize("stride", [None, "1536", "2048"])
def test_wide_stride_capped_accumulators_terms_within_bound(monkeypatch, stride, robust):
    """700 cameras over 12 workgroups: the library takes the 2048-slot stride by itself, 314 accumulators fit beside it, and
    the chunks of the other cameras get records of their own (ck_layout.hpp: CkShape::wide_slots) -- those records are what
    the wide runs check."""
    p, cams, lms_h, obs = _synth("p700")
    env = {"POVAR_E0_WGS": "12"}
    if stride:
        env["POVAR_CKH_STRIDE"] = stride
    ctx = _context(monkeypatch, "e0_ck_h", p.n_cams, p.lm_off, p.cam_idx, obs, cams, lms_h, robust, 0.5, env)
    li = _ran(ctx, "e0_ck_h")
    assert li.ckh_ready == 1 and li.ckh_stride == int(stride or 2048)
    if li.ckh_stride == 2048:
        assert li.ckh_accumulators == 314 < li.lds_slots and li.ckh_capped_obs > 0
    else:
        assert li.ckh_accumulators == li.lds_slots and li.ckh_capped_obs == 0
    _terms_within_bound(ctx, "e0_ck_h", obs, robust, 0.5, f"p700/{robust}/stride={stride or 'auto'}")
    ctx.close()
