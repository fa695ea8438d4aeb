"""The row walk and the row stream of the camera-chunk kernels (povar_kernels_ck_parts.hpp: ck_walk_rows, CkRowStream) where
they can go wrong: tiles SHORTER than the stream's depth and tiles of odd height.  POVAR_CK_HMAX caps the height of a chunk
tile for both steps' layouts; the heights are chosen against both depths (2: every kernel but variant 2 of e0_ck; 4: variant 2):
  height 1    only the tail of the walk runs, for depth 2 and depth 4 (every request of start() past the first is clamped)
  height 3    one unrolled block and an odd tail for depth 2, the tail alone for depth 4
  height 5    a block and one row for depth 4
  height 16   the shipped shape
on the problem and set-up of test_e0_ck_several_batches_and_cold_chunks (tests/test_gpu_e0_ck.py): several landmark batches per
workgroup, 64 accumulator slots, so chunks with partial records of their own.

Per case what tests/test_gpu_e0_bounds.py / test_gpu_e0h_bounds.py assert -- step 1: E0 x, step 2: each power-series term,
within the componentwise bound of tests/rounding_bounds.py for the family's model, no entry over -- and the 20-term increment
against the oracle at the tolerance the kernel has elsewhere (1e-10: test_gpu_e0_ck.py, test_gpu_step2.py; the fp32 terms:
1e-5, test_gpu_fp32_terms.py)."""
import os

import numpy as np
import pytest

import test_gpu_e0_bounds as S1
import test_gpu_e0h_bounds as S2
from conftest import rel

pytestmark = pytest.mark.gpu
ALPHA, LAM, M = S1.ALPHA, S1.LAM, 20
NT = min(os.cpu_count() or 1, 16)
ENV = {"POVAR_E0_V1": "0", "POVAR_LPL_PLACE": "sync", "POVAR_HOT_ACC": "64", "POVAR_CK_NB": "5"}
HEIGHTS = [1, 3, 5, 16]
# kernel: (step, family of the bounds module, e0_ck variant or None, robust norm, tolerance of the increment)
KERNELS = {
    "e0_ck-v1": (1, "e0_ck", 1, "NONE", 1e-10),         # depth 2
    "e0_ck-v2": (1, "e0_ck", 2, "NONE", 1e-10),         # depth 4
    "e0_ck-v3": (1, "e0_ck", 3, "NONE", 1e-10),         # depth 2, DB: the next tile's rows in a second stream
    "e0_ck-huber": (1, "e0_ck", 1, "HUBER", 1e-10),
    "e0_ck_h": (2, "e0_ck_h", None, "NONE", 1e-10),
    "e0_ck_f32": (1, "e0_ck_f32", None, "NONE", 1e-5),
    "e0_ck_det": (1, "e0_ck_det", None, "NONE", 1e-10),
    "e0_ck_h_det": (2, "e0_ck_h_det", None, "NONE", 1e-10),
}
HUBER1, HUBER2 = 1.0, 0.5

_REF = {}


def _problem():
    from povar_amd import synth
    if "p" not in _REF:
        _REF["p"] = synth.make_problem(300, 20000, 90000, seed=5)
    return _REF["p"]


def _ref_step1(robust):
    """landmarks of the linearisation point and the oracle's 20-term increment (once per norm)"""
    from oracle import povar_oracle as O
    key = ("step1", robust)
    if key not in _REF:
        p = _problem()
        orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=robust, huber=HUBER1)
        lms = orc.init_landmarks_pose(ALPHA, p.cams)
        st, diag2, jls, sigma, ok = orc.stage1_pose(ALPHA, p.cams, lms)
        assert ok
        orc.scale_jp_cols_pose(st, sigma)
        hll, b, binv = orc.prepare_hb_pose(st, LAM)
        ref = orc.solve_pose(st, hll, binv, b, M, n_threads=NT)[0]
        _REF[key] = (lms, ref)
    return _REF[key]


def _ref_step2():
    """the state of tests/test_gpu_step2.py (_state) and the oracle's 20-term increment"""
    from oracle import povar_oracle as O
    if "step2" not in _REF:
        p = _problem()
        rng = np.random.default_rng(11)
        cams = rng.normal(size=(p.n_cams, 12))
        cams[:, 8:11] *= 0.1
        cams[:, 11] = 5 + rng.random(p.n_cams)
        cams /= np.linalg.norm(cams, axis=1, keepdims=True)
        lms_h = np.concatenate([rng.normal(size=(p.n_lms, 3)), np.ones((p.n_lms, 1))], 1)
        obs = p.obs / 500.0
        orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, obs, robust_norm="NONE", huber=HUBER2)
        st_h, ok = orc.linearize_homogeneous(cams, lms_h)
        diag2 = orc.jp_diag2_homogeneous(st_h)
        orc.scale_jl_cols_homogeneous(st_h)
        orc.scale_jp_cols_joint(st_h, 1.0 / (1e-5 + np.sqrt(diag2)))
        st_n = orc.linearize_nullspace(cams, lms_h, st_h)
        hll, b, binv = orc.prepare_hb_joint(st_h, st_n, LAM)
        ref = orc.solve_joint(st_n, hll, binv, b, M)[0]
        _REF["step2"] = (cams, lms_h, obs, ref)
    return _REF["step2"]


@pytest.mark.parametrize("hmax", HEIGHTS)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_short_and_odd_tiles(monkeypatch, kernel, hmax):
    from povar_amd import capi
    step, fam, variant, robust, tol = KERNELS[kernel]
    p = _problem()
    env = dict(ENV, POVAR_CK_HMAX=str(hmax))
    label = f"hmax={hmax}/{kernel}"
    if step == 1:
        lms, ref = _ref_step1(robust)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = S1._context(monkeypatch, fam, p.n_cams, p.lm_off, p.cam_idx, p.obs, p.cams, robust=robust, huber=HUBER1, lms=lms)
        li = ctx.layout_info()
        assert li.ck_ready == 1 and li.ck_batches >= 5 and li.ck_cold_chunks > 0
        assert li.ck_chunks * hmax >= p.n_obs, "the cap on the tile height was not applied"  # (a chunk: <= hmax observations)
        if variant is not None:
            ctx.set_e0_kernel(variant)
            assert ctx.layout_info().e0_kernel == variant
        S1._run(ctx, fam, p.obs, robust, HUBER1, S1._xs(p.n_cams), label)
        inc, it, status, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
        li = ctx.layout_info()
        if fam == "e0_ck_f32":
            assert li.fp32_terms == 1
        else:
            assert li.e0_kernel == (S1.CK_VARIANTS + 1 if fam == "e0_ck_det" else variant)
    else:
        cams, lms_h, obs, ref = _ref_step2()
        ctx = S2._context(monkeypatch, fam, p.n_cams, p.lm_off, p.cam_idx, obs, cams, lms_h, robust, HUBER2, env)
        li = ctx.layout_info()
        assert li.ckh_ready == 1 and li.ckh_batches >= 5
        assert li.ckh_chunks * hmax >= p.n_obs, "the cap on the tile height was not applied"
        S2._terms_within_bound(ctx, fam, obs, robust, HUBER2, label)
        inc, it, status, rc = ctx.solve_joint(LAM, M)
        S2._ran(ctx, fam)
    r = rel(inc, ref)
    print(f"CKROWS {label} increment rel={r:.3g} (tolerance {tol:g})")
    assert rc == 0 and it == M
    assert r < tol, (label, r)
    ctx.close()
