"""e0_ck requests the first tile of a landmark batch (camera record gathers, header, first rows) while the wavefront ends the
batch before, and the first batch's before the LDS set-up (povar_kernels_ck.hpp: request_first_meta / request_first_tile).
Those values cross the batch loop's back edge and a workgroup barrier: held here against the oracle at venice size and at
trafalgar, with packed and with 16-byte rows, and against e0_lpl where a workgroup walks many batches of every size.

Tolerances as tests/test_gpu_e0_ck.py: E0 x 1e-12, 20-term increment 1e-10, relative 2-norms.
"""
import os

import numpy as np
import pytest

from conftest import rel

pytestmark = pytest.mark.gpu
ALPHA, LAM, M = 0.01, 1e-4, 20
NT = min(os.cpu_count() or 1, 16)


@pytest.mark.parametrize("pack", ["1", "0"])
@pytest.mark.parametrize("name", ["trafalgar-257", "venice-1778"])
def test_e0_ck_first_tile_ahead_against_the_oracle(name, pack, monkeypatch):
    """E0 x and the 20-term increment of the shipped instantiation (1) and of the two-group one (4) against the oracle."""
    from povar_amd import capi, synth
    from oracle import povar_oracle as O
    monkeypatch.setenv("POVAR_CK_PACK", pack)
    p = synth.make_bal_problem(name)
    orc = O.Oracle(p.n_cams, p.lm_off, p.cam_idx, p.obs)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, e0_mode=capi.E0_IMPLICIT_LDSACC)
    ctx.layout_finalize(True)
    li = ctx.layout_info()
    assert li.ck_ready == 1 and li.ck_batches >= 1 and li.ck_packed == (1 if pack == "1" else 0)
    lms = orc.init_landmarks_pose(ALPHA, p.cams)
    ctx.set_cameras(p.cams)
    ctx.set_landmarks(lms)
    assert ctx.linearize_pose(ALPHA)
    st, diag2, jls, sigma, ok = orc.stage1_pose(ALPHA, p.cams, lms)
    assert ok
    orc.scale_jp_cols_pose(st, sigma)
    hll, b, binv = orc.prepare_hb_pose(st, LAM)
    ctx.prepare_pose(LAM)
    x = np.random.default_rng(11).normal(size=12 * p.n_cams)
    e0_ref = orc.right_mul_e0_pose(st, hll, x, n_threads=NT)
    ref, it, status, _ = orc.solve_pose(st, hll, binv, b, M, n_threads=NT)
    for kernel in (1, 4):
        ctx.set_e0_kernel(kernel)
        if ctx.layout_info().e0_kernel != kernel:  # (4 needs an even batch count: the layout's, not this kernel's, choice)
            assert kernel != 1
            continue
        assert rel(ctx.right_mul_e0_pose(x), e0_ref) < 1e-12, kernel
        inc, it2, st2, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
        assert rc == 0 and (it2, st2) == (it, status) and rel(inc, ref) < 1e-10, kernel
    del st
    ctx.close()


@pytest.mark.parametrize("pack", ["1", "0"])
def test_e0_ck_first_tile_ahead_over_many_batches(pack, monkeypatch):
    """Six landmark batches per workgroup (POVAR_CK_NB=6), 64 accumulator slots (cold chunks), every instantiation: the first
    tile of batch b + 1 is requested in batch b.  Same E0 x and increment as e0_lpl, which test_gpu_e0_ck.py holds against the
    oracle.  (The table of the first batch's requests, wavefronts without a tile included, is checked on the host:
    test_ck_first_table.py.)"""
    from povar_amd import capi, synth
    monkeypatch.setenv("POVAR_E0_V1", "0")
    monkeypatch.setenv("POVAR_HOT_ACC", "64")
    monkeypatch.setenv("POVAR_CK_NB", "6")
    monkeypatch.setenv("POVAR_LPL_PLACE", "sync")
    monkeypatch.setenv("POVAR_CK_PACK", pack)
    p = synth.make_problem(300, 20000, 90000, seed=13)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, e0_mode=capi.E0_IMPLICIT_LDSACC)
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(ALPHA)
    assert ctx.linearize_pose(ALPHA)
    ctx.prepare_pose(LAM)
    li = ctx.layout_info()
    assert li.ck_ready == 1 and li.ck_batches >= 6 and li.ck_cold_chunks > 0
    x = np.random.default_rng(17).normal(size=12 * p.n_cams)
    ctx.set_e0_kernel(0)
    y0 = ctx.right_mul_e0_pose(x)
    inc0 = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)[0]
    for kernel in range(1, 7):
        ctx.set_e0_kernel(kernel)
        assert ctx.layout_info().e0_kernel == kernel
        assert rel(ctx.right_mul_e0_pose(x), y0) < 1e-12, kernel
        assert rel(ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)[0], inc0) < 1e-10, kernel
    ctx.close()
