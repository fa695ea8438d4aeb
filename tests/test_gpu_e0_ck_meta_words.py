"""e0_ck / e0_ck_h carry a lane's metadata (CkP::lane_meta) across their workgroup barriers as the raw words and decode them
where rank, run and accumulator slot are first read (povar_kernels_ck.hpp: request_first_meta).  The arithmetic is untouched;
what changed hands is which value is alive where -- so the cases are the ones in which those words differ from lane to lane
and from tile to tile: many landmark batches (the next batch's words requested behind a barrier of this one), wavefronts
with a second and third tile (the words of the tile before on the way back), chunks with records of their own
(accumulator word < 0), empty lanes (word < 0), a single batch (the words are preset, never loaded) and wavefronts without
a first tile.

Every e0_ck instantiation against e0_lpl of the SAME context (tests/test_gpu_e0_ck.py holds that kernel to the oracle), with
that file's tolerances: E0 x 1e-12, the 20-term increment 1e-10, relative 2-norms.  Small problems: a second or two each.
"""
import numpy as np
import pytest

from conftest import rel

pytestmark = pytest.mark.gpu
ALPHA, LAM, M = 0.01, 1e-4, 20
N_VARIANTS = 6
KNOBS = ("POVAR_E0_V1", "POVAR_HOT_ACC", "POVAR_CK_NB", "POVAR_LPL_PLACE", "POVAR_CK_PACK", "POVAR_CKH_STRIDE", "POVAR_CKH_ACC_CAP",
         "POVAR_E0_WGS", "POVAR_LPL_K0", "POVAR_LPL_STRATEGY", "POVAR_E0_CK", "POVAR_NO_CK")


def _env(monkeypatch, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, v)


def _step1_context(p, robust):
    from povar_amd import capi
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, robust_norm=robust, e0_mode=capi.E0_IMPLICIT_LDSACC)
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(ALPHA)
    assert ctx.linearize_pose(ALPHA)
    ctx.prepare_pose(LAM)
    return ctx


def _every_kernel_against_e0_lpl(ctx, n_cams, seed, kernels=range(1, N_VARIANTS + 1)):
    from povar_amd import capi
    x = np.random.default_rng(seed).normal(size=12 * n_cams)
    ctx.set_e0_kernel(0)
    assert ctx.layout_info().e0_kernel == 0
    y0 = ctx.right_mul_e0_pose(x)
    inc0, it0, st0, rc0 = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
    assert rc0 == 0
    for kernel in kernels:
        ctx.set_e0_kernel(kernel)
        assert ctx.layout_info().e0_kernel == kernel  # (the kernel that runs, not the one asked for)
        e_x = rel(ctx.right_mul_e0_pose(x), y0)
        inc, it, st, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
        e_inc = rel(inc, inc0)
        print(f"kernel {kernel}: E0 x {e_x:.3e}, increment {e_inc:.3e}")
        assert e_x < 1e-12, kernel
        assert rc == 0 and (it, st) == (it0, st0) and e_inc < 1e-10, kernel


@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
@pytest.mark.parametrize("pack", ["1", "0"])
def test_many_batches_later_tiles_own_records_and_empty_lanes(pack, robust, monkeypatch):
    """Six landmark batches per workgroup and 64 accumulator slots: every batch but the last requests the next one's words
    behind its second barrier, wavefronts walk a second and a third tile, chunks of cameras without a slot carry the
    complement of their record in the accumulator word, short tiles have empty lanes."""
    from povar_amd import synth
    _env(monkeypatch, POVAR_E0_V1="0", POVAR_HOT_ACC="64", POVAR_CK_NB="6", POVAR_LPL_PLACE="sync", POVAR_CK_PACK=pack)
    p = synth.make_problem(300, 20000, 90000, seed=13)
    ctx = _step1_context(p, robust)
    li = ctx.layout_info()
    assert li.ck_ready == 1 and li.ck_batches >= 6 and li.ck_cold_chunks > 0
    _every_kernel_against_e0_lpl(ctx, p.n_cams, 3)
    ctx.close()


@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
@pytest.mark.parametrize("nb,kernels", [(1, (1, 2, 3, 6)), (2, (4, 5))])
def test_one_batch_takes_the_preset_words(nb, kernels, robust, monkeypatch):
    """One landmark batch per workgroup: there is no next batch, the words of a next batch are the preset ones.  The
    instantiations whose wavefronts work as two groups (4 and 5: povar_ctx.hpp) run an even number of batches only -- with one
    batch the library plans e0_lpl for them --: two batches are one batch per group, no next batch for either."""
    from povar_amd import synth
    _env(monkeypatch, POVAR_E0_V1="0", POVAR_HOT_ACC="64", POVAR_CK_NB=str(nb), POVAR_LPL_PLACE="sync")
    p = synth.make_problem(300, 20000, 90000, seed=13)
    ctx = _step1_context(p, robust)
    li = ctx.layout_info()
    assert li.ck_ready == 1 and li.ck_batches == nb
    _every_kernel_against_e0_lpl(ctx, p.n_cams, 4, kernels)
    ctx.close()


@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
@pytest.mark.parametrize("nb,kernels", [(None, (1, 2, 3, 6)), (2, (4, 5))])
def test_fewer_chunk_tiles_than_wavefronts(nb, kernels, robust, monkeypatch):
    """A problem with fewer chunk tiles per batch than the workgroup has wavefronts: wavefronts whose first tile does not exist
    (the first-request table says so at entry, the tile range for the later batches), at the default batch count -- one batch;
    the two-group instantiations at two, as above."""
    from povar_amd import synth
    _env(monkeypatch, POVAR_E0_V1="0", POVAR_LPL_PLACE="sync", **({"POVAR_CK_NB": str(nb)} if nb else {}))
    p = synth.make_problem(40, 3000, 12000, seed=5)
    ctx = _step1_context(p, robust)
    li = ctx.layout_info()
    assert li.ck_ready == 1 and li.ck_batches == (nb or 1)
    assert li.ck_tiles_max < 8  # fewer tiles in a batch than the smallest workgroup (or group) has wavefronts
    print("batches", li.ck_batches, "tiles at most", li.ck_tiles_max, "chunks", li.ck_chunks)
    _every_kernel_against_e0_lpl(ctx, p.n_cams, 5, kernels)
    ctx.close()


@pytest.mark.parametrize("robust", ["NONE", "HUBER"])
def test_step2_many_batches_against_e0_lpl_h(robust, monkeypatch):
    """The step-2 twin of the many-batch case: e0_ck_h against e0_lpl_h of the same context -- the first term and the 20-term
    increment (built like the step-2 case of tests/test_gpu_e0_ck.py)."""
    from povar_amd import capi, synth
    _env(monkeypatch, POVAR_E0_V1="0", POVAR_HOT_ACC="64", POVAR_CK_NB="6", POVAR_LPL_PLACE="sync")
    p = synth.make_problem(300, 20000, 90000, seed=13)
    rng = np.random.default_rng(11)
    cams = rng.normal(size=(p.n_cams, 12))
    cams[:, 8:11] *= 0.1
    cams[:, 11] = 5 + rng.random(p.n_cams)
    cams /= np.linalg.norm(cams, axis=1, keepdims=True)
    lms_h = np.concatenate([rng.normal(size=(p.n_lms, 3)), np.ones((p.n_lms, 1))], 1)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs / 500.0, robust_norm=robust, huber=0.5, e0_mode=capi.E0_IMPLICIT_LDSACC)
    li = ctx.layout_info()
    assert li.ckh_ready == 1 and li.ckh_batches >= 6 and li.ckh_cold_chunks > 0
    ctx.set_cameras(cams)
    ctx.set_landmarks_homogeneous(lms_h)
    assert ctx.linearize_homogeneous()
    ctx.prepare_joint(LAM)
    res = {}
    for kernel in (0, 1):
        ctx.set_e0_kernel(kernel)
        assert ctx.layout_info().e0_kernel_h == kernel
        ctx.power_series_begin()
        ctx.power_series_step()
        t1 = ctx.get_term(11).copy()
        inc, it, st, rc = ctx.solve_joint(LAM, M)
        assert rc == 0 and it == M
        res[kernel] = (t1, inc)
    e_t, e_inc = rel(res[1][0], res[0][0]), rel(res[1][1], res[0][1])
    print(f"first term {e_t:.3e}, increment {e_inc:.3e}")
    assert e_t < 1e-12 and e_inc < 1e-10
    ctx.close()
