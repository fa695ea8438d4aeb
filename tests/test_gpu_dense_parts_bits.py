"""The dense-factor path is reproducible to the bit on an input where its one unordered sum is order-free: two fresh
contexts, both steps, NONE and HUBER, every buffer of the direct solve and of the covariance calls byte for byte.

The assembly (sc_dense_offdiag[_h], sc_dense_diag) adds into S with atomics, in no defined order.  Three landmarks with
pairwise disjoint camera sets take the order out by construction: an entry of S receives at most two addends, B_c and one
landmark's term, and a sum of two terms commutes.  Everything behind the assembly -- factorisation, substitution, the
triangular inverse, W W^T, the per-landmark and per-observation contractions -- sums in a fixed order.  Tracks of 65, 33 and 6
cameras (104 cameras): both chunk loops of both steps' stagings repeat (chunks of 64 and 32), N = 1 280 / 1 152 rows, so the
256-row outer update runs, cov_lauum takes ten or more K steps and camera blocks straddle 64-edges.  Damped gauge: the free
gauge rightly fails on a block-diagonal system.

This guards refactors of povar_kernels_sc.hpp / _chol.hpp / _cov.hpp, povar_sc.hip and povar_cov.hip: profiles/dense_parts_bits.txt compares
the same buffers between two builds of the library."""
import numpy as np
import pytest

import landmark_covariance_reference as L

TRACKS = (65, 33, 6)
LAMBDA = 1e-2
SEED = 5


def dense_parts_problem():
    """104 cameras, three landmarks; landmark l sees the cameras of its own range only (ascending).  A subgraph of the
    generator's complete graph, so the image points are the generator's own projections."""
    from povar_amd import synth
    n_c, n_l = sum(TRACKS), len(TRACKS)
    full = synth.make_problem(n_c, n_l, n_c * n_l, seed=SEED, popularity="uniform")
    assert np.all(np.diff(full.lm_off) == n_c)
    first = np.concatenate([[0], np.cumsum(TRACKS)])
    keep = np.concatenate([n_c * l + np.arange(first[l], first[l + 1]) for l in range(n_l)])
    assert np.array_equal(full.cam_idx[keep], np.arange(n_c))
    return synth.Problem(n_c, n_l, first.astype(np.int32), np.ascontiguousarray(full.cam_idx[keep]),
                         np.ascontiguousarray(full.obs[keep]), full.cams, full.lms)


def dense_parts_buffers(p, step, norm):
    """{name: array} of a fresh deterministic context: the direct solve, then the landmark call in both coordinate systems
    (camera blocks with it) and the observation call, damped."""
    from povar_amd import capi
    joint = step == 2
    cams, lms, obs = L.state(p, step)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, obs, robust_norm=norm, huber=L.HUBER[step], flags=capi.FLAG_DETERMINISTIC)
    out = {}
    try:
        ctx.set_cameras(cams)
        if joint:
            ctx.set_landmarks_homogeneous(lms)
            assert ctx.linearize_homogeneous()
            inc, _, _, rc = ctx.solve_joint_sc(LAMBDA, method=capi.SC_CHOLESKY)
        else:
            ctx.set_landmarks(lms)
            assert ctx.linearize_pose(L.ALPHA)
            inc, _, _, rc = ctx.solve_pose_sc(LAMBDA, method=capi.SC_CHOLESKY)
        assert rc == 0
        out["increment"] = inc
        out["SC_FACTOR"] = ctx.get_buffer(capi.BUF_SC_FACTOR, joint=joint)
        ctx.set_cov_inspect(True)
        for coords, tag in ((capi.COV_LANDMARK_COORDS, "own"), (capi.COV_SOLVER_COORDS, "solver")):
            lm, cam, rc = ctx.landmark_covariance(step=step, lam=LAMBDA, gauge=capi.COV_DAMPED, coords=coords, with_cameras=True)
            assert rc == 0
            out["landmark_blocks_" + tag], out["camera_blocks_" + tag] = lm, cam
        for which in ("COV_FACTOR", "COV_INVERSE", "COV_PANEL"):
            out[which] = ctx.get_buffer(getattr(capi, "BUF_" + which), joint=joint)
        rows, rc = ctx.observation_covariance(step=step, lam=LAMBDA, gauge=capi.COV_DAMPED)
        assert rc == 0
        out["observation_rows"] = rows
    finally:
        ctx.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["NONE", "HUBER"])
@pytest.mark.parametrize("step", [1, 2])
def test_dense_path_is_bit_reproducible_on_disjoint_tracks(step, norm):
    p = dense_parts_problem()
    a, b = dense_parts_buffers(p, step, norm), dense_parts_buffers(p, step, norm)
    assert a["SC_FACTOR"].shape[0] == (1280 if step == 1 else 1152)
    for name in a:
        assert np.all(np.isfinite(a[name])), name
        assert a[name].tobytes() == b[name].tobytes(), f"step {step} {norm}: {name} differs between two contexts"
