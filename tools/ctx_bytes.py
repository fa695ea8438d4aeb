"""What povar_device_bytes reports over a context's life, and the bits of a deterministic context's solves: the A/B of a change
that may move neither (run it with POVAR_LIB on two builds of the library; the outputs are compared line for line --
profiles/ctx_ownership_bytes.txt).
usage: [POVAR_LIB=<library>] python3 tools/ctx_bytes.py"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from povar_amd import capi, synth  # noqa: E402

ALPHA, LAM, M = 0.01, 1e-4, 20


def start(ctx, p):
    ctx.set_cameras(p.cams)
    ctx.init_landmarks_pose(ALPHA)
    assert ctx.linearize_pose(ALPHA)


def to_step2(ctx, p):
    lms = ctx.get_landmarks()
    ctx.set_landmarks_homogeneous(np.concatenate([lms, np.ones((p.n_lms, 1))], axis=1))
    ctx.normalize_joint()
    assert ctx.linearize_homogeneous()


def life(tag, p, env, covariance):
    for k in ("POVAR_LPL_PLACE", "POVAR_E0_V1"):
        os.environ.pop(k, None)
    os.environ.update(env)
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, e0_mode=capi.E0_IMPLICIT_LDSACC)
    say = lambda what: print(f"{tag}: device_bytes after {what}: {ctx.device_bytes()}", flush=True)  # noqa: E731
    say("create")
    start(ctx, p)
    assert ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)[3] == 0
    say("the first solve")
    ctx.layout_finalize(wait=True)
    say(f"layout_finalize(wait=True), placement {ctx.layout_info().placement}")
    assert ctx.linearize_pose(ALPHA)
    assert ctx.solve_pose_sc(LAM, capi.SC_CHOLESKY)[3] == 0
    say("CHOLESKY")
    if covariance:
        assert ctx.camera_covariance(step=1, lam=LAM, gauge=capi.COV_DAMPED)[1] == 0
        say("camera_covariance")
        assert ctx.landmark_covariance(step=1, lam=LAM, gauge=capi.COV_DAMPED)[1] == 0
        say("landmark_covariance")
        assert ctx.observation_covariance(step=1, lam=LAM, gauge=capi.COV_DAMPED)[1] == 0
        say("observation_covariance")
    to_step2(ctx, p)
    assert ctx.solve_joint_sc(LAM, method=capi.SC_CHOLESKY)[3] == 0
    say("RICHOLESKY")
    ctx.comm_init_host(1, 0, lambda buf: None)
    for attempt in ("", " again"):
        handle = ctx.p2p_export(1)
        say("p2p_export" + attempt)
        ctx.p2p_attach(1, 0, [handle])
        say("p2p_attach" + attempt)
    ctx.close()


def bits(p):
    ctx = capi.Context(p.n_cams, p.lm_off, p.cam_idx, p.obs, e0_mode=capi.E0_IMPLICIT_LDSACC, flags=capi.FLAG_DETERMINISTIC)
    print(f"deterministic: device_bytes after create: {ctx.device_bytes()}")
    start(ctx, p)
    inc, _, _, rc = ctx.solve_pose(LAM, capi.POWER_VARPROJ, M)
    assert rc == 0
    print(f"deterministic: sha256 of the step-1 increment: {hashlib.sha256(inc.tobytes()).hexdigest()}")
    to_step2(ctx, p)
    inc, _, _, rc = ctx.solve_joint(LAM, M)
    assert rc == 0
    print(f"deterministic: sha256 of the step-2 increment: {hashlib.sha256(inc.tobytes()).hexdigest()}")
    print(f"deterministic: device_bytes after both solves: {ctx.device_bytes()}")
    ctx.close()


if __name__ == "__main__":
    big = synth.make_problem(300, 60000, 300000, seed=4)
    small = synth.make_problem(29, 400, 2400, seed=11, popularity="uniform")
    life("300 cameras, rows placed on a host thread", big, {"POVAR_LPL_PLACE": "async", "POVAR_E0_V1": "0"}, covariance=False)
    life("300 cameras, rows placed in povar_create", big, {"POVAR_LPL_PLACE": "sync", "POVAR_E0_V1": "0"}, covariance=False)
    life("29 cameras", small, {}, covariance=True)
    bits(big)
