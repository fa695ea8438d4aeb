#!/usr/bin/env python3
"""How is the work of the ordered dense assembly (sc_dense_ordered, povar_kernels_sc.hpp) spread over its workgroups?  Counts,
on the host and from the graph alone, the kernel's own loops on a synthetic BAL shape: camera pairs (i <= j) of every landmark,
the 256-observation walk steps of every (row camera, 32-camera tile) workgroup and its windows of at most 32 staged pairs -- the
figures behind "where the ordered time goes" (profiles/sc_ordered_times.txt).  No GPU needed.
usage: sc_ordered_count.py [shape]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from povar_amd import synth  # noqa: E402

T, WALK, PAIRS = 32, 256, 32  # SCO_T, SCO_WALK, SCO_PAIRS


def main():
    p = synth.make_bal_problem(sys.argv[1] if len(sys.argv) > 1 else "venice-1778")
    off, cam = p.lm_off.astype(np.int64), p.cam_idx.astype(np.int64)
    n_obs, k = cam.size, np.diff(off)
    # position of every observation inside its camera's camera-major run (a stable sort by camera, as build_layout_b's)
    order = np.argsort(cam, kind="stable")
    start = np.r_[0, np.cumsum(np.bincount(cam, minlength=p.n_cams))]
    pos = np.empty(n_obs, np.int64)
    pos[order] = np.arange(n_obs) - start[cam[order]]
    # the pairs of every observation: itself and the later observations of its landmark (cameras ascend inside a landmark)
    cnt = off[np.repeat(np.arange(k.size), k) + 1] - np.arange(n_obs)
    own = np.repeat(np.arange(n_obs), cnt)
    par = own + np.arange(own.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    nt = (p.n_cams + T - 1) // T
    max_steps = int(np.bincount(cam).max()) // WALK + 1
    key = (cam[own] * nt + cam[par] // T) * max_steps + pos[own] // WALK  # (workgroup, walk step)
    uk, c = np.unique(key, return_counts=True)
    win = (c + PAIRS - 1) // PAIRS
    wg_u, inv = np.unique(uk // max_steps, return_inverse=True)
    wins, prs = np.bincount(inv, weights=win), np.bincount(inv, weights=c)
    n_c = np.bincount(cam, minlength=p.n_cams)
    steps = np.ceil(n_c[wg_u // nt] / WALK)
    all_steps = sum(int(np.ceil(n_c[ci] / WALK)) * (nt - ci // T) for ci in range(p.n_cams))
    print(f"pairs {own.size}, windows {int(win.sum())} ({own.size / win.sum():.1f} pairs per window), walk steps {all_steps}, "
          f"workgroups with pairs {wg_u.size}")
    print(f"observations per camera: max {n_c.max()}, median {np.median(n_c):.0f}")
    print(f"mean workgroup: {steps.mean():.1f} walk steps, {wins.mean():.1f} windows")
    for t in np.argsort(-wins)[:8]:
        print(f"  camera {wg_u[t] // nt} tile {wg_u[t] % nt}: {int(steps[t])} walk steps, {int(wins[t])} windows, {int(prs[t])} pairs")
    print(f"windows per resident workgroup if balanced over 768: {win.sum() / 768:.0f}")


if __name__ == "__main__":
    main()
