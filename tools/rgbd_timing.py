"""Frames/s of the RGB-D registration kernel (acez_register_rgbd_device) at 60 x 80 cells and 64 hypotheses, next to the RGB
path's (acez_register_rgb_device) on the same batch size: HIP events around each batched call, median of the repetitions.

    python tools/rgbd_timing.py [--frames 2048] [--reps 10] [--tries 16]

Synthetic frames: camera coordinates back-projected from random depth (1 cm noise, 20 % missing), scene coordinates from a random
pose with 30 % outliers; the RGB frames are synth.make_registration_frames'. Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acezero_amd import dsacstar, synth  # noqa: E402


def rgbd_frames(n, h=60, w=80, focal=525.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    depth = torch.rand(n, h, w, generator=g, device="cuda") * 3 + 1
    eye = dsacstar.camera_coordinates(depth, focal, w * 4.0, h * 4.0)
    q = torch.nn.functional.normalize(torch.randn(n, 4, generator=g, device="cuda"), dim=1)
    a, b, c, d = q.unbind(1)
    R = torch.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c),
                     2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b),
                     2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], 1).view(n, 3, 3)
    t = torch.rand(n, 3, 1, 1, generator=g, device="cuda") * 6 - 3
    sc = torch.einsum("nji,njhw->nihw", R, eye - t)
    bad = torch.rand(n, 1, h, w, generator=g, device="cuda") < 0.3
    sc = torch.where(bad, torch.rand(n, 3, h, w, generator=g, device="cuda") * 10 - 5, sc)
    cc = eye + torch.randn(eye.shape, generator=g, device="cuda") * 0.01
    cc = torch.where(torch.rand(n, 1, h, w, generator=g, device="cuda") < 0.2, torch.zeros_like(cc), cc)
    return sc.contiguous(), cc.contiguous()


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tries", type=int, default=16)
    a = ap.parse_args()
    n = a.frames
    sc, cc = rgbd_frames(n)
    ids = list(range(n))
    prm = dict(hyps=64, thr=10.0, alpha=100.0, max_reproj=100.0, max_tries=a.tries)
    ms_d = _time(lambda: dsacstar.register_batch_rgbd(sc, cc, prm, 1305, ids, want_masks=False), a.reps)
    _, inl, _ = dsacstar.register_batch_rgbd(sc, cc, prm, 1305, ids, want_masks=False)
    fr = synth.make_registration_frames(seed=3, n_frames=64)
    rsc = torch.from_numpy(fr["scene_coords"]).cuda().repeat((n + 63) // 64, 1, 1, 1)[:n].contiguous()
    rprm = dict(hyps=64, thr=10.0, alpha=100.0, max_reproj=100.0, sub=8, max_tries=a.tries)
    intr = [(fr["focal"], fr["ppx"], fr["ppy"])] * n
    ms_r = _time(lambda: dsacstar.register_batch(rsc, intr, rprm, 1305, ids, want_masks=False), a.reps)
    print(f"RGB-D: {n} frames in {ms_d:.3f} ms = {n / ms_d * 1e3:.0f} frames/s (median inliers {float(inl.float().median()):.0f}); "
          f"RGB: {ms_r:.3f} ms = {n / ms_r * 1e3:.0f} frames/s")
    print(json.dumps({"frames": n, "hyps": 64, "cells": "60x80", "max_tries": a.tries, "rgbd_ms": ms_d, "rgbd_frames_per_s": n / ms_d * 1e3,
                      "rgb_ms": ms_r, "rgb_frames_per_s": n / ms_r * 1e3}))


if __name__ == "__main__":
    main()
