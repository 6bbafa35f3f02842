"""Frames/s of the DSAC* backward kernels (acez_register_rgbd_backward_device, acez_register_rgb_backward_device) at 60 x 80 cells and
64 hypotheses, next to the forward kernels on the same frames: HIP events around each batched call, median of the repetitions.

    python tools/rgbd_grad_timing.py [--frames 1024] [--reps 10] [--tries 16]

Frames are tools/rgbd_timing.py's, with the scene coordinates' map moved by 2 degrees / 5 cm so that the loss is not at its minimum.
The RGB frames are synth.make_registration_frames' with their ground-truth poses. Prints one JSON line."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from acezero_amd import dsacstar, synth  # noqa: E402
from rgbd_timing import _time, rgbd_frames  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tries", type=int, default=16)
    a = ap.parse_args()
    n = a.frames
    sc, cc = rgbd_frames(n)
    c, s = math.cos(math.radians(2)), math.sin(math.radians(2))
    Rz = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], device="cuda")
    sc = (torch.einsum("ij,njhw->nihw", Rz, sc) + torch.tensor([0.05, 0.0, 0.0], device="cuda").view(1, 3, 1, 1)).contiguous()
    gt = torch.eye(4).repeat(n, 1, 1)   # the loss value does not change the work, only the sampled frames do
    ids = list(range(n))
    prm = dict(hyps=64, thr=10.0, alpha=100.0, max_reproj=100.0, max_tries=a.tries)
    grad = torch.zeros_like(sc)
    ms_b = _time(lambda: dsacstar.register_batch_rgbd_backward(sc, cc, gt, prm, 1305, ids, 1.0, 100.0, 100.0, out_grad=grad), a.reps)
    ms_f = _time(lambda: dsacstar.register_batch_rgbd(sc, cc, prm, 1305, ids, want_masks=False), a.reps)
    dsacstar.register_batch_rgbd_backward(sc, cc, gt, prm, 1305, ids, 1.0, 100.0, 100.0)
    torch.cuda.synchronize()
    probs = dsacstar.debug_fetch_rgbd_backward(n, 64, 60, 80)["probs"]
    refined = float((probs >= dsacstar.PROB_THRESH).sum(1).mean())
    fr = synth.make_registration_frames(seed=3, n_frames=64)
    rep = (n + 63) // 64
    rsc = torch.from_numpy(fr["scene_coords"]).cuda().repeat(rep, 1, 1, 1)[:n].contiguous()
    rgt = torch.from_numpy(np.asarray(fr["poses"], np.float32)).repeat(rep, 1, 1)[:n]
    rprm = dict(hyps=64, thr=10.0, alpha=100.0, max_reproj=100.0, sub=8, max_tries=a.tries)
    intr = [(fr["focal"], fr["ppx"], fr["ppy"])] * n
    rgrad = torch.zeros_like(rsc)
    ms_rb = _time(lambda: dsacstar.register_batch_backward(rsc, intr, rgt, rprm, 1305, ids, 1.0, 100.0, 100.0, out_grad=rgrad), a.reps)
    ms_rf = _time(lambda: dsacstar.register_batch(rsc, intr, rprm, 1305, ids, want_masks=False), a.reps)
    dsacstar.register_batch_backward(rsc, intr, rgt, rprm, 1305, ids, 1.0, 100.0, 100.0)
    torch.cuda.synchronize()
    rrefined = float((dsacstar.debug_fetch_rgb_backward(n, 64, 60, 80)["probs"] >= dsacstar.PROB_THRESH).sum(1).mean())
    print(f"RGB backward: {ms_rb:.3f} ms = {n / ms_rb * 1e3:.0f} frames/s ({rrefined:.1f} hypotheses refined per frame); "
          f"forward: {ms_rf:.3f} ms = {n / ms_rf * 1e3:.0f} frames/s")
    print(f"RGB-D backward: {n} frames in {ms_b:.3f} ms = {n / ms_b * 1e3:.0f} frames/s ({refined:.1f} hypotheses refined per frame); "
          f"forward: {ms_f:.3f} ms = {n / ms_f * 1e3:.0f} frames/s")
    print(json.dumps({"frames": n, "hyps": 64, "cells": "60x80", "max_tries": a.tries, "rgbd_backward_ms": ms_b,
                      "rgbd_backward_frames_per_s": n / ms_b * 1e3, "rgbd_forward_ms": ms_f, "rgbd_forward_frames_per_s": n / ms_f * 1e3,
                      "refined_per_frame": refined, "rgb_backward_ms": ms_rb, "rgb_backward_frames_per_s": n / ms_rb * 1e3,
                      "rgb_forward_ms": ms_rf, "rgb_forward_frames_per_s": n / ms_rf * 1e3, "rgb_refined_per_frame": rrefined}))


if __name__ == "__main__":
    main()
