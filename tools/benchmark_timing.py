"""Time of the reprojection scorer (acezero_amd.benchmark.score_views = acez_reproject_score: clear, nearest, accumulate, score) for one
session-sized case: about 1 M points (a 1000-frame session's filtered cloud), 125 held-out views of 60 x 80 cells. HIP events around the
call, median of 20 after a warm-up; the scratch allocation is outside the timed region. Writes one JSON object.

    python tools/benchmark_timing.py [--out profiles/benchmark_timing.json]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

M, T, OH, OW, REPS = 1_000_000, 125, 60, 80, 20


def make_case(seed=0):
    """Points on the walls of a 6 x 4 x 3 m room, cameras near its centre turning through 360 degrees (f = 525 px at 640 x 480)."""
    from acezero_amd.benchmark import make_views
    rng = np.random.default_rng(seed)
    room = np.array([6.0, 4.0, 3.0])
    pts = rng.uniform(0, 1, (M, 3)) * room
    axis = rng.integers(0, 3, M)
    pts[np.arange(M), axis] = room[axis] * rng.integers(0, 2, M)
    w2c = np.zeros((T, 4, 4))
    for i in range(T):
        a = 2 * math.pi * i / T
        c2w = np.eye(4)
        c2w[:3, :3] = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        c2w[:3, 3] = room / 2 + rng.normal(0, 0.2, 3)
        w2c[i] = np.linalg.inv(c2w)
    return (pts.astype(np.float32), rng.integers(0, 256, (M, 3)).astype(np.uint8), make_views(w2c, 525.0, 320.0, 240.0),
            rng.integers(0, 256, (T, OH, OW, 3)).astype(np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "benchmark_timing.json"))
    a = ap.parse_args()
    import ctypes as C
    from acezero_amd import _native as N
    from acezero_amd.head import _ptr, _stream
    pts, clr, views, targets = (torch.from_numpy(x).cuda() for x in make_case())
    need = C.c_int64(0)
    N.check(N.lib().acez_reproject_scratch_size(T, OH, OW, C.byref(need)))
    scratch = torch.empty((need.value // 8,), dtype=torch.int64, device="cuda")
    sse = torch.empty((T,), dtype=torch.int64, device="cuda")
    cov = torch.empty((T,), dtype=torch.int32, device="cuda")

    def call():
        N.check(N.lib().acez_reproject_score(_ptr(pts), _ptr(clr), M, _ptr(views), T, OH, OW, _ptr(targets), 0.05, _ptr(scratch), need.value,
                                             _ptr(sse), _ptr(cov), None, None, _stream()))
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    out = {"points": M, "views": T, "cells": [OH, OW], "reps": REPS, "median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3),
           "max_ms": round(max(ms), 3), "mean_coverage": round(float((cov.cpu().numpy() / (OH * OW)).mean()), 4),
           "projections_per_s": round(M * T * 2 / (float(np.median(ms)) * 1e-3)), "device": torch.cuda.get_device_name(0)}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
