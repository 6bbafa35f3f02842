"""Pose evaluation (estimate_alignment + per-frame errors) on the GPU against a CPU run of the same algorithm, at N = 500 and
3000 frames, H = 10 000 hypotheses, on the trajectory cases of tests/eval_cases.py. Prints one JSON line:
  gpu_ms[N][scale]  median wall time of acezero_amd.evaluate.evaluate_poses (one call = upload, three launches, one sync)
  cpu_s[N][scale]   tests/eval_restated.py (numpy, vectorised over hypotheses) on the same inputs and the same triples

    python tools/eval_timing.py                 # both
    python tools/eval_timing.py --cpu-only      # no GPU needed
    python tools/eval_timing.py --gpu-only      # e.g. under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests.eval_cases import CASES, make_inputs  # noqa: E402

H = 10000


def inputs(n):
    spec = dict(CASES["traj_n3000"], n=n)
    return make_inputs(spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    out = {"H": H, "gpu_ms": {}, "cpu_s": {}}
    for n in (500, 3000):
        est, gt, conf = inputs(n)
        tri = np.stack([np.random.RandomState(h).choice(n, 3, replace=False) for h in range(H)])
        for scale in (True, False):
            key = f"scale{int(scale)}"
            if not a.cpu_only:
                from acezero_amd.evaluate import evaluate_poses
                evaluate_poses(est, gt, conf, estimate_alignment_scale=scale, samples=tri)       # context allocation, code-object load
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    evaluate_poses(est, gt, conf, estimate_alignment_scale=scale, samples=tri)
                    ts.append((time.perf_counter() - t0) * 1e3)
                out["gpu_ms"].setdefault(str(n), {})[key] = round(float(np.median(ts)), 3)
            if not a.gpu_only:
                from tests.eval_restated import estimate_alignment
                t0 = time.perf_counter()
                estimate_alignment(gt, est, conf, tri, estimate_scale=scale, chunk=100)
                out["cpu_s"].setdefault(str(n), {})[key] = round(time.perf_counter() - t0, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
