"""Kernel time of one acez_render_frame call (1280 x 720, HIP events around the call, median of 20 after 3 warm-up calls) at 0.1 M,
1 M and 4 M points plus 10^4 triangles of camera geometry. Prints one JSON line per size."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acezero_amd import render  # noqa: E402


def main():
    rng = np.random.default_rng(0)
    T = np.eye(4)
    T[:3, 3] = [0, 0, 5.0]
    r = render.Renderer()
    mesh = render.Mesh.concatenate([render.frustum_outline(np.eye(4) + np.pad(rng.normal(size=(3, 1)), ((0, 1), (3, 0))),
                                                           size=0.1) for _ in range(105)])
    tri, rgba = (torch.from_numpy(a).cuda() for a in mesh.triangles())
    for n in (100_000, 1_000_000, 4_000_000):
        xyz = torch.from_numpy((rng.normal(size=(n, 3)) * 1.5).astype(np.float32)).cuda()
        rgb = torch.from_numpy(rng.integers(0, 256, size=(n, 3)).astype(np.uint8)).cuda()
        for _ in range(3):
            r.render_device(xyz, rgb, tri, rgba, T)
        ms = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r.render_device(xyz, rgb, tri, rgba, T)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        print(json.dumps({"points": n, "triangles": int(tri.shape[0]), "width": 1280, "height": 720, "ms_median": float(np.median(ms)),
                          "ms_min": float(np.min(ms))}), flush=True)


if __name__ == "__main__":
    main()
