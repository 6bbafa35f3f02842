"""Kernel time of one acez_render_frame call (1280 x 720, HIP events around the call, median of 20 after 3 warm-up calls) at 0.1 M,
1 M and 4 M points plus 10^4 triangles of camera geometry. Prints one JSON line per size.

Then a registration frame (0.1 M points, the same camera geometry) without and with the query's 480 x 640 image in its frustum: the
image on the device (mip chain build + render), and the image on the host (upload + mip chain build + render)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acezero_amd import render  # noqa: E402


def _median_ms(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


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
        med, mn = _median_ms(lambda: r.render_device(xyz, rgb, tri, rgba, T))
        print(json.dumps({"points": n, "triangles": int(tri.shape[0]), "width": 1280, "height": 720, "ms_median": med, "ms_min": mn}), flush=True)
    # registration frame: the query 1 m in front of the viewer's path, its frustum (scale 0.3) and thumbnail a few dozen px tall
    n = 100_000
    xyz = torch.from_numpy((rng.normal(size=(n, 3)) * 1.5).astype(np.float32)).cuda()
    rgb = torch.from_numpy(rng.integers(0, 256, size=(n, 3)).astype(np.uint8)).cuda()
    query = np.eye(4)
    query[:3, 3] = [0.2, 0.1, 4.0]
    host_img = rng.integers(0, 256, size=(480, 640, 3)).astype(np.uint8)
    dev_img = torch.from_numpy(host_img).cuda()
    quad, uv = render.image_box(query, 640 / 480, 0.3)
    with_frustum = render.Mesh.concatenate([mesh, render.frustum_outline(query, size=0.3)])
    ftri, frgba = (torch.from_numpy(a).cuda() for a in with_frustum.triangles())
    cases = {"outline": None, "thumbnail_device_image": [(quad, uv, dev_img)], "thumbnail_host_image": [(quad, uv, host_img)]}
    for name, textured in cases.items():
        med, mn = _median_ms(lambda: r.render_device(xyz, rgb, ftri, frgba, T, textured=textured))
        print(json.dumps({"registration_frame": name, "points": n, "triangles": int(ftri.shape[0]), "texture": [480, 640] if textured else None,
                          "width": 1280, "height": 720, "ms_median": med, "ms_min": mn}), flush=True)


if __name__ == "__main__":
    main()
