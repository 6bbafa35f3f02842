"""A mesh as its surface: the face counts, the samples and the polygon crop on a height field of 10^6
triangles sampled at some 10 points per face, the kernels alone and sample_mesh() as a whole (counts, torch's integer scan, the
read-back of the areas, samples), beside the numpy restatement (tests/surface_restated.py) on the same machine. HIP events around each
call, median of the repetitions, the kernels alternating over three rounds.

    python tools/surface_timing.py [--faces 1000000] [--per_face 10] [--reps 10] [--no_numpy] [--output profiles/surface_timing.json]

Beside each kernel: the bytes it must read and write at the least (every input once, every output once; SAMPLE's binary search reads
its offsets through L2 and is not counted again) over the HBM bandwidth of MI355X_MICROARCH.md, 6.29 TB/s measured for a float4
copy (8 TB/s on the data sheet). SAMPLE finds a sample's face by a per-lane binary search; the per-wavefront search and walk was not
built (DESIGN.md section 4n says why), so there is one time, not two. Prints one JSON line and, with --output, writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acezero_amd import _native as N  # noqa: E402
from acezero_amd import geometry as G  # noqa: E402
from acezero_amd.formats import CropVolume  # noqa: E402
from acezero_amd.head import _ptr, _stream  # noqa: E402
from tests import surface_restated as SR  # noqa: E402
from tools.rgbd_timing import _time  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def height_field(faces, seed=1, cell=0.01):
    """(vertices float32 [m,3], faces int32 [k,3], colours uint8 [m,3]): a grid of quads, two triangles each, over a rough surface."""
    rows = int(round(np.sqrt(faces / 4)))
    cols = faces // (2 * rows)
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(rows + 1) * cell, np.arange(cols + 1) * cell, indexing="ij")
    z = 0.05 * np.sin(3 * x) * np.cos(2 * y) + rng.normal(scale=cell / 5, size=x.shape)
    v = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    i = (np.arange(rows)[:, None] * (cols + 1) + np.arange(cols)[None, :]).reshape(-1)
    f = np.stack([np.stack([i, i + 1, i + cols + 2], 1), np.stack([i, i + cols + 2, i + cols + 1], 1)], 1).reshape(-1, 3).astype(np.int32)
    return v, f, rng.integers(0, 256, (len(v), 3), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=1_000_000)
    ap.add_argument("--per_face", type=float, default=10.0, help="samples per face on average")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no_numpy", action="store_true")
    ap.add_argument("--output", type=str, default=None)
    a = ap.parse_args()
    v_h, f_h, c_h = height_field(a.faces)
    m, k = len(v_h), len(f_h)
    area = SR.face_counts(v_h, f_h, 1.0, 0)[1].sum()
    spacing = float(np.sqrt(area / (a.per_face * k)))
    density, seed = G.sample_density(spacing), 0
    v, f, c = (torch.from_numpy(x).cuda() for x in (v_h, f_h, c_h))
    counts = torch.empty(k, dtype=torch.int32, device="cuda")
    areas = torch.empty(k, dtype=torch.float64, device="cuda")
    lib = N.lib()

    def counts_kernel():
        N.check(lib.acez_geom_face_counts(_ptr(v), m, _ptr(f), k, density, seed, _ptr(counts), _ptr(areas), _stream()))

    counts_kernel()
    offsets = torch.zeros(k + 1, dtype=torch.int64, device="cuda")

    def scan():
        offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)

    scan()
    n = int(offsets[-1].item())
    points = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    face = torch.empty(n, dtype=torch.int32, device="cuda")
    colours = torch.empty((n, 3), dtype=torch.uint8, device="cuda")
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")

    def sample_kernel(with_colours=False):
        N.check(lib.acez_geom_sample_faces(_ptr(v), m, _ptr(f), k, _ptr(offsets), n, seed, _ptr(c) if with_colours else None, _ptr(points),
                                           _ptr(face), _ptr(colours) if with_colours else None, _stream()))

    polygons = {}
    for corners in (8, 64, 1024):
        th = np.arange(corners) * (2 * np.pi / corners)
        centre, radius = v_h[:, :2].mean(0), 0.4 * (v_h[:, :2].max(0) - v_h[:, :2].min(0))
        polygons[corners] = torch.from_numpy((centre + radius * np.stack([np.cos(th), np.sin(th)], 1)).astype(np.float32)).cuda()

    def crop_kernel(corners):
        N.check(lib.acez_geom_crop_polygon(_ptr(points), n, _ptr(polygons[corners]), corners, 2, -1.0, 1.0, _ptr(keep), _stream()))

    legs = {"counts_kernel": counts_kernel, "scan_torch_cumsum": scan, "sample_kernel": sample_kernel,
            "sample_kernel_with_colours": lambda: sample_kernel(True)}
    legs.update({f"crop_kernel_{corners}_corners": (lambda corners=corners: crop_kernel(corners)) for corners in polygons})
    ms = {name: [] for name in legs}
    for _ in range(3):                                            # alternate the legs
        for name, fn in legs.items():
            ms[name].append(_time(fn, a.reps))
    out = {"vertices": m, "faces": k, "samples": n, "spacing": spacing, "reps": a.reps, "find_face": "binary search per lane"}
    for name, rounds in ms.items():
        out[name + "_ms"], out[name + "_ms_rounds"] = float(np.median(rounds)), rounds
    least = {"counts_kernel": m * 12 + k * 12 + k * 12, "sample_kernel": n * 16 + (k + 1) * 8 + k * 12 + m * 12,
             "sample_kernel_with_colours": n * 19 + (k + 1) * 8 + k * 12 + m * 15}
    least.update({f"crop_kernel_{corners}_corners": n * 13 for corners in polygons})
    for name, b in least.items():
        out[name + "_least_bytes"] = b
        out[name + "_hbm_bound_ms_at_6.29_TB_s"], out[name + "_hbm_bound_ms_at_8_TB_s"] = b / HBM_MEASURED * 1e3, b / HBM_SPEC * 1e3
        out[name + "_share_of_measured_hbm_bound"] = b / HBM_MEASURED * 1e3 / out[name + "_ms"]
    out["crop_edge_tests_per_s_1024_corners"] = n * 1024 / (out["crop_kernel_1024_corners_ms"] * 1e-3)
    out["sample_mesh_ms"] = _time(lambda: G.sample_mesh(v, f, spacing=spacing, seed=seed), max(3, a.reps // 2))
    out["sample_mesh_with_colours_ms"] = _time(lambda: G.sample_mesh(v, f, spacing=spacing, seed=seed, colours=c), max(3, a.reps // 2))
    crop = CropVolume(polygons[64].cpu().numpy(), 2, np.float32(-1), np.float32(1))
    out["crop_to_polygon_64_corners_ms"] = _time(lambda: G.crop_to_polygon(points, crop), max(3, a.reps // 2))
    if not a.no_numpy:
        t0 = time.perf_counter()
        want_counts, want_areas = SR.face_counts(v_h, f_h, density, seed)
        t1 = time.perf_counter()
        want = SR.sample_faces(v_h, f_h, SR.offsets_of(want_counts), seed)
        t2 = time.perf_counter()
        got_points = points.cpu().numpy()
        want_keep = SR.crop_keep(got_points, polygons[8].cpu().numpy(), 2, -1.0, 1.0)
        t3 = time.perf_counter()
        out["numpy_counts_s"], out["numpy_sample_s"], out["numpy_crop_8_corners_s"] = t1 - t0, t2 - t1, t3 - t2
        sample_kernel()
        crop_kernel(8)
        torch.cuda.synchronize()
        out["areas_equal"] = bool(np.array_equal(areas.cpu().numpy().view(np.uint64), want_areas.view(np.uint64)))
        out["counts_equal"] = bool(np.array_equal(counts.cpu().numpy(), want_counts))
        out["samples_equal"] = bool(np.array_equal(points.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
                                    and np.array_equal(face.cpu().numpy(), want[1]))
        out["crop_equal"] = bool(np.array_equal(keep.cpu().numpy().astype(bool), want_keep))
    line = json.dumps({key: (float(f"{x:.4g}") if isinstance(x, float) else x) for key, x in out.items()})
    print(line)
    if a.output:
        with open(a.output, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
