"""Cloud distances on the box: one directed nearest-neighbour search of n x n points, the kernel alone and
nearest_distances() as a whole (grid build, sorts, kernel, un-ordering), beside scipy's k-d tree with 16 workers on the same
machine. HIP events around each call, median of the repetitions.

    python tools/geometry_timing.py [--points 1000000] [--radius 0.02 0.05] [--reps 10] [--no_tree] [--also name=other_build.so]

The clouds are samples of the walls of the analytic box room of tests/fusion_cases.py (8.85 m^2: 10^6 points are 3 mm apart), the
reference with 2 mm of noise, the queries with 5 mm. The kernel is timed on the same buffers, alternating: the product build, the
diagnostics build, and the diagnostics build with ACEZ_GEOM_PLAIN (every workgroup takes the per-lane form instead of staging in
LDS); --also adds other builds of the library (tools/lib_variant.sh) to the rotation. `pairs` counts the references in each query's
own 27 cells, the distance evaluations the per-lane form makes; the bound beside it is that count times 13 vector instructions over
78.6e12 lane-instructions per second (the fp32 vector peak without
counting an fma twice). Prints one JSON line."""
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
from acezero_amd.head import _ptr, _stream  # noqa: E402
from tests import fusion_cases as FC  # noqa: E402
from tools.rgbd_timing import _time  # noqa: E402

VALU_LANE_OPS_PER_S = 78.6e12
OPS_PER_PAIR = 13


def wall_samples(seed, n, noise, half=FC.ROOM_HALF):
    rng = np.random.default_rng(seed)
    area = np.array([half[1] * half[2], half[0] * half[2], half[0] * half[1]])
    axis = rng.choice(3, n, p=area / area.sum())
    p = rng.uniform(-1, 1, (n, 3)) * half
    p[np.arange(n), axis] = np.where(rng.random(n) < 0.5, -1, 1) * half[axis]
    return (p + rng.normal(scale=noise, size=(n, 3))).astype(np.float32)


def prepared(query, ref, r):
    """The buffers nearest_distances() hands to acez_geom_nearest, and the number of references in every query's own 27 cells."""
    lo, hi = (a.cpu().numpy() for a in (ref.min(0).values, ref.max(0).values))
    c = np.float32(r) * G.MARGIN
    dims = G.grid_dims(lo, hi, c)
    cells = G.point_cells(ref, lo, c, dims)
    order = torch.sort(cells, stable=True)
    n_cells = dims[0] * dims[1] * dims[2]
    start = torch.zeros(n_cells + 1, dtype=torch.int32, device=ref.device)
    start[1:] = torch.cumsum(torch.bincount(order.values.long(), minlength=n_cells), 0).to(torch.int32)
    key = G.point_cells(torch.minimum(torch.maximum(query, ref.min(0).values), ref.max(0).values), lo, c, dims)
    q_sorted = query[torch.sort(key, stable=True).indices].contiguous()
    ijk = torch.floor((q_sorted - torch.from_numpy(lo).to(ref.device)) / float(c)).long()
    pairs = 0
    big = start.long()
    for dk in (-1, 0, 1):
        for dj in (-1, 0, 1):
            j, k = ijk[:, 1] + dj, ijk[:, 2] + dk
            ok = (j >= 0) & (j < dims[1]) & (k >= 0) & (k < dims[2]) & (ijk[:, 0] >= -1) & (ijk[:, 0] <= dims[0])
            base = (k.clamp(0, dims[2] - 1) * dims[1] + j.clamp(0, dims[1] - 1)) * dims[0]
            i0, i1 = (ijk[:, 0] - 1).clamp(0, dims[0] - 1), (ijk[:, 0] + 1).clamp(0, dims[0] - 1)
            pairs += int(((big[base + i1 + 1] - big[base + i0]) * ok).sum().item())
    args = (ref[order.indices].contiguous(), order.indices.to(torch.int32), start, lo, float(c), dims, q_sorted)
    return args, pairs, int((torch.bincount(order.values.long(), minlength=n_cells) > 0).sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--radius", type=float, nargs="+", default=[0.02, 0.05])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no_tree", action="store_true")
    ap.add_argument("--also", nargs="*", default=[], help="name=path of further builds of the library to time on the same buffers")
    a = ap.parse_args()
    others = {spec.split("=", 1)[0]: N._load(spec.split("=", 1)[1]) for spec in a.also}
    n = a.points
    ref_h, query_h = wall_samples(1, n, 0.002), wall_samples(2, n, 0.005)
    ref, query = torch.from_numpy(ref_h).cuda(), torch.from_numpy(query_h).cuda()
    out = {"points": n, "reps": a.reps}
    for r in a.radius:
        (ref_s, ref_i, start, lo, c, dims, q_s), pairs, occupied = prepared(query, ref, r)
        d2 = torch.empty(n, dtype=torch.float32, device="cuda")
        idx = torch.empty(n, dtype=torch.int32, device="cuda")

        def kernel(lib=None):
            N.check((lib or N.lib()).acez_geom_nearest(_ptr(ref_s), _ptr(ref_i), _ptr(start), n, float(lo[0]), float(lo[1]), float(lo[2]), c, *dims,
                                              _ptr(q_s), n, float(np.float32(r)), _ptr(d2), _ptr(idx), _stream()))

        tag = f"r{r}"
        out[f"{tag}_grid"], out[f"{tag}_occupied_cells"], out[f"{tag}_pairs"] = "x".join(map(str, dims)), occupied, pairs
        out[f"{tag}_valu_bound_ms"] = pairs * OPS_PER_PAIR / VALU_LANE_OPS_PER_S * 1e3
        results = {}
        ms = {name: [] for name in ["product", "diag_staged", "diag_per_lane"] + list(others)}
        for _ in range(3):                                        # alternate the forms
            ms["product"].append(_time(kernel, a.reps))
            results["product"] = (d2.clone(), idx.clone())
            for name, lib in others.items():
                ms[name].append(_time(lambda: kernel(lib), a.reps))
                results[name] = (d2.clone(), idx.clone())
            with N.diag_library():
                ms["diag_staged"].append(_time(kernel, a.reps))
                results["diag_staged"] = (d2.clone(), idx.clone())
                os.environ["ACEZ_GEOM_PLAIN"] = "1"
                try:
                    ms["diag_per_lane"].append(_time(kernel, a.reps))
                finally:
                    del os.environ["ACEZ_GEOM_PLAIN"]
                results["diag_per_lane"] = (d2.clone(), idx.clone())
        for name, v in ms.items():
            out[f"{tag}_kernel_{name}_ms"] = float(np.median(v))
            out[f"{tag}_kernel_{name}_ms_rounds"] = v
            assert torch.equal(results[name][0], results["product"][0]) and torch.equal(results[name][1], results["product"][1]), name
        out[f"{tag}_found"] = int((results["product"][1] >= 0).sum().item())
        out[f"{tag}_nearest_distances_ms"] = _time(lambda: G.nearest_distances(query, ref, r), max(3, a.reps // 2))
        whole = G.nearest_distances(query, ref, r)
        if not a.no_tree:
            from scipy.spatial import cKDTree
            t0 = time.perf_counter()
            tree = cKDTree(ref_h)
            t1 = time.perf_counter()
            dist, _ = tree.query(query_h, k=1, distance_upper_bound=r, workers=16)
            t2 = time.perf_counter()
            out[f"{tag}_ckdtree_build_s"], out[f"{tag}_ckdtree_query_16_workers_s"] = t1 - t0, t2 - t1
            found = np.isfinite(dist)
            out[f"{tag}_ckdtree_found"] = int(found.sum())
            got = np.sqrt(whole[0].cpu().numpy().astype(np.float64))
            both = found & np.isfinite(got)
            out[f"{tag}_max_rel_difference_to_ckdtree"] = float(np.max(np.abs(got[both] - dist[both]) / np.maximum(dist[both], 1e-12)))
    print(json.dumps({k: (float(f"{x:.4g}") if isinstance(x, float) else x) for k, x in out.items()}))


if __name__ == "__main__":
    main()
