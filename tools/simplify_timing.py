"""The mesh simplification on the box: the whole call for both placements and every stage on its own, on the
meshes fuse_depth.py produces, at a cell of three voxels. HIP events around each stage, median of the repetitions; the meshes are on
the device before the timed calls.

    python tools/simplify_timing.py [--frames 48] [--dim 256] [--sparse_voxel 0.0075] [--reps 10] [--no_sparse]

Meshes: the room of tools/fusion_timing.py fused into the dense dim^3 volume at 0.02 m, and the same room fused into the block-sparse
volume at --sparse_voxel. `filter_*_ms`: mesh.filter_components on the same mesh, without a criterion and with keep_largest=1, whole
calls like `whole_*_ms`. Stages: the kernels of acezero_amd/csrc/simplify_api.hip one by one and torch's sorts and searches between
them. `layouts`: the per-cluster quadric sums alone in the two layouts of include/acez.h section Q step 5 (tools/simplify_layouts.hip,
built here into tools/libacez_simplify_layouts.so): one lane per cluster, and one wavefront per cluster, which is what the product
does, alternating, with the largest relative difference between their sums. open3d's simplify_vertex_clustering on the host is timed on the same
mesh if open3d can be imported, else `open3d` says that it cannot. Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acezero_amd import _native as N  # noqa: E402
from acezero_amd import fusion, mesh, simplify  # noqa: E402
from acezero_amd.head import _ptr, _stream  # noqa: E402
from tests import fusion_cases as FC  # noqa: E402
from tools.rgbd_timing import _time  # noqa: E402


def layouts_library():
    so, src = os.path.join(ROOT, "tools", "libacez_simplify_layouts.so"), os.path.join(ROOT, "tools", "simplify_layouts.hip")
    deps = [src] + [os.path.join(ROOT, "acezero_amd", "csrc", f) for f in ("simplify_solve.h", "svd3.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src],
                       check=True)
    lib = C.CDLL(so)
    lib.simplify_layout_accumulate.restype = C.c_int
    lib.simplify_layout_accumulate.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_float] * 4 + [
        C.c_void_p, C.c_void_p]
    return lib


def stages(vertices, colours, faces, cell, reps):
    """simplify.simplify_mesh's steps one by one (the same calls in the same order), each timed on its own."""
    lib, dev = N.lib(), faces.device
    m, k = vertices.shape[0], faces.shape[0]
    out = {"vertices": m, "faces": k, "cell": cell}
    for placement in simplify.PLACEMENTS:
        out[f"whole_{placement}_ms"] = _time(lambda: simplify.simplify_mesh(vertices, colours, faces, cell, placement), reps)
    for name, criteria in (("plain", {}), ("keep_largest", dict(keep_largest=1))):      # the clean-up that shares the compaction (mesh.py)
        out[f"filter_{name}_ms"] = _time(lambda: mesh.filter_components(vertices, colours, faces, **criteria), reps)
    got = simplify.simplify_mesh(vertices, colours, faces, cell)
    out["info"] = got[3]
    finite = torch.isfinite(vertices).all(1, keepdim=True)
    assert bool(finite.all())
    bounds = torch.cat([vertices.amin(0), vertices.amax(0)]).cpu().tolist()
    origin = bounds[:3]
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    out["keys_ms"] = _time(lambda: N.check(lib.acez_simplify_keys(_ptr(vertices), m, *bounds, cell, _ptr(keys), _stream())), reps)

    def vertex_sort():
        sorted_keys, order = torch.sort(keys, stable=True)
        first = torch.ones(m, dtype=torch.bool, device=dev)
        first[1:] = sorted_keys[1:] != sorted_keys[:-1]
        cluster_sorted = (torch.cumsum(first, 0, dtype=torch.int32) - 1).to(torch.int32)
        return sorted_keys, order, cluster_sorted, simplify._segments(cluster_sorted, m)

    out["vertex_sort_ms"] = _time(vertex_sort, reps)
    sorted_keys, order, cluster_sorted, segments = vertex_sort()
    n_clusters = int(cluster_sorted[-1].item()) + 1
    vertex_cluster = torch.empty(m, dtype=torch.int32, device=dev)
    out["clusters_ms"] = _time(lambda: N.check(lib.acez_simplify_clusters(_ptr(order), _ptr(cluster_sorted), m, _ptr(vertex_cluster), _stream())), reps)
    face_class = torch.empty(k, dtype=torch.uint8, device=dev)
    triples = torch.empty((k, 3), dtype=torch.int32, device=dev)
    corner_keys = torch.empty(3 * k, dtype=torch.int32, device=dev)
    out["faces_ms"] = _time(lambda: N.check(lib.acez_simplify_faces(_ptr(faces), k, _ptr(vertex_cluster), m, _ptr(face_class), _ptr(triples),
                                                                     _ptr(corner_keys), _stream())), reps)

    def corner_sort():
        sorted_corners, corner_order = torch.sort(corner_keys, stable=True)
        return corner_order, simplify._segments(sorted_corners, m)

    out["corner_sort_ms"] = _time(corner_sort, reps)
    corner_order, corner_segments = corner_sort()
    positions = torch.empty((m, 3), dtype=torch.float32, device=dev)
    cluster_colours = torch.empty((m, 3), dtype=torch.uint8, device=dev)
    fallback = torch.zeros(m, dtype=torch.uint8, device=dev)
    quadrics = torch.empty((m, 9), dtype=torch.float64, device=dev)
    out["quadrics_ms"] = _time(lambda: N.check(lib.acez_simplify_quadrics(
        _ptr(vertices), m, _ptr(faces), k, _ptr(sorted_keys), _ptr(segments), _ptr(corner_order), _ptr(corner_segments), *origin, cell,
        _ptr(quadrics), _stream())), reps)
    for sums, name in ((quadrics, "quadric"), (None, "mean")):
        out[f"place_{name}_ms"] = _time(lambda: N.check(lib.acez_simplify_place(
            _ptr(vertices), _ptr(colours), m, _ptr(sorted_keys), _ptr(order), _ptr(segments), _ptr(sums), *origin, cell, _ptr(positions),
            _ptr(cluster_colours), _ptr(fallback), _stream())), reps)

    def face_sort():
        by_third = torch.sort(triples[:, 2], stable=True).indices
        pair = triples[:, 0].long() * (m + 1) + triples[:, 1].long()
        return by_third[torch.sort(pair[by_third], stable=True).indices].contiguous()

    out["face_sort_ms"] = _time(face_sort, reps)
    perm = face_sort()
    face_keep = torch.empty(k, dtype=torch.uint8, device=dev)
    cluster_used = torch.empty(m, dtype=torch.uint8, device=dev)
    out["unique_ms"] = _time(lambda: N.check(lib.acez_simplify_unique(_ptr(triples), _ptr(face_class), _ptr(perm), k, m, _ptr(face_keep),
                                                                      _ptr(cluster_used), _stream())), reps)
    # the two layouts of the quadric sums, alternating
    probe = layouts_library()
    sums = [torch.zeros((m, 9), dtype=torch.float64, device=dev) for _ in range(2)]

    def accumulate(layout):
        rc = probe.simplify_layout_accumulate(layout, n_clusters, _ptr(vertices), m, _ptr(faces), k, _ptr(sorted_keys), _ptr(segments),
                                              _ptr(corner_order), _ptr(corner_segments), *origin, cell, _ptr(sums[layout]), _stream())
        assert rc == 0, rc

    lane, wave = [], []
    for _ in range(3):
        lane.append(_time(lambda: accumulate(0), reps))
        wave.append(_time(lambda: accumulate(1), reps))
    scale = sums[0][:n_clusters].abs().amax(1, keepdim=True).clamp_min(1e-300)
    corners = (corner_segments[1:n_clusters + 1] - corner_segments[:n_clusters]).to(torch.float64)
    out["layouts"] = {"clusters": n_clusters, "corners_per_cluster_mean": float(corners.mean().item()), "corners_per_cluster_max": int(corners.max().item()),
                      "lane_per_cluster_ms": lane, "wave_per_cluster_ms": wave,
                      "largest_relative_difference": float(((sums[0] - sums[1])[:n_clusters].abs() / scale).max().item()),
                      "product_is_wave_per_cluster_bit_for_bit": bool(torch.equal(quadrics[:n_clusters].view(torch.int64),
                                                                                  sums[1][:n_clusters].view(torch.int64)))}
    try:
        import open3d as o3d
    except ImportError:
        out["open3d"] = "not importable on this machine: no same-machine comparison"
    else:
        o3d_mesh = o3d.geometry.TriangleMesh(o3d.utility.Vector3dVector(vertices.cpu().numpy().astype(np.float64)),
                                             o3d.utility.Vector3iVector(faces.cpu().numpy()))
        best = []
        for _ in range(3):
            t0 = time.perf_counter()
            small = o3d_mesh.simplify_vertex_clustering(cell, o3d.geometry.SimplificationContraction.Quadric)
            best.append((time.perf_counter() - t0) * 1e3)
        out["open3d"] = {"host_ms": min(best), "vertices": len(small.vertices), "faces": len(small.triangles)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--sparse_voxel", type=float, default=0.0075)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no_sparse", action="store_true")
    a = ap.parse_args()
    n, dim, v, h, w, focal = a.frames, a.dim, 0.02, 480, 640, 525.0
    side = dim * v
    half = np.array([0.47, 0.31, 0.47]) * side
    c2w = FC.room_cameras(n, radius=0.1 * side)
    depth = np.stack([FC.room_depth(T, h, w, focal, half) for T in c2w])
    rgb = np.stack([FC.room_rgb(T, h, w, focal, half) for T in c2w])
    d_depth, d_rgb = torch.from_numpy(depth.view(np.int16)).cuda(), torch.from_numpy(rgb).cuda()
    frames = dict(cam_to_world=c2w, focals=focal, max_depth=0.75 * side)
    out = {"reps": a.reps}
    vol = fusion.TSDFVolume((-0.5 * side + 0.5 * v,) * 3, (dim, dim, dim), v, 4 * v, "cuda")
    vol.integrate(d_depth, rgb=d_rgb, **frames)
    out[f"room_dense_{dim}"] = stages(*vol.extract_mesh(2.0), 3 * v, a.reps)
    del vol
    if not a.no_sparse:
        sv = a.sparse_voxel
        sdim = int(round(side / sv))
        svol = fusion.SparseTSDFVolume((-0.5 * side + 0.5 * sv,) * 3, (sdim, sdim, sdim), sv, 4 * sv, "cuda")
        svol.mark(d_depth, **frames)
        svol.allocate()
        svol.integrate(d_depth, rgb=d_rgb, **frames)
        mesh_ = svol.extract_mesh(2.0)
        del svol
        out[f"room_sparse_{sv}"] = stages(*mesh_, 3 * sv, a.reps)

    def rounded(x):
        if isinstance(x, dict):
            return {key: rounded(val) for key, val in x.items()}
        if isinstance(x, list):
            return [rounded(val) for val in x]
        return float(f"{x:.4g}") if isinstance(x, float) else x

    print(json.dumps(rounded(out)))


if __name__ == "__main__":
    main()
