"""The mesh clean-up on the box: the component labelling, the counts, and select + compact, each on its own, on
the meshes fuse_depth.py produces and on the adversarial strip, beside scipy.sparse.csgraph.connected_components on the host.
HIP events around each stage, median of the repetitions; the meshes are on the device before the timed calls.

    python tools/mesh_timing.py [--frames 48] [--dim 256] [--sparse_voxel 0.0075] [--reps 10] [--no_sparse] [--no_scipy]

Meshes: the room of tools/fusion_timing.py fused into the dense dim^3 volume at 0.02 m, the same room fused into the block-sparse
volume at --sparse_voxel, and the triangle strip of 2 * 10^5 faces with its vertex ids in random order (tests/mesh_cases.py). The
filter that is timed keeps the largest component (the sort behind keep_largest included in `filter_ms`, not in the stages). scipy:
the graph's construction (a COO matrix of the faces' edges) and the labelling timed apart, best of three. Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acezero_amd import _native as N  # noqa: E402
from acezero_amd import fusion, mesh  # noqa: E402
from acezero_amd.head import _ptr, _stream  # noqa: E402
from tests import fusion_cases as FC  # noqa: E402
from tests import mesh_cases as MC  # noqa: E402
from tests.mesh_restated import classify  # noqa: E402
from tools.rgbd_timing import _time  # noqa: E402


def stages(vertices, colours, faces, reps, with_scipy):
    lib, dev = N.lib(), faces.device
    m, k = vertices.shape[0], faces.shape[0]
    out = {"vertices": m, "faces": k}
    out["label_ms"] = _time(lambda: mesh._label(faces, m), reps)
    labels, _ = mesh._label(faces, m)
    out["counts_ms"] = _time(lambda: mesh.component_sizes(faces, labels), reps)
    faces_of, _ = mesh.component_sizes(faces, labels)
    keep = torch.zeros(m, dtype=torch.uint8, device=dev)
    keep[faces_of.argmax()] = 1
    out["components"], out["largest_component_faces"] = int((faces_of > 0).sum().item()), int(faces_of.max().item())
    face_keep = torch.empty(k, dtype=torch.uint8, device=dev)
    used = torch.empty(m, dtype=torch.uint8, device=dev)
    N.check(lib.acez_mesh_select(_ptr(faces), k, _ptr(labels), m, _ptr(keep), _ptr(face_keep), _ptr(used), _stream()))
    n_f, n_v = int(face_keep.sum().item()), int(used.sum().item())
    out_v = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
    out_c = torch.empty((n_v, 3), dtype=torch.uint8, device=dev)
    out_f = torch.empty((n_f, 3), dtype=torch.int32, device=dev)

    def select_compact():
        N.check(lib.acez_mesh_select(_ptr(faces), k, _ptr(labels), m, _ptr(keep), _ptr(face_keep), _ptr(used), _stream()))
        face_rank, vertex_rank = torch.cumsum(face_keep, 0, dtype=torch.int32), torch.cumsum(used, 0, dtype=torch.int32)
        N.check(lib.acez_mesh_compact(_ptr(vertices), _ptr(colours), m, _ptr(faces), k, _ptr(face_keep), _ptr(face_rank), _ptr(used),
                                      _ptr(vertex_rank), _ptr(out_v), _ptr(out_c), n_v, _ptr(out_f), n_f, _stream()))

    out["select_compact_ms"] = _time(select_compact, reps)
    out["filter_ms"] = _time(lambda: mesh.filter_components(vertices, colours, faces, keep_largest=1), reps)
    if with_scipy:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        f = faces.cpu().numpy().astype(np.int64)
        f = f[classify(f, m)[0]]
        build, label = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
            graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(m, m)).tocsr()
            t1 = time.perf_counter()
            n, part = connected_components(graph, directed=False)
            t2 = time.perf_counter()
            build.append((t1 - t0) * 1e3)
            label.append((t2 - t1) * 1e3)
        out["scipy_graph_ms"], out["scipy_label_ms"], out["scipy_components"] = min(build), min(label), int(n)
        isolated = int((np.bincount(f.reshape(-1), minlength=m) == 0).sum())
        assert n - isolated == out["components"], (n, isolated, out["components"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--sparse_voxel", type=float, default=0.0075)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no_sparse", action="store_true")
    ap.add_argument("--no_scipy", action="store_true")
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
    out[f"room_dense_{dim}"] = stages(*vol.extract_mesh(2.0), a.reps, not a.no_scipy)
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
        out[f"room_sparse_{sv}"] = stages(*mesh_, a.reps, not a.no_scipy)
    faces, m = MC.strip(200_000, "random")
    sv_, sc_ = MC.attributes(m)
    out["strip_random"] = stages(torch.from_numpy(sv_).cuda(), torch.from_numpy(sc_).cuda(), torch.from_numpy(faces).cuda(), a.reps, not a.no_scipy)
    print(json.dumps({key: ({k: (float(f"{x:.4g}") if isinstance(x, float) else x) for k, x in val.items()} if isinstance(val, dict) else val)
                      for key, val in out.items()}))


if __name__ == "__main__":
    main()
