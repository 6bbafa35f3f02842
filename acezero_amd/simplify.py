"""A mesh with fewer faces: quadric vertex clustering (include/acez.h section Q; simplify_mesh.py is the command
line, fuse_depth.py has --simplify_cell).

    vertices, colours, faces, info = simplify_mesh(vertices, colours, faces, cell=0.03)                  # placement="quadric"
    vertices, colours, faces, info = simplify_mesh(vertices, None, faces, cell=0.03, placement="mean")

The vertices of one grid cell of edge `cell` become one vertex: the minimiser of the summed plane quadrics of the faces around them
(walls stay flat, edges and corners stay sharp), or their mean. Faces whose corners fall into fewer than three cells disappear, and so
do duplicates. The mesh lives in HBM; the cell keys, the clusters, the face classes, the per-cluster sums with the 3 x 3 solve and the
duplicate flags are HIP kernels (acezero_amd/csrc/simplify_api.hip), the compaction is mesh.py's; the stable sorts, the prefix sums
and the segment searches between them are torch's, on the device. Every sum has a fixed order: the result is a function of the mesh
alone, bit for bit. There is no CPU fallback."""
import math

import torch

from . import _native as N
from ._device import ptr as _ptr, stream as _stream
from .mesh import check_mesh, compact, compact_ranks, empty_mesh

__all__ = ["simplify_mesh"]

PLACEMENTS = ("quadric", "mean")
NO_CELL = 2 ** 63 - 1                       # the key of a vertex that is not finite
INVALID, DEGENERATE, COLLAPSED, CANDIDATE = 0, 1, 2, 3


def _segments(sorted_ids, m):
    """int64 [m + 1]: where every id 0 .. m starts in the ascending int32 ids."""
    return torch.searchsorted(sorted_ids, torch.arange(m + 1, dtype=torch.int32, device=sorted_ids.device))


def simplify_mesh(vertices, colours, faces, cell, placement="quadric"):
    """The mesh with one vertex per occupied grid cell of edge `cell`: (vertices float32 [m',3], colours uint8 [m',3] or None, faces
    int32 [k',3], info). vertices float32 [m,3], colours uint8 [m,3] or None, faces int32 [k,3], all on the device. The grid starts at
    the component-wise minimum of the finite vertices. placement "quadric": the cell's vertex minimises the plane quadrics of the
    faces at its corners, moved from the mean only along the directions they determine, and is the mean where that fails (info
    ["fallbacks"]); "mean": the mean of the cell's vertices. A colour is the rounded mean. A face is kept iff its corners lie in three
    different cells and no earlier face has the same three cells in the same orientation; it is written with its smallest index
    first. Faces with an index out of range, with two equal indices or with a vertex that is not finite are dropped, and so are the
    cells no kept face uses; what stays keeps its order. Two host synchronisations: the bounds, the counts. info: clusters,
    vertices_in, faces_in, vertices_out, faces_out, invalid_faces, degenerate_faces, nonfinite_vertices, collapsed_faces,
    duplicate_faces, unused_clusters, fallbacks (output vertices placed at the mean for want of a usable quadric)."""
    what = "simplify_mesh"
    vertices, colours, faces = check_mesh(vertices, colours, faces, what, "the simplification is HIP kernels")
    cell = float(cell)
    if not (math.isfinite(cell) and cell > 0.0):
        raise ValueError(f"{what}: cell must be positive and finite")
    if placement not in PLACEMENTS:
        raise ValueError(f"{what}: placement must be one of {PLACEMENTS}")
    dev, m, k = vertices.device, vertices.shape[0], faces.shape[0]
    quadric = placement == "quadric"

    def empty(n_clusters, counts):
        info = dict(clusters=n_clusters, vertices_in=m, faces_in=k, vertices_out=0, faces_out=0, invalid_faces=0, degenerate_faces=0,
                    nonfinite_vertices=0, collapsed_faces=0, duplicate_faces=0, unused_clusters=n_clusters, fallbacks=0)
        info.update(counts)
        return (*empty_mesh(dev, colours is not None), info)

    if m == 0:
        return empty(0, dict(invalid_faces=k))
    lib = N.lib()
    finite = torch.isfinite(vertices).all(1, keepdim=True)
    inf = torch.tensor(math.inf, dtype=torch.float32, device=dev)
    bounds = torch.cat([torch.where(finite, vertices, inf).amin(0), torch.where(finite, vertices, -inf).amax(0)]).cpu().tolist()   # synchronises
    if not all(math.isfinite(b) for b in bounds):                                   # no finite vertex: every key is NO_CELL
        bounds = [0.0] * 6
    origin = bounds[:3]
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    vertex_cluster = torch.empty(m, dtype=torch.int32, device=dev)
    face_class = torch.empty(k, dtype=torch.uint8, device=dev)
    triples = torch.empty((k, 3), dtype=torch.int32, device=dev)
    corner_keys = torch.empty(3 * k, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        N.check(lib.acez_simplify_keys(_ptr(vertices), m, *bounds, cell, _ptr(keys), _stream()))
        sorted_keys, order = torch.sort(keys, stable=True)
        has_cell = sorted_keys != NO_CELL
        first = has_cell.clone()
        first[1:] &= sorted_keys[1:] != sorted_keys[:-1]
        cluster_sorted = torch.where(has_cell, torch.cumsum(first, 0, dtype=torch.int32) - 1, m).to(torch.int32)
        N.check(lib.acez_simplify_clusters(_ptr(order), _ptr(cluster_sorted), m, _ptr(vertex_cluster), _stream()))
        segments = _segments(cluster_sorted, m)
        N.check(lib.acez_simplify_faces(_ptr(faces), k, _ptr(vertex_cluster), m, _ptr(face_class), _ptr(triples), _ptr(corner_keys), _stream()))
        quadrics = None
        if quadric:
            sorted_corners, corner_order = torch.sort(corner_keys, stable=True)
            corner_segments = _segments(sorted_corners, m)
            quadrics = torch.empty((m, 9), dtype=torch.float64, device=dev)
            N.check(lib.acez_simplify_quadrics(_ptr(vertices), m, _ptr(faces), k, _ptr(sorted_keys), _ptr(segments), _ptr(corner_order),
                                               _ptr(corner_segments), *origin, cell, _ptr(quadrics), _stream()))
        positions = torch.empty((m, 3), dtype=torch.float32, device=dev)
        cluster_colours = None if colours is None else torch.empty((m, 3), dtype=torch.uint8, device=dev)
        fallback = torch.zeros(m, dtype=torch.uint8, device=dev)
        N.check(lib.acez_simplify_place(_ptr(vertices), _ptr(colours), m, _ptr(sorted_keys), _ptr(order), _ptr(segments), _ptr(quadrics), *origin,
                                        cell, _ptr(positions), _ptr(cluster_colours), _ptr(fallback), _stream()))
        # the faces by (first, second, third) of their triples, equal triples in input order: two stable sorts
        by_third = torch.sort(triples[:, 2], stable=True).indices
        pair = triples[:, 0].long() * (m + 1) + triples[:, 1].long()
        perm = by_third[torch.sort(pair[by_third], stable=True).indices].contiguous()
        face_keep = torch.empty(k, dtype=torch.uint8, device=dev)
        cluster_used = torch.empty(m, dtype=torch.uint8, device=dev)
        N.check(lib.acez_simplify_unique(_ptr(triples), _ptr(face_class), _ptr(perm), k, m, _ptr(face_keep), _ptr(cluster_used), _stream()))
    face_rank, cluster_rank, d_n_f, d_n_v = compact_ranks(face_keep, cluster_used)
    n_f, n_v, n_clusters, n_cells, n_invalid, n_degenerate, n_collapsed, n_candidates, n_fallbacks = torch.stack(
        [d_n_f, d_n_v, first.sum(), has_cell.sum()]
        + [(face_class == c).sum() for c in (INVALID, DEGENERATE, COLLAPSED, CANDIDATE)] + [(fallback & cluster_used).sum()]).cpu().tolist()   # synchronises
    counts = dict(invalid_faces=n_invalid, degenerate_faces=n_degenerate, nonfinite_vertices=m - n_cells, collapsed_faces=n_collapsed,
                  duplicate_faces=n_candidates - n_f)
    if n_f == 0:
        return empty(n_clusters, counts)
    out = compact(positions, cluster_colours, triples, face_keep, face_rank, cluster_used, cluster_rank, n_f, n_v)
    info = dict(clusters=n_clusters, vertices_in=m, faces_in=k, vertices_out=n_v, faces_out=n_f, unused_clusters=n_clusters - n_v,
                fallbacks=n_fallbacks, **counts)
    return (*out, info)
