"""The connected components of a triangle mesh, and the mesh without its small ones: the clean-up between fusion and scoring
(include/acez.h section P; clean_mesh.py is the command line, fuse_depth.py has the same three flags).

    labels = connected_components(faces, n_vertices)                 # int32 [m]: the smallest vertex id of every vertex's component
    faces_of, vertices_of = component_sizes(faces, labels)           # int32 [m] each, indexed by label
    vertices, colours, faces, info = filter_components(vertices, colours, faces, min_faces=100)
    vertices, colours, faces, info = filter_components(vertices, colours, faces, keep_largest=1)

The mesh lives in HBM; the labelling (a lock-free union-find), the counts, the face and vertex flags and the compaction are HIP kernels
(acezero_amd/csrc/mesh_api.hip); the selection from the counts, the sort behind keep_largest and the prefix sums are torch's, on the
device. Everything is integer arithmetic: the result is a function of the mesh alone. There is no CPU fallback."""
import math

import torch

from . import _native as N
from ._device import no_cpu, ptr as _ptr, stream as _stream

__all__ = ["connected_components", "component_sizes", "filter_components"]

HISTOGRAM_EDGES = (10, 100, 1000, 10000)     # info["size_histogram"]: the components of 1-9, 10-99, .. and 10000 or more faces
WHY = "mesh components are HIP kernels"      # there is no CPU path


def _faces(faces, what, why=WHY):
    if not torch.is_tensor(faces) or not faces.is_cuda:
        raise no_cpu(what, why)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{what}: expected int32 faces [k,3], got {faces.dtype} {tuple(faces.shape)}")
    return faces.contiguous()


def check_mesh(vertices, colours, faces, what, why):
    """(vertices float32 [m,3], colours uint8 [m,3] or None, faces int32 [k,3]), contiguous, or the error of the first rule broken:
    all of them device tensors, then the faces' type and shape, the vertices', the colours'."""
    if not all(torch.is_tensor(t) and t.is_cuda for t in (vertices, faces) + (() if colours is None else (colours,))):
        raise no_cpu(what, why)
    faces = _faces(faces, what, why)
    if vertices.ndim != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError(f"{what}: expected float32 vertices [m,3], got {vertices.dtype} {tuple(vertices.shape)}")
    if colours is not None and (colours.shape != vertices.shape or colours.dtype != torch.uint8):
        raise ValueError(f"{what}: expected uint8 colours {tuple(vertices.shape)}, got {colours.dtype} {tuple(colours.shape)}")
    return vertices.contiguous(), None if colours is None else colours.contiguous(), faces


def empty_mesh(device, with_colours):                # (vertices, colours or None, faces) of the mesh without a vertex
    return (torch.empty((0, 3), dtype=torch.float32, device=device), torch.empty((0, 3), dtype=torch.uint8, device=device) if with_colours else None,
            torch.empty((0, 3), dtype=torch.int32, device=device))


def compact_ranks(face_keep, vertex_used):
    """The compaction's first half, without a synchronisation: (face_rank, vertex_rank, n_faces, n_vertices) from the byte flags of the
    faces and of the vertices (at least one): their inclusive int32 prefix sums, and the rows that stay as int64 device scalars."""
    face_rank, vertex_rank = (torch.cumsum(flags, 0, dtype=torch.int32) for flags in (face_keep, vertex_used))
    n_faces = face_rank[-1].long() if face_keep.shape[0] else torch.zeros((), dtype=torch.int64, device=face_keep.device)
    return face_rank, vertex_rank, n_faces, vertex_rank[-1].long()


def compact(vertices, colours, faces, face_keep, face_rank, vertex_used, vertex_rank, n_faces, n_vertices):
    """The compaction's second half, the two counts on the host: the flagged rows in their order, the faces renamed (acez_mesh_compact)."""
    dev, m, k = vertices.device, vertices.shape[0], faces.shape[0]
    out_vertices = torch.empty((n_vertices, 3), dtype=torch.float32, device=dev)
    out_colours = None if colours is None else torch.empty((n_vertices, 3), dtype=torch.uint8, device=dev)
    out_faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    if n_vertices:                                                                   # else no face is kept: nothing to move
        with torch.cuda.device(dev):
            N.check(N.lib().acez_mesh_compact(_ptr(vertices), _ptr(colours), m, _ptr(faces), k, _ptr(face_keep), _ptr(face_rank), _ptr(vertex_used),
                                              _ptr(vertex_rank), _ptr(out_vertices), _ptr(out_colours), n_vertices, _ptr(out_faces), n_faces,
                                              _stream()))
    return out_vertices, out_colours, out_faces


def _label(faces, m):
    """(labels int32 [m], status int32 [1]) without a synchronisation."""
    labels = torch.empty(m, dtype=torch.int32, device=faces.device)
    status = torch.empty(1, dtype=torch.int32, device=faces.device)
    with torch.cuda.device(faces.device):
        N.check(N.lib().acez_mesh_components(_ptr(faces), faces.shape[0], m, _ptr(labels), _ptr(status), _stream()))
    return labels, status


def _check_status(status):
    if int(status) != 0:
        raise RuntimeError("the component labelling ran out of its loop bound, which no mesh can cause: the labels are not to be trusted")


def connected_components(faces, n_vertices):
    """int32 [n_vertices]: for every vertex the smallest vertex id of its component (itself, if no valid face holds it). faces int32
    [k,3] on the device; a face with an index outside 0 .. n_vertices - 1 or with two equal indices connects nothing."""
    faces = _faces(faces, "connected_components")
    m = int(n_vertices)
    if m < 0:
        raise ValueError("n_vertices must not be negative")
    if m == 0:
        return torch.empty(0, dtype=torch.int32, device=faces.device)
    labels, status = _label(faces, m)
    _check_status(status.item())
    return labels


def component_sizes(faces, labels):
    """(faces_of, vertices_of) int32 [m], indexed by label: the valid faces and the vertices of every component that has a valid
    face; 0 everywhere else."""
    faces = _faces(faces, "component_sizes")
    if not torch.is_tensor(labels) or not labels.is_cuda:
        raise no_cpu("component_sizes", WHY)
    if labels.ndim != 1 or labels.dtype != torch.int32:
        raise ValueError(f"component_sizes: expected int32 labels [m], got {labels.dtype} {tuple(labels.shape)}")
    labels = labels.contiguous()
    m = labels.shape[0]
    faces_of = torch.empty(m, dtype=torch.int32, device=faces.device)
    vertices_of = torch.empty(m, dtype=torch.int32, device=faces.device)
    if m:
        with torch.cuda.device(faces.device):
            N.check(N.lib().acez_mesh_component_counts(_ptr(faces), faces.shape[0], _ptr(labels), m, _ptr(faces_of), _ptr(vertices_of),
                                                       _stream()))
    return faces_of, vertices_of


def filter_components(vertices, colours, faces, min_faces=0, min_ratio=0.0, keep_largest=None):
    """The mesh without the components that fail a criterion: (vertices float32 [m',3], colours uint8 [m',3] or None, faces int32
    [k',3], info). A component is kept iff it has at least min_faces faces, and at least min_ratio times the largest component's, and
    is among the keep_largest largest (ties: the smaller label first); each criterion is off by default. Invalid and degenerate faces
    and the vertices no kept face uses are dropped in any case; what stays keeps its order. colours may be None. One host
    synchronisation. info: components, components_kept, faces_dropped, vertices_dropped, largest_component_faces, invalid_faces,
    degenerate_faces, size_histogram (the components found with 1-9, 10-99, 100-999, 1000-9999 and 10000 or more faces)."""
    _faces(faces, "filter_components")                                # the faces' shape is refused before anyone asks where the vertices live
    vertices, colours, faces = check_mesh(vertices, colours, faces, "filter_components", WHY)
    min_faces, min_ratio = int(min_faces), float(min_ratio)
    if min_faces < 0 or not math.isfinite(min_ratio) or min_ratio < 0.0 or (keep_largest is not None and int(keep_largest) < 0):
        raise ValueError("min_faces, min_ratio and keep_largest must not be negative, min_ratio finite")
    dev, m, k = faces.device, vertices.shape[0], faces.shape[0]
    if k == 0 or m == 0:
        info = dict(components=0, components_kept=0, faces_dropped=k, vertices_dropped=m, largest_component_faces=0,
                    invalid_faces=k if m == 0 else 0, degenerate_faces=0, size_histogram=[0] * (len(HISTOGRAM_EDGES) + 1))
        return (*empty_mesh(dev, colours is not None), info)
    labels, status = _label(faces, m)
    faces_of, vertices_of = component_sizes(faces, labels)
    exists = faces_of > 0
    largest = faces_of.max()
    keep = exists & (faces_of.long() >= min(min_faces, 2 ** 62)) &(faces_of.to(torch.float64) >= min_ratio * largest.to(torch.float64))
    if keep_largest is not None:
        order = torch.sort(faces_of, descending=True, stable=True).indices          # ties: the smaller label first
        rank = torch.empty(m, dtype=torch.int64, device=dev)
        rank[order] = torch.arange(m, dtype=torch.int64, device=dev)
        keep &= rank < int(keep_largest)
    keep = keep.to(torch.uint8)
    face_keep = torch.empty(k, dtype=torch.uint8, device=dev)
    vertex_used = torch.empty(m, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        N.check(N.lib().acez_mesh_select(_ptr(faces), k, _ptr(labels), m, _ptr(keep), _ptr(face_keep), _ptr(vertex_used), _stream()))
    face_rank, vertex_rank, d_n_f, d_n_v = compact_ranks(face_keep, vertex_used)
    invalid = ((faces < 0) | (faces >= m)).any(1)
    degenerate = ~invalid & ((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2]))
    n_f, n_v, bad, found, kept, most, n_invalid, n_degenerate, *at_least = torch.stack(
        [d_n_f, d_n_v, status[0].long(), exists.sum(), keep.sum(), largest.long(), invalid.sum(),
         degenerate.sum()] + [(faces_of >= t).sum() for t in HISTOGRAM_EDGES]).cpu().tolist()       # the one synchronisation
    _check_status(bad)
    out = compact(vertices, colours, faces, face_keep, face_rank, vertex_used, vertex_rank, n_f, n_v)
    info = dict(components=found, components_kept=kept, faces_dropped=k - n_f, vertices_dropped=m - n_v, largest_component_faces=most,
                invalid_faces=n_invalid, degenerate_faces=n_degenerate,
                size_histogram=[found - at_least[0]] + [a - b for a, b in zip(at_least, at_least[1:] + [0])])
    return (*out, info)
