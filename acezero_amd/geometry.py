"""Distances between a reconstructed point cloud and a ground-truth cloud, and the Tanks-and-Temples scores built on them:
precision, recall and F-score per distance threshold (include/acez.h section N; eval_geometry.py is the
command line).

    d2, index = nearest_distances(query, ref, radius=0.05)            # squared distance and index of the nearest ref within 5 cm
    small = voxel_downsample(points, voxel=0.01)
    res = evaluate_geometry(rec, gt, [0.01, 0.02, 0.05], transform=T)  # dict: precision, recall, fscore per threshold, ...
    T, info = icp_stage(src, tgt, radius=0.05)                         # one ICP stage from the identity, the loop on the device
    T, stages = refine_alignment(rec, gt, T0, distances=[0.2, 0.1, 0.05])  # coarse to fine, from the alignment T0
    points, face, colours, info = sample_mesh(vertices, faces, spacing=0.005)   # a mesh as its surface: section O, DESIGN 4n
    kept, dropped = crop_to_polygon(points, formats.read_crop_file(path))       # the volume of a Tanks and Temples crop file

The clouds live in HBM; the grid cells, the nearest-neighbour search, the voxel means and the ICP loop (the search with the
correspondence moments, the Umeyama solve) are HIP kernels (acezero_amd/csrc/geometry_api.hip), and so are the face counts, the
face samples and the polygon crop (acezero_amd/csrc/surface_api.hip); sorting and prefix sums are torch's.
There is no CPU fallback."""
import collections

import numpy as np
import torch

from . import _native as N
from ._device import no_cpu, ptr as _ptr, read_loops, stream as _stream

MAX_DIM = 1024                      # cells per axis (section N)
MAX_CELLS = 2 ** 24
MARGIN = np.float32(1.0 + 2.0 ** -10)
WHY = "the cloud distances are HIP kernels"


def _points(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise no_cpu(what, WHY)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"{what}: expected points [n,3], got {tuple(t.shape)}")
    return t.to(torch.float32).contiguous()


def grid_dims(lo, hi, c):
    """Cells per axis of the box lo .. hi (float32 [3] host arrays) at cell edge c, in the kernel's arithmetic: the cell of hi, + 1."""
    with np.errstate(over="ignore"):
        return [int(v) + 1 for v in np.floor((hi.astype(np.float32) - lo.astype(np.float32)) / np.float32(c)).astype(np.float64)]


def _fits(dims):
    return max(dims) <= MAX_DIM and dims[0] * dims[1] * dims[2] <= MAX_CELLS


def _bounds(points):
    """(lo, hi) float32 [3] host arrays over the points with finite coordinates; None if there is none."""
    finite = points[torch.isfinite(points).all(1)]
    if finite.shape[0] == 0:
        return None
    return finite.min(0).values.cpu().numpy(), finite.max(0).values.cpu().numpy()


def point_cells(points, origin, c, dims):
    """int32 [n]: the linear grid cell of every point, -1 outside the grid or not finite (acez_geom_cells)."""
    out = torch.empty(points.shape[0], dtype=torch.int32, device=points.device)
    with torch.cuda.device(points.device):
        N.check(N.lib().acez_geom_cells(_ptr(points), points.shape[0], float(origin[0]), float(origin[1]), float(origin[2]), float(c),
                                        int(dims[0]), int(dims[1]), int(dims[2]), _ptr(out), _stream()))
    return out


Grid = collections.namedtuple("Grid", "ref_sorted ref_index cell_start origin cell dims hi")


def build_grid(ref, radius, cell=None):
    """The grid of section N over the reference cloud (a float32 [m,3] device tensor): Grid(ref_sorted, ref_index, cell_start, origin,
    cell, dims, hi) -- the references sorted by cell (stable; those that are not finite dropped), their original rows (int32), the
    first sorted position of every cell (int32 [cells + 1]), the box's minimum (float32 [3] host array), the cell edge (float32), the
    cells per axis, and the box's maximum. The cell edge is radius * (1 + 2^-10), enlarged until the grid has at most 1024 cells per
    axis and 2^24 in all; `cell` sets the edge instead."""
    ref, r = _points(ref, "build_grid"), _radius(radius)
    dev = ref.device
    box = _bounds(ref)
    lo, hi = box if box is not None else (np.zeros(3, np.float32), np.zeros(3, np.float32))
    with np.errstate(over="ignore"):
        if not np.isfinite(hi - lo).all():
            raise ValueError("the reference cloud's extent overflows float32")
    if cell is None:
        c = r * MARGIN
        while not _fits(grid_dims(lo, hi, c)):
            c = np.float32(c * np.float32(1.125))
    else:
        c = np.float32(cell)
        if not _fits(grid_dims(lo, hi, c)):
            raise ValueError(f"cell {cell} gives a grid of {grid_dims(lo, hi, c)} cells: more than {MAX_DIM} per axis or {MAX_CELLS} in all")
    dims = grid_dims(lo, hi, c)
    n_cells = dims[0] * dims[1] * dims[2]
    # the grid: references sorted by cell (stable), their rows, and the first sorted position of every cell
    cells = point_cells(ref, lo, c, dims)
    rows = torch.nonzero(cells >= 0).reshape(-1)                   # drops the references that are not finite: nothing is near them
    order = torch.sort(cells[rows], stable=True)
    rows = rows[order.indices]
    ref_sorted, ref_index = ref[rows].contiguous(), rows.to(torch.int32)
    cell_start = torch.zeros(n_cells + 1, dtype=torch.int32, device=dev)
    if rows.shape[0]:
        cell_start[1:] = torch.cumsum(torch.bincount(order.values.long(), minlength=n_cells), 0).to(torch.int32)
    return Grid(ref_sorted, ref_index, cell_start, lo, c, dims, hi)


def order_by_cell(points, grid):
    """int64 [n]: the stable order of the points by the cell of their nearest point of the grid's box, so that a wavefront's lanes
    share a neighbourhood."""
    points = _points(points, "order_by_cell")
    dev = points.device
    t_lo, t_hi = torch.from_numpy(grid.origin).to(dev), torch.from_numpy(grid.hi).to(dev)
    key = point_cells(torch.minimum(torch.maximum(points, t_lo), t_hi), grid.origin, grid.cell, grid.dims)
    return torch.sort(key, stable=True).indices


def _radius(radius):
    r = np.float32(radius)
    if not (np.isfinite(r) and r > 0):
        raise ValueError(f"radius must be positive and finite, got {radius}")
    return r


def nearest_distances(query, ref, radius, cell=None):
    """For every query point [n,3] the nearest reference point [m,3] within `radius`: (d2 float32 [n], index int32 [n]), the squared
    distance (dx * dx + dy * dy) + dz * dz in fp32 and the reference's row; +inf and -1 where no reference is within the radius (or
    the query is not finite). Among references at the same d2 the lowest row wins: the result is that of a brute-force scan, bit for
    bit, whatever the grid. The grid covers the reference's bounding box with cells of radius * (1 + 2^-10), enlarged until it has
    at most 1024 cells per axis and 2^24 in all; `cell` sets the edge instead (tests)."""
    query, ref = _points(query, "nearest_distances"), _points(ref, "nearest_distances")
    if ref.device != query.device:
        raise ValueError("query and ref must be on the same device")
    r = _radius(radius)
    dev, n = query.device, query.shape[0]
    g = build_grid(ref, r, cell)
    lo, c, dims = g.origin, g.cell, g.dims
    # queries ordered by the cell of their nearest point of the box, so that a wavefront's lanes share a neighbourhood
    q_order = order_by_cell(query, g)
    q_sorted = query[q_order].contiguous()
    d2_sorted = torch.empty(n, dtype=torch.float32, device=dev)
    index_sorted = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        N.check(N.lib().acez_geom_nearest(_ptr(g.ref_sorted), _ptr(g.ref_index), _ptr(g.cell_start), g.ref_sorted.shape[0], float(lo[0]),
                                          float(lo[1]), float(lo[2]), float(c), dims[0], dims[1], dims[2], _ptr(q_sorted), n, float(r),
                                          _ptr(d2_sorted), _ptr(index_sorted), _stream()))
    d2, index = torch.empty_like(d2_sorted), torch.empty_like(index_sorted)
    d2[q_order] = d2_sorted
    index[q_order] = index_sorted
    return d2, index


ICP_TILE, ICP_TERMS, ICP_STATE, ICP_RECORD = 256, 18, 34, 16           # include/acez.h section N
ICP_STATUS = {0: "max_iterations", 1: "converged", 2: "degenerate"}     # a loop still running after the last pair ran out


def icp_stage(src, tgt, radius, *, max_iterations=30, with_scale=False, rel_fitness=1e-6, rel_rmse=1e-6, cell=None):
    """One ICP stage from the identity (include/acez.h section N, ICP): the similarity T (4 x 4 float64) that brings the source cloud
    [n,3] onto the target cloud [m,3] by iterated closest points within `radius`, rigid or with_scale, and an info dict: status
    ("converged": fitness and rmse both moved less than rel_fitness / rel_rmse; "max_iterations"; "degenerate": fewer than three
    or collinear correspondences, T is then the last well-determined one), iterations, and per iteration fitness (the share of
    sources with a target within the radius), rmse (over those), count, sum_d2 and transforms (the T the iteration searched under).
    The target grid is built once, the sources are ordered by cell once, and the max_iterations ACCUMULATE + UPDATE launches are
    enqueued back to back on the current stream: the loop's state lives on the device, launches after it has stopped return at
    once, and the host reads state and history back once."""
    src, tgt = _points(src, "icp_stage"), _points(tgt, "icp_stage")
    if src.device != tgt.device:
        raise ValueError("src and tgt must be on the same device")
    r = _radius(radius)
    max_iterations = int(max_iterations)
    if max_iterations < 1:
        raise ValueError("max_iterations must be at least 1")
    if not all(np.isfinite(v) and v >= 0 for v in (rel_fitness, rel_rmse)):
        raise ValueError("rel_fitness and rel_rmse must be finite and not negative")
    dev, n = src.device, src.shape[0]
    if n == 0:
        raise ValueError("the source cloud is empty")
    g = build_grid(tgt, r, cell)
    lo, c, dims = g.origin, g.cell, g.dims
    pivot = (g.origin + g.hi) * np.float32(0.5)
    pivot = [float(v) if np.isfinite(v) else 0.0 for v in pivot]
    src_sorted = src[order_by_cell(src, g)].contiguous()
    state = torch.zeros(ICP_STATE, dtype=torch.float64, device=dev)
    state[[0, 5, 10]] = 1.0
    partials = torch.empty(((n + ICP_TILE - 1) // ICP_TILE, ICP_TERMS), dtype=torch.float64, device=dev)
    history = torch.zeros((max_iterations, ICP_RECORD), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        lib, stream = N.lib(), _stream()
        for _ in range(max_iterations):                            # no synchronisation in between
            N.check(lib.acez_geom_icp_accumulate(_ptr(g.ref_sorted), _ptr(g.ref_index), _ptr(g.cell_start), g.ref_sorted.shape[0], float(lo[0]),
                                                 float(lo[1]), float(lo[2]), float(c), dims[0], dims[1], dims[2], _ptr(src_sorted), n, float(r),
                                                 pivot[0], pivot[1], pivot[2], _ptr(state), _ptr(partials), stream))
            N.check(lib.acez_geom_icp_update(_ptr(partials), n, pivot[0], pivot[1], pivot[2], int(bool(with_scale)), float(rel_fitness),
                                             float(rel_rmse), max_iterations, _ptr(state), _ptr(history), stream))
    (state_h,), (history_h,), (status,), (done,) = read_loops([state[None]], [history[None]])      # the one read-back
    T = np.eye(4)
    T[:3] = state_h[:12].reshape(3, 4)
    info = {"status": ICP_STATUS[status], "iterations": int(done), "fitness": [float(v) for v in history_h[:done, 14]],
            "rmse": [float(v) for v in history_h[:done, 15]], "count": [int(v) for v in history_h[:done, 12]],
            "sum_d2": [float(v) for v in history_h[:done, 13]],
            "transforms": [np.vstack([history_h[k, :12].reshape(3, 4), [0.0, 0.0, 0.0, 1.0]]) for k in range(done)]}
    return T, info


def refine_alignment(rec, gt, transform=None, *, distances, voxels=None, max_iterations=30, with_scale=False):
    """Refine the similarity `transform` (4 x 4, reconstruction -> ground truth; None: the identity) by ICP, coarse to fine as Tanks
    and Temples does after its trajectory alignment: one icp_stage per search radius of `distances`, on the clouds downsampled to
    voxels[k] where that is given. Stage k takes apply_similarity(rec, T) under the alignment found so far, runs from the identity
    and composes T <- T_stage T. A degenerate stage keeps the alignment it started with (its info says "kept_previous": True).
    Returns (T 4 x 4 float64, the list of stage infos: icp_stage's, plus distance, voxel, kept_previous)."""
    rec, gt = _points(rec, "refine_alignment"), _points(gt, "refine_alignment")
    distances = [float(d) for d in distances]
    if not distances or not all(np.isfinite(d) and d > 0 for d in distances):
        raise ValueError("distances must be positive numbers, at least one")
    voxels = [None] * len(distances) if voxels is None else [None if v is None else float(v) for v in voxels]
    if len(voxels) != len(distances):
        raise ValueError(f"{len(voxels)} voxel sizes for {len(distances)} distances: one per stage")
    T = np.eye(4) if transform is None else np.array(transform, np.float64).reshape(4, 4)
    infos = []
    for d, v in zip(distances, voxels):
        moved, target = apply_similarity(rec, T), gt
        if v is not None:
            moved, target = voxel_downsample(moved, v), voxel_downsample(target, v)
        T_stage, info = icp_stage(moved, target, d, max_iterations=max_iterations, with_scale=with_scale)
        info.update(distance=d, voxel=v, kept_previous=info["status"] == "degenerate")
        if not info["kept_previous"]:
            T = T_stage @ T
        infos.append(info)
    return T, infos


def voxel_downsample(points, voxel):
    """The Tanks-and-Temples downsample: one point per occupied voxel of edge `voxel`, the mean of the voxel's points (float32
    [s,3], in ascending voxel order; the sums run in the points' order). Voxel (0,0,0)'s corner is the cloud's minimum; points that
    are not finite are dropped. The voxel grid obeys the limits of section N: at most 1024 voxels per axis and 2^24 in all."""
    points = _points(points, "voxel_downsample")
    v = np.float32(voxel)
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f"voxel must be positive and finite, got {voxel}")
    box = _bounds(points)
    if box is None:
        return torch.empty((0, 3), dtype=torch.float32, device=points.device)
    dims = grid_dims(box[0], box[1], v)
    if not _fits(dims):
        raise ValueError(f"voxel {voxel} gives {dims[0]} x {dims[1]} x {dims[2]} voxels over the cloud's box: more than {MAX_DIM} per axis "
                         f"or {MAX_CELLS} in all; use a larger voxel or crop the cloud")
    cells = point_cells(points, box[0], v, dims)
    rows = torch.nonzero(cells >= 0).reshape(-1)
    order = torch.sort(cells[rows], stable=True)
    ordered = points[rows[order.indices]].contiguous()
    _, counts = torch.unique_consecutive(order.values, return_counts=True)
    start = torch.zeros(counts.shape[0] + 1, dtype=torch.int32, device=points.device)
    start[1:] = torch.cumsum(counts, 0).to(torch.int32)
    out = torch.empty((counts.shape[0], 3), dtype=torch.float32, device=points.device)
    with torch.cuda.device(points.device):
        N.check(N.lib().acez_geom_voxel_means(_ptr(ordered), ordered.shape[0], _ptr(start), counts.shape[0], _ptr(out), _stream()))
    return out


def apply_similarity(points, transform):
    """float32 [n,3]: T (4 x 4, rows 0 .. 2 used) applied to float32 points in float64, x' = ((T00 x + T01 y) + T02 z) + T03, rounded
    to float32 once."""
    T = np.asarray(transform, np.float64).reshape(4, 4)
    p = points.to(torch.float64)
    cols = [((float(T[r, 0]) * p[:, 0] + float(T[r, 1]) * p[:, 1]) + float(T[r, 2]) * p[:, 2]) + float(T[r, 3]) for r in range(3)]
    return torch.stack(cols, 1).to(torch.float32)


def fscore(precision, recall):
    return 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0


def crop_to_box(rec, gt, margin):
    """(the points of rec inside gt's bounding box enlarged by `margin` on every side, the number dropped); float32 comparisons, so a
    point that is not finite is dropped. Tensors on any one device."""
    finite = gt[torch.isfinite(gt).all(1)]
    if finite.shape[0] == 0:
        return rec, 0
    lo, hi = finite.min(0).values - np.float32(margin), finite.max(0).values + np.float32(margin)
    keep = ((rec >= lo) & (rec <= hi)).all(1)
    return rec[keep].contiguous(), int(rec.shape[0] - int(keep.sum().item()))


def scores(d2_rec, d2_gt, thresholds, max_distance):
    """The scores from the two directed searches' squared distances (float32 host arrays, +inf = nothing within max_distance): per
    threshold the counts with d2 <= float32(t)^2, precision, recall and fscore as Python floats from the integer counts; mean and
    median (element n // 2 of the sorted values, evaluate.median_of_sorted's convention) of the distances clipped to max_distance."""
    d2_rec, d2_gt = np.asarray(d2_rec, np.float32), np.asarray(d2_gt, np.float32)
    n_rec, n_gt = len(d2_rec), len(d2_gt)
    res = dict(rec_within=[], gt_within=[], precision=[], recall=[], fscore=[])
    for t in thresholds:
        t2 = np.float32(t) * np.float32(t)
        a, b = int((d2_rec <= t2).sum()), int((d2_gt <= t2).sum())
        res["rec_within"].append(a)
        res["gt_within"].append(b)
        res["precision"].append(a / n_rec)
        res["recall"].append(b / n_gt)
        res["fscore"].append(fscore(a / n_rec, b / n_gt))
    r2 = np.float32(max_distance) * np.float32(max_distance)
    for name, d2 in (("accuracy", d2_rec), ("completeness", d2_gt)):
        d = np.sort(np.sqrt(np.minimum(d2, r2).astype(np.float64)))
        res[name + "_mean"], res[name + "_median"] = float(d.mean()), float(d[len(d) // 2])
    return res


def evaluate_geometry(rec, gt, thresholds, *, transform=None, voxel=None, crop=True, max_distance=None):
    """Score the reconstructed cloud `rec` against the ground truth `gt` (device tensors [n,3], metres). transform: 4 x 4 similarity
    from the reconstruction's frame to the ground truth's; voxel: downsample both clouds first; crop: drop reconstruction points
    outside the ground truth's bounding box enlarged by max_distance; max_distance: search radius, default the largest threshold.
    Per threshold t: precision = share of reconstruction points with a ground-truth point within t (d2 <= float32(t)^2), recall =
    the same from ground truth to reconstruction, fscore = 2PR / (P + R). Accuracy / completeness: mean and median of the distances
    rec -> gt / gt -> rec, clipped to max_distance (scores()). Returns a dict of Python numbers."""
    rec, gt = _points(rec, "evaluate_geometry"), _points(gt, "evaluate_geometry")
    thresholds = [float(t) for t in thresholds]
    if not thresholds or not all(np.isfinite(t) and t > 0 for t in thresholds):
        raise ValueError("thresholds must be positive numbers, at least one")
    r = float(max(thresholds) if max_distance is None else max_distance)
    if not (np.isfinite(r) and r > 0):
        raise ValueError("max_distance must be positive and finite")
    res = {"rec_points_read": int(rec.shape[0]), "gt_points_read": int(gt.shape[0]), "max_distance": r, "voxel": voxel}
    if transform is not None:
        rec = apply_similarity(rec, transform)
    if voxel is not None:
        rec, gt = voxel_downsample(rec, voxel), voxel_downsample(gt, voxel)
    dropped = 0
    if crop:
        rec, dropped = crop_to_box(rec, gt, r)
    if gt.shape[0] == 0:
        raise ValueError("the ground-truth cloud is empty")
    if rec.shape[0] == 0:
        raise ValueError("the reconstruction is empty" + (f" after cropping to the ground truth's box ({dropped} points dropped): are the "
                                                          "clouds in the same frame?" if dropped else ""))
    d2_rec, _ = nearest_distances(rec, gt, r)
    d2_gt, _ = nearest_distances(gt, rec, r)
    res.update(rec_points=int(rec.shape[0]), gt_points=int(gt.shape[0]), dropped=dropped, thresholds=thresholds)
    res.update(scores(d2_rec.cpu().numpy(), d2_gt.cpu().numpy(), thresholds, r))
    return res


# ------------------------------------------------------------------------------------- surfaces (include/acez.h section O)
MAX_SAMPLES = 2 ** 31 - 1


def sample_density(spacing):
    """Samples per square metre at `spacing` metres between samples: 1 / spacing^2 in float64, the product first."""
    s = float(spacing)
    if not (np.isfinite(s) and s > 0):
        raise ValueError(f"spacing must be positive and finite, got {spacing}")
    if s * s == 0.0 or 1.0 / (s * s) == 0.0:
        raise ValueError(f"spacing {spacing}: its square or the density 1 / spacing^2 is outside float64's range")
    return 1.0 / (s * s)


def sample_mesh(vertices, faces, *, spacing, seed=0, colours=None):
    """Sample the surface of a triangle mesh at about one point per spacing x spacing (include/acez.h section O): vertices float32
    [m,3] and faces int32 [k,3] device tensors, colours uint8 [m,3] or None. Every face draws its own number of samples, floor(area /
    spacing^2) plus one more with the probability of the remainder, and its own uniform samples, from a counter-based stream keyed by
    (seed, face): the result is a function of the mesh, the spacing and the seed alone. Returns (points float32 [n,3], face_index
    int32 [n], colours uint8 [n,3] or None, info): the samples in face order, and info = dict(faces, faces_invalid (an index outside
    the vertices, or an area that is not finite: no samples), area (the valid faces' areas, summed in face order by math.fsum),
    samples). ValueError if the mesh asks for more than 2^31 - 1 samples."""
    import math
    vertices = _points(vertices, "sample_mesh")
    dev = vertices.device
    if not torch.is_tensor(faces) or faces.device != dev:
        raise no_cpu("sample_mesh", WHY)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"sample_mesh: expected integer faces [k,3], got {faces.dtype} {tuple(faces.shape)}")
    faces = faces.to(torch.int32).contiguous()
    if colours is not None:
        if not torch.is_tensor(colours) or colours.device != dev:
            raise no_cpu("sample_mesh", WHY)
        if colours.dtype != torch.uint8 or tuple(colours.shape) != tuple(vertices.shape):
            raise ValueError(f"sample_mesh: expected uint8 colours {tuple(vertices.shape)}, got {colours.dtype} {tuple(colours.shape)}")
        colours = colours.contiguous()
    density, seed = sample_density(spacing), int(seed) & (2 ** 64 - 1)
    m, k = vertices.shape[0], faces.shape[0]
    counts = torch.empty(k, dtype=torch.int32, device=dev)
    areas = torch.empty(k, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        N.check(N.lib().acez_geom_face_counts(_ptr(vertices), m, _ptr(faces), k, density, seed, _ptr(counts), _ptr(areas), _stream()))
    offsets = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)       # the one scan: over integers
    areas_h = areas.cpu().numpy()
    n = int(offsets[-1].item())
    info = {"faces": k, "faces_invalid": int((areas_h < 0).sum()), "area": math.fsum(areas_h[areas_h >= 0].tolist()), "samples": n}
    if n > MAX_SAMPLES:
        raise ValueError(f"spacing {spacing} asks for {n} samples of {info['area']:.6g} m^2, more than 2^31 - 1: use a larger spacing")
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    face_index = torch.empty(n, dtype=torch.int32, device=dev)
    out_colours = None if colours is None else torch.empty((n, 3), dtype=torch.uint8, device=dev)
    if n:
        with torch.cuda.device(dev):
            N.check(N.lib().acez_geom_sample_faces(_ptr(vertices), m, _ptr(faces), k, _ptr(offsets), n, seed,
                                                   None if colours is None else _ptr(colours), _ptr(points), _ptr(face_index),
                                                   None if colours is None else _ptr(out_colours), _stream()))
    return points, face_index, out_colours, info


def polygon_mask(points, crop):
    """bool [n]: the points inside the volume `crop` (a formats.CropVolume, read_crop_file's result): finite, axis_min <= w <= axis_max, and inside the
    polygon by the crossing rule of include/acez.h section O (acez_geom_crop_polygon)."""
    points = _points(points, "crop_to_polygon")
    polygon = np.ascontiguousarray(np.asarray(crop.polygon, np.float32).reshape(-1, 2))
    if not np.isfinite(polygon).all():
        raise ValueError("the crop polygon has a corner that is not finite")
    keep = torch.empty(points.shape[0], dtype=torch.uint8, device=points.device)
    poly_d = torch.from_numpy(polygon).to(points.device)
    with torch.cuda.device(points.device):
        N.check(N.lib().acez_geom_crop_polygon(_ptr(points), points.shape[0], _ptr(poly_d), polygon.shape[0], int(crop.axis),
                                               float(np.float32(crop.axis_min)), float(np.float32(crop.axis_max)), _ptr(keep), _stream()))
    return keep.bool()


def crop_to_polygon(points, crop):
    """(the points inside the crop volume, the number dropped): polygon_mask's points, compacted by torch as in crop_to_box."""
    points = _points(points, "crop_to_polygon")
    keep = polygon_mask(points, crop)
    return points[keep].contiguous(), int(points.shape[0] - int(keep.sum().item()))


def score_reconstruction(rec, gt, thresholds, *, rec_faces=None, rec_colours=None, gt_faces=None, transform=None, sample_spacing=None,
                         gt_sample_spacing=None, sample_seed=0, crop_volume=None, crop_ground_truth=False, icp_distances=None,
                         icp_voxels=None, icp_max_iterations=30, icp_scale=False, voxel=None, crop=True, max_distance=None):
    """eval_geometry.py's pipeline on device tensors, in the order of DESIGN.md section 4n. Points (no spacing, no crop_volume): ICP
    (icp_distances given) starts from `transform`, evaluate_geometry applies the result. A surface: move the vertices by `transform`,
    sample the faces (rec_faces / gt_faces at their spacing), drop what lies outside crop_volume (a formats.CropVolume; with
    crop_ground_truth the ground truth's points too), ICP from the identity, then voxel, box crop and search in evaluate_geometry.
    Returns (res, points, colours): evaluate_geometry's dict with `transform` (file frame -> ground truth: T_icp T_initial; rows of
    floats or None) and, where they apply, `sampling`, `crop_file`, `transform_initial` and `icp` (the stage infos without their
    matrices), as eval_geometry.py --output_json holds them; the reconstruction's points as they are scored (sampled, cropped by the
    polygon, under the final alignment) and their colours (None without rec_colours). ValueError if a cloud ends up empty."""
    initial = None if transform is None else np.array(transform, np.float64).reshape(4, 4)
    surface = sample_spacing is not None or gt_sample_spacing is not None or crop_volume is not None
    T, colours = initial, rec_colours                                # T: what is still to be applied to rec
    sampling = crop_info = stages = None
    try:
        if surface:
            if T is not None:
                rec = apply_similarity(rec, T)
            T = None
            if sample_spacing is not None or gt_sample_spacing is not None:
                sampling = {"seed": sample_seed}
            if sample_spacing is not None:
                rec, _, colours, info = sample_mesh(rec, rec_faces, spacing=sample_spacing, seed=sample_seed, colours=colours)
                sampling.update(spacing=sample_spacing, **info)
            if gt_sample_spacing is not None:
                gt, _, _, info = sample_mesh(gt, gt_faces, spacing=gt_sample_spacing, seed=sample_seed)
                sampling.update(gt_spacing=gt_sample_spacing, **{"gt_" + k: v for k, v in info.items()})
            if crop_volume is not None:
                keep = polygon_mask(rec, crop_volume)
                crop_info = {"orthogonal_axis": "XYZ"[crop_volume.axis], "corners": int(len(crop_volume.polygon)),
                             "axis_min": float(crop_volume.axis_min), "axis_max": float(crop_volume.axis_max),
                             "dropped": int(rec.shape[0] - int(keep.sum().item()))}
                rec = rec[keep].contiguous()
                if colours is not None:
                    colours = colours[keep].contiguous()
                if crop_ground_truth:
                    gt, crop_info["gt_dropped"] = crop_to_polygon(gt, crop_volume)
                if rec.shape[0] == 0:
                    raise ValueError(f"the reconstruction is empty after the crop file's polygon ({crop_info['dropped']} points dropped): "
                                     "are the clouds in the same frame?")
        if icp_distances is not None:
            T, stages = refine_alignment(rec, gt, T, distances=icp_distances, voxels=icp_voxels, max_iterations=icp_max_iterations,
                                         with_scale=icp_scale)
        res = evaluate_geometry(rec, gt, thresholds, transform=T, voxel=voxel, crop=crop, max_distance=max_distance)
    except ValueError as e:
        raise ValueError(str(e) + (f" (the crop file's polygon dropped {crop_info['dropped']} points before)"
                                   if crop_info is not None and "crop file" not in str(e) and "is empty" in str(e) else ""))
    points = rec if T is None else apply_similarity(rec, T)
    if surface and initial is not None:                              # what is reported maps the file's frame: T_icp T_initial
        T = initial if T is None else T @ initial
    rows = lambda M: None if M is None else [[float(x) for x in row] for row in M]
    res["transform"] = rows(T)
    if sampling is not None:
        res["sampling"] = sampling
    if crop_info is not None:
        res["crop_file"] = crop_info
    if stages is not None:
        res["transform_initial"] = rows(initial)
        res["icp"] = [{k: v for k, v in stage.items() if k != "transforms"} for stage in stages]
    return res, points, colours


def log_lines(res):
    """The summary eval_geometry.py logs: the counts, then one line per threshold."""
    lines = [f"Reconstruction: {res['rec_points']} points ({res['rec_points_read']} read, {res['dropped']} dropped outside the ground "
             f"truth's box). Ground truth: {res['gt_points']} points ({res['gt_points_read']} read).",
             f"Accuracy (rec -> gt, clipped to {res['max_distance']} m): mean {res['accuracy_mean'] * 1000:.2f} mm, median "
             f"{res['accuracy_median'] * 1000:.2f} mm. Completeness (gt -> rec): mean {res['completeness_mean'] * 1000:.2f} mm, median "
             f"{res['completeness_median'] * 1000:.2f} mm."]
    for k, t in enumerate(res["thresholds"]):
        lines.append(f"Threshold {t} m: precision {res['precision'][k] * 100:.2f}%, recall {res['recall'][k] * 100:.2f}%, "
                     f"F-score {res['fscore'][k] * 100:.2f}%")
    return lines


__all__ = ["nearest_distances", "voxel_downsample", "evaluate_geometry", "apply_similarity", "crop_to_box", "scores", "fscore",
           "log_lines", "grid_dims", "point_cells", "build_grid", "order_by_cell", "icp_stage", "refine_alignment", "sample_mesh",
           "sample_density", "crop_to_polygon", "polygon_mask", "score_reconstruction"]
