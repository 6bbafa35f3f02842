"""Distances between a reconstructed point cloud and a ground-truth cloud, and the Tanks-and-Temples scores built on them:
precision, recall and F-score per distance threshold (include/acez.h section N; eval_geometry.py is the
command line).

    d2, index = nearest_distances(query, ref, radius=0.05)            # squared distance and index of the nearest ref within 5 cm
    small = voxel_downsample(points, voxel=0.01)
    res = evaluate_geometry(rec, gt, [0.01, 0.02, 0.05], transform=T)  # dict: precision, recall, fscore per threshold, ...

The clouds live in HBM; the grid cells, the nearest-neighbour search and the voxel means are HIP kernels
(acezero_amd/csrc/geometry_api.hip), sorting and prefix sums are torch's. There is no CPU fallback."""
import numpy as np
import torch

from . import _native as N
from .head import _ptr, _stream

MAX_DIM = 1024                      # cells per axis (section N)
MAX_CELLS = 2 ** 24
MARGIN = np.float32(1.0 + 2.0 ** -10)


def _no_cpu(what):
    return RuntimeError(f"{what} needs device tensors: the cloud distances are HIP kernels, there is no CPU path")


def _points(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _no_cpu(what)
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


def nearest_distances(query, ref, radius, cell=None):
    """For every query point [n,3] the nearest reference point [m,3] within `radius`: (d2 float32 [n], index int32 [n]), the squared
    distance (dx * dx + dy * dy) + dz * dz in fp32 and the reference's row; +inf and -1 where no reference is within the radius (or
    the query is not finite). Among references at the same d2 the lowest row wins: the result is that of a brute-force scan, bit for
    bit, whatever the grid. The grid covers the reference's bounding box with cells of radius * (1 + 2^-10), enlarged until it has
    at most 1024 cells per axis and 2^24 in all; `cell` sets the edge instead (tests)."""
    query, ref = _points(query, "nearest_distances"), _points(ref, "nearest_distances")
    if ref.device != query.device:
        raise ValueError("query and ref must be on the same device")
    r = np.float32(radius)
    if not (np.isfinite(r) and r > 0):
        raise ValueError(f"radius must be positive and finite, got {radius}")
    dev, n = query.device, query.shape[0]
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
    # queries ordered by the cell of their nearest point of the box, so that a wavefront's lanes share a neighbourhood
    t_lo, t_hi = torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)
    key = point_cells(torch.minimum(torch.maximum(query, t_lo), t_hi), lo, c, dims)
    q_order = torch.sort(key, stable=True).indices
    q_sorted = query[q_order].contiguous()
    d2_sorted = torch.empty(n, dtype=torch.float32, device=dev)
    index_sorted = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        N.check(N.lib().acez_geom_nearest(_ptr(ref_sorted), _ptr(ref_index), _ptr(cell_start), ref_sorted.shape[0], float(lo[0]), float(lo[1]),
                                          float(lo[2]), float(c), dims[0], dims[1], dims[2], _ptr(q_sorted), n, float(r), _ptr(d2_sorted),
                                          _ptr(index_sorted), _stream()))
    d2, index = torch.empty_like(d2_sorted), torch.empty_like(index_sorted)
    d2[q_order] = d2_sorted
    index[q_order] = index_sorted
    return d2, index


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
           "log_lines", "grid_dims", "point_cells"]
