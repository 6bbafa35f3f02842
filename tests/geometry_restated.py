"""include/acez.h section N and acezero_amd/geometry.py restated in numpy: the grid cell of a point, the nearest reference within a
radius as a brute-force scan in float32, the voxel downsample and the precision / recall / F-score arithmetic. A helper module, not
a test file; tests/test_geometry_cpu.py checks it against scipy's k-d tree, tests/test_geometry_gpu.py compares the kernels with it
bit for bit. Nothing here imports acezero_amd.geometry."""
import numpy as np

F = np.float32


def cells(points, origin, c, dims):
    """int32 [n]: (k * ny + j) * nx + i with i = floor((x - ox) / c) in float32, -1 if out of range or not finite."""
    p = np.asarray(points, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        f = np.floor((p - np.asarray(origin, F)[None, :]) / F(c))
    n = np.asarray(dims, np.float64)[None, :]
    ok = (np.isfinite(p) & (f >= 0) & (f < n)).all(1)
    ijk = np.where(ok[:, None], f, 0).astype(np.int64)
    lin = (ijk[:, 2] * int(dims[1]) + ijk[:, 1]) * int(dims[0]) + ijk[:, 0]
    return np.where(ok, lin, -1).astype(np.int32)


def nearest(query, ref, radius, chunk=256):
    """(d2 float32 [n], index int32 [n]): over ALL references, d2 = (dx * dx + dy * dy) + dz * dz in float32 with dx = qx - px; the
    smallest d2 with d2 <= radius * radius and the lowest index that attains it; +inf and -1 if there is none."""
    q, p = np.asarray(query, F).reshape(-1, 3), np.asarray(ref, F).reshape(-1, 3)
    r2 = F(radius) * F(radius)
    d2_out, idx_out = np.full(len(q), np.inf, F), np.full(len(q), -1, np.int32)
    if len(p) == 0:
        return d2_out, idx_out
    for lo in range(0, len(q), chunk):
        part = q[lo:lo + chunk]
        with np.errstate(all="ignore"):
            dx, dy, dz = (part[:, None, a] - p[None, :, a] for a in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F
            d2 = np.where(d2 <= r2, d2, F(np.inf))                # NaN fails the comparison
        best = d2.min(1)
        first = (d2 == best[:, None]).argmax(1)                   # the lowest index among the minima
        found = np.isfinite(best)
        d2_out[lo:lo + chunk] = best
        idx_out[lo:lo + chunk] = np.where(found, first, -1)
    return d2_out, idx_out


def nearest_d2_tree(query, ref, radius, k=16):
    """nearest()'s d2 for clouds too large to scan: the float32 d2 of the k nearest references by a float64 k-d tree, and their
    minimum. Asserts what makes that the scan's result: the k-th candidate is farther than the minimum by more than float32 rounding
    (or there are fewer than k candidates), so no reference outside the candidates can attain the float32 minimum."""
    from scipy.spatial import cKDTree
    q, p = np.asarray(query, F).reshape(-1, 3), np.asarray(ref, F).reshape(-1, 3)
    r2 = F(radius) * F(radius)
    k = min(k, len(p))
    dist, idx = cKDTree(p.astype(np.float64)).query(q.astype(np.float64), k=k, distance_upper_bound=float(radius) * (1 + 1e-4))
    dist, idx = dist.reshape(len(q), k), idx.reshape(len(q), k)
    cand = p[np.minimum(idx, len(p) - 1)]
    dx, dy, dz = (q[:, None, a] - cand[:, :, a] for a in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz
    d2 = np.where((idx < len(p)) & (d2 <= r2), d2, F(np.inf))
    full = np.isfinite(dist[:, -1]) & (k < len(p))               # all k slots used: a (k + 1)-th candidate may exist
    assert (dist[full, -1] > dist[full, 0] * (1 + 1e-5)).all(), "raise k: the candidates may miss the float32 minimum"
    return d2.min(1)


def voxel_downsample(points, voxel):
    """float32 [s,3]: per occupied voxel (edge `voxel`, voxel (0,0,0)'s corner at the cloud's minimum), in ascending voxel order, the
    sequential float32 sum of its points in their original order, per component, divided by float32(count)."""
    p = np.asarray(points, F).reshape(-1, 3)
    finite = p[np.isfinite(p).all(1)]
    if len(finite) == 0:
        return np.zeros((0, 3), F)
    lo, hi = finite.min(0), finite.max(0)
    dims = [int(v) + 1 for v in np.floor((hi - lo) / F(voxel))]
    c = cells(p, lo, voxel, dims)
    keep = np.nonzero(c >= 0)[0]
    order = keep[np.argsort(c[keep], kind="stable")]
    sorted_cells = c[order]
    start = np.nonzero(np.r_[True, sorted_cells[1:] != sorted_cells[:-1]])[0]
    count = np.diff(np.r_[start, len(order)])
    total = np.zeros((len(start), 3), F)
    for t in range(int(count.max())):                             # the t-th point of every voxel that has one: sequential per voxel
        has = count > t
        total[has] = total[has] + p[order[start[has] + t]]
    return total / count.astype(F)[:, None]


def apply_similarity(points, T):
    p, T = np.asarray(points, F).astype(np.float64), np.asarray(T, np.float64).reshape(4, 4)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1).astype(F)


def crop(rec, gt, margin):
    """(rec inside gt's box enlarged by margin, float32 comparisons; number dropped)."""
    lo, hi = gt.min(0) - F(margin), gt.max(0) + F(margin)
    keep = ((rec >= lo) & (rec <= hi)).all(1)
    return rec[keep], int((~keep).sum())


def scores(d2_rec, d2_gt, thresholds, max_distance):
    out = dict(rec_within=[], gt_within=[], precision=[], recall=[], fscore=[])
    for t in thresholds:
        t2 = F(t) * F(t)
        a, b = int(np.count_nonzero(d2_rec <= t2)), int(np.count_nonzero(d2_gt <= t2))
        P, R = a / len(d2_rec), b / len(d2_gt)
        out["rec_within"].append(a)
        out["gt_within"].append(b)
        out["precision"].append(P)
        out["recall"].append(R)
        out["fscore"].append(2 * P * R / (P + R) if P + R > 0 else 0.0)
    r2 = F(max_distance) * F(max_distance)
    for name, d2 in (("accuracy", d2_rec), ("completeness", d2_gt)):
        d = sorted(float(np.sqrt(np.float64(min(x, r2)))) for x in d2)
        out[name + "_mean"], out[name + "_median"] = float(np.mean(np.array(d))), d[len(d) // 2]
    return out


def evaluate(rec, gt, thresholds, transform=None, voxel=None, do_crop=True, max_distance=None, search=None):
    """acezero_amd.geometry.evaluate_geometry restated; `search(query, ref, radius) -> d2` defaults to the brute-force scan."""
    search = search or (lambda q, p, r: nearest(q, p, r)[0])
    rec, gt = np.asarray(rec, F).reshape(-1, 3), np.asarray(gt, F).reshape(-1, 3)
    r = float(max(thresholds) if max_distance is None else max_distance)
    out = dict(rec_points_read=len(rec), gt_points_read=len(gt))
    if transform is not None:
        rec = apply_similarity(rec, transform)
    if voxel is not None:
        rec, gt = voxel_downsample(rec, voxel), voxel_downsample(gt, voxel)
    dropped = 0
    if do_crop:
        rec, dropped = crop(rec, gt, r)
    out.update(rec_points=len(rec), gt_points=len(gt), dropped=dropped)
    out.update(scores(search(rec, gt, r), search(gt, rec, r), thresholds, r))
    return out
