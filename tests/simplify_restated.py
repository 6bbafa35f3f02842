"""The mesh simplification of include/acez.h section Q restated on the host: float32 cells, fp64 sums in the header's order (the k-th
vertex or corner of every cluster is added in pass k, so each cluster's sum runs in its own order while numpy works across clusters;
a cluster's corners go to 64 lanes in turn and the lanes are folded by the header's butterfly),
svd3 (acezero_amd/csrc/svd3.h) and the placement (acezero_amd/csrc/simplify_solve.h) in Python floats, one IEEE operation per
operation written. The HIP kernels are compared with it bit for bit (tests/test_simplify_gpu.py), the host instantiation of the solve
too (tests/test_simplify_cpu.py). A helper module, not a test file. Nothing here imports acezero_amd.simplify."""
import math

import numpy as np

from tests.ordered_sums import WAVE, wave_sums

F = np.float32
AXIS_BITS = 21
NO_CELL = 2 ** 63 - 1
RANK_RATIO = 1e-3
EPS = 2.220446049250313e-16


# ------------------------------------------------------------------------------------------------------------------- svd3.h
def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def any_orthogonal(a):
    e = [0.0, 0.0, 0.0]
    ax, ay, az = abs(a[0]), abs(a[1]), abs(a[2])
    e[0 if (ax <= ay and ax <= az) else (1 if ay <= az else 2)] = 1.0
    c = cross3(a, e)
    n = math.sqrt(dot3(c, c))
    return [c[0] / n, c[1] / n, c[2] / n]


def svd3(C):
    """(u, v, s) of the row-major 3 x 3 C (nine floats): u[i], v[i] the i-th columns, s descending with s[2] signed; the one-sided
    Jacobi of svd3.h statement by statement."""
    b = [[C[r * 3 + i] for r in range(3)] for i in range(3)]
    v = [[1.0 if r == i else 0.0 for r in range(3)] for i in range(3)]
    for _ in range(12):
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            al, be, ga = dot3(b[p], b[p]), dot3(b[q], b[q]), dot3(b[p], b[q])
            if not abs(ga) > EPS * math.sqrt(al * be):
                continue
            rotated = True
            zeta = (be - al) / (2.0 * ga)
            t = (1.0 if zeta >= 0.0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
            c = 1.0 / math.sqrt(1.0 + t * t)
            s = c * t
            for r in range(3):
                bp, bq = b[p][r], b[q][r]
                b[p][r] = c * bp - s * bq
                b[q][r] = s * bp + c * bq
                vp, vq = v[p][r], v[q][r]
                v[p][r] = c * vp - s * vq
                v[q][r] = s * vp + c * vq
        if not rotated:
            break
    n = [math.sqrt(dot3(b[i], b[i])) for i in range(3)]
    order = [0, 1, 2]
    for i in range(2):
        for j in range(2 - i):
            if n[order[j]] < n[order[j + 1]]:
                order[j], order[j + 1] = order[j + 1], order[j]
    ov = [list(v[order[0]]), list(v[order[1]])]
    ov.append(cross3(ov[0], ov[1]))
    s = [n[order[0]], n[order[1]], 0.0]
    ou = [[1.0, 0.0, 0.0], None, None]
    if s[0] > 0.0:
        ou[0] = [b[order[0]][r] / s[0] for r in range(3)]
    if s[1] > 0.0:
        ou[1] = [b[order[1]][r] / s[1] for r in range(3)]
    else:
        ou[1] = any_orthogonal(ou[0]) if s[0] > 0.0 else [0.0, 1.0, 0.0]
    ou[2] = cross3(ou[0], ou[1])
    cv = [C[r * 3] * ov[2][0] + C[r * 3 + 1] * ov[2][1] + C[r * 3 + 2] * ov[2][2] for r in range(3)]
    s[2] = dot3(ou[2], cv)
    return ou, ov, s


# ----------------------------------------------------------------------------------------------------------- simplify_solve.h
def corner_terms(a, b, c):
    """float64 [n,9] from the float64 [n,3] vertices of n faces, relative to the cell centre of the cluster each term goes to."""
    e1, e2 = b - a, c - a
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    d = -((n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2])
    return np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2], n[:, 2] * n[:, 2],
                     d * n[:, 0], d * n[:, 1], d * n[:, 2]], 1)


def solve(q, mean, cell):
    """(solved, x): the placement from the nine sums q, the mean relative to the cell centre and the cell edge, all Python floats."""
    q, mean, cell = [float(t) for t in q], [float(t) for t in mean], float(cell)
    A = [q[0], q[1], q[2], q[1], q[3], q[4], q[2], q[4], q[5]]
    _, v, s = svd3(A)
    if not s[0] > 0.0:
        return False, mean
    g = [-q[6 + j] - ((A[3 * j] * mean[0] + A[3 * j + 1] * mean[1]) + A[3 * j + 2] * mean[2]) for j in range(3)]
    least = RANK_RATIO * s[0]
    y = list(mean)
    for i in range(3):
        if not s[i] > least:
            continue
        step = dot3(v[i], g) / s[i]
        for j in range(3):
            y[j] = y[j] + v[i][j] * step
    if any(not math.isfinite(t) or abs(t) > cell for t in y):
        return False, mean
    return True, y


# --------------------------------------------------------------------------------------------------------------- the steps
def ordered_sums(rows, group, n_groups):
    """float64 [n_groups, c]: per group the rows [n, c] added one by one to 0.0 in the order they stand in; `group` ascends."""
    start = np.searchsorted(group, np.arange(n_groups))
    count = np.searchsorted(group, np.arange(n_groups), side="right") - start
    acc = np.zeros((n_groups, rows.shape[1]))
    for j in range(int(count.max()) if n_groups else 0):
        sel = np.flatnonzero(count > j)
        acc[sel] = acc[sel] + rows[start[sel] + j]
    return acc, count


def wavefront_sums(rows, group, n_groups):
    """float64 [n_groups, c]: per group, lane l of 64 adds the rows at positions l, l + 64, .. of the group one by one to 0.0, then the
    xor butterfly 32, 16, .. 1 over the lanes; lane 0's sums. `group` ascends."""
    start = np.searchsorted(group, np.arange(n_groups))
    count = np.searchsorted(group, np.arange(n_groups), side="right") - start
    lanes = np.zeros((n_groups, WAVE, rows.shape[1]))
    for j in range(int(count.max()) if n_groups else 0):
        sel = np.flatnonzero(count > j)
        lanes[sel, j % WAVE] = lanes[sel, j % WAVE] + rows[start[sel] + j]
    return wave_sums(lanes)


def clusters(vertices, cell):
    """(origin float32 [3], vertex_cluster int32 [m] with -1 for the vertices that are not finite, cell index int64 [K,3])."""
    v, cell = np.asarray(vertices, F).reshape(-1, 3), F(cell)
    finite = np.isfinite(v).all(1)
    origin = v[finite].min(0) if finite.any() else np.zeros(3, F)
    keys = np.full(len(v), NO_CELL, np.int64)
    with np.errstate(all="ignore"):
        index = np.floor((v[finite] - origin) / cell)
    assert index.dtype == F and (not len(index) or index.max() < 2 ** AXIS_BITS - 1)
    index = index.astype(np.int64)
    keys[finite] = index[:, 0] | (index[:, 1] << AXIS_BITS) | (index[:, 2] << (2 * AXIS_BITS))
    occupied, inverse = np.unique(keys[finite], return_inverse=True)
    vertex_cluster = np.full(len(v), -1, np.int32)
    vertex_cluster[finite] = inverse
    mask = 2 ** AXIS_BITS - 1
    return origin, vertex_cluster, np.stack([occupied & mask, (occupied >> AXIS_BITS) & mask, occupied >> (2 * AXIS_BITS)], 1)


def classify(faces, vertex_cluster):
    """(invalid, degenerate, valid) bool [k] and the clusters of the corners int32 [k,3] (meaningful where valid)."""
    f, m = np.asarray(faces, np.int32).reshape(-1, 3), len(vertex_cluster)
    in_range = ((f >= 0) & (f < m)).all(1)
    distinct = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    mapped = vertex_cluster[np.where(in_range[:, None], f, 0)] if m else np.full(f.shape, -1, np.int32)
    valid = in_range & distinct & (mapped >= 0).all(1)
    degenerate = in_range & ~distinct
    return ~valid & ~degenerate, degenerate, valid, mapped


def simplify_mesh(vertices, colours, faces, cell, placement="quadric"):
    """acezero_amd.simplify.simplify_mesh restated: (vertices, colours or None, faces, info)."""
    v, f, cell = np.asarray(vertices, F).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3), F(cell)
    m, k = len(v), len(f)
    origin, vertex_cluster, index = clusters(v, cell)
    K = len(index)
    invalid, degenerate, valid, mapped = classify(f, vertex_cluster)
    # 4: the mean and the colour, a cluster's vertices in ascending id
    with_cell = np.flatnonzero(vertex_cluster >= 0)
    order = with_cell[np.argsort(vertex_cluster[with_cell], kind="stable")]
    sums, count = ordered_sums(v[order].astype(np.float64), vertex_cluster[order], K)
    mean = sums / count[:, None].astype(np.float64)
    position = mean.copy()
    cluster_colours = None
    if colours is not None:
        rgb = np.zeros((K, 3), np.int64)
        np.add.at(rgb, vertex_cluster[order], np.asarray(colours, np.uint8)[order].astype(np.int64))
        cluster_colours = ((2 * rgb + count[:, None]) // (2 * count[:, None])).astype(np.uint8)
    fallback = np.zeros(K, bool)
    if placement == "quadric":
        # 5: every corner of every valid face, a cluster's corners in ascending 3 face + corner
        centre = origin.astype(np.float64) + (index.astype(np.float64) + 0.5) * np.float64(cell)
        corner = np.flatnonzero(np.repeat(valid, 3))
        corner = corner[np.argsort(mapped.reshape(-1)[corner], kind="stable")]
        to = mapped.reshape(-1)[corner]
        face = f[corner // 3]
        p = [v[face[:, c]].astype(np.float64) - centre[to] for c in range(3)]
        q = wavefront_sums(corner_terms(*p), to, K)
        rel = mean - centre
        for c in range(K):
            solved, y = solve(q[c], rel[c], cell)
            fallback[c] = not solved
            if solved:
                position[c] = centre[c] + np.array(y)
    else:
        assert placement == "mean"
    # 7: the faces
    distinct = (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 0] != mapped[:, 2])
    candidate = np.flatnonzero(valid & distinct)
    tri = mapped[candidate]
    tri = np.take_along_axis(tri, (np.argmin(tri, 1)[:, None] + np.arange(3)[None, :]) % 3, 1)
    by_triple = np.lexsort((candidate, tri[:, 2], tri[:, 1], tri[:, 0]))
    s = tri[by_triple]
    first = np.ones(len(s), bool)
    first[1:] = (s[1:] != s[:-1]).any(1)
    kept = np.zeros(len(tri), bool)
    kept[by_triple[first]] = True
    out_faces = tri[kept]
    # 8: the vertices
    used = np.zeros(K, bool)
    used[out_faces.reshape(-1)] = True
    rename = np.cumsum(used) - 1
    info = dict(clusters=K, vertices_in=m, faces_in=k, vertices_out=int(used.sum()), faces_out=len(out_faces), invalid_faces=int(invalid.sum()),
                degenerate_faces=int(degenerate.sum()), nonfinite_vertices=m - len(with_cell), collapsed_faces=int((valid & ~distinct).sum()),
                duplicate_faces=len(tri) - len(out_faces), unused_clusters=K - int(used.sum()), fallbacks=int((fallback & used).sum()))
    return (position[used].astype(F), None if colours is None else cluster_colours[used].reshape(-1, 3),
            rename[out_faces].astype(np.int32).reshape(-1, 3), info)
