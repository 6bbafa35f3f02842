"""include/acez.h section O restated in numpy: the face areas and counts, the samples of the faces and the polygon crop, in float64
and uint64 arithmetic exactly as the header writes them. A helper module, not a test file; tests/test_surface_cpu.py checks its
properties, tests/test_surface_gpu.py compares the kernels with it bit for bit. Nothing here imports acezero_amd.geometry."""
import math

import numpy as np

F = np.float32
U64 = np.uint64
STRIDE = U64(0xD1B54A32D192ED03)


def mix64(z):
    """mix64 of acezero_amd/csrc/ransac_math.h on uint64 arrays, modulo 2^64."""
    z = np.asarray(z, U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def face_keys(seed, t):
    return mix64(mix64(U64(int(seed) & (2 ** 64 - 1))) ^ np.asarray(t, U64))


def density_of(spacing):
    s = float(spacing)
    return 1.0 / (s * s)


def _corners(vertices, faces):
    """(valid [k], a, e1, e2 float64 [k,3]) with the indices of invalid faces replaced by 0."""
    v = np.asarray(vertices, F).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valid = ((f >= 0) & (f < len(v))).all(1)
    f = np.where(valid[:, None], f, 0)
    if len(v) == 0:
        z = np.zeros((len(f), 3))
        return valid, z, z, z
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return valid, a, b - a, c - a


def face_counts(vertices, faces, density, seed):
    """(counts int32 [k], areas float64 [k]): COUNTS."""
    valid, a, e1, e2 = _corners(vertices, faces)
    k = len(valid)
    with np.errstate(all="ignore"):
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        s = (nx * nx + ny * ny) + nz * nz
        area = 0.5 * np.sqrt(s)
        valid = valid & np.isfinite(area)
        x = np.where(valid, area, 0.0) * np.float64(density)
        f = np.floor(x)
        u0 = (face_keys(seed, np.arange(k)) >> U64(11)).astype(np.float64) * 2.0 ** -53
        extra = u0 < x - f                                        # x = inf: inf - inf is NaN, the comparison is false
        counts = np.minimum(f, 2.0 ** 30).astype(np.int64) + extra
    return np.where(valid, counts, 0).astype(np.int32), np.where(valid, area, -1.0)


def offsets_of(counts):
    return np.r_[0, np.cumsum(np.asarray(counts, np.int64))].astype(np.int64)


def barycentric(seed, t, i):
    """(u, v) float64 of sample i of face t, after the fold."""
    with np.errstate(over="ignore"):
        r = mix64(face_keys(seed, t) + (np.asarray(i, U64) + U64(1)) * STRIDE)
    u = (r >> U64(40)).astype(np.float64) * 2.0 ** -24
    v = ((r >> U64(16)) & U64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    fold = u + v > 1.0
    return np.where(fold, 1.0 - u, u), np.where(fold, 1.0 - v, v)


def sample_faces(vertices, faces, offsets, seed, colours=None):
    """(points float32 [n,3], face int32 [n], colours uint8 [n,3] or None): SAMPLE over the exclusive offsets int64 [k + 1]."""
    offsets = np.asarray(offsets, np.int64)
    k, n = len(offsets) - 1, int(offsets[-1])
    if n == 0:
        return np.zeros((0, 3), F), np.zeros(0, np.int32), None if colours is None else np.zeros((0, 3), np.uint8)
    j = np.arange(n, dtype=np.int64)
    t = np.searchsorted(offsets[:k], j, side="right") - 1        # the last face with offsets[t] <= j
    i = j - offsets[t]
    u, v = barycentric(seed, t, i)
    m = len(np.asarray(vertices).reshape(-1, 3))
    f = np.clip(np.asarray(faces, np.int64).reshape(-1, 3)[t], 0, m - 1)
    vert = np.asarray(vertices, F).reshape(-1, 3).astype(np.float64)
    a = vert[f[:, 0]]
    e1, e2 = vert[f[:, 1]] - a, vert[f[:, 2]] - a
    with np.errstate(all="ignore"):
        points = ((a + u[:, None] * e1) + v[:, None] * e2).astype(F)
    out = None
    if colours is not None:
        col = np.asarray(colours, np.uint8).reshape(-1, 3).astype(np.float64)
        w = (1.0 - u) - v
        out = np.floor(((w[:, None] * col[f[:, 0]] + u[:, None] * col[f[:, 1]]) + v[:, None] * col[f[:, 2]]) + 0.5).astype(np.uint8)
    return points, t.astype(np.int32), out


def sample_mesh(vertices, faces, spacing, seed=0, colours=None):
    """acezero_amd.geometry.sample_mesh restated: (points, face, colours, info)."""
    counts, areas = face_counts(vertices, faces, density_of(spacing), seed)
    points, face, col = sample_faces(vertices, faces, offsets_of(counts), seed, colours)
    info = {"faces": len(counts), "faces_invalid": int((areas < 0).sum()), "area": math.fsum(areas[areas >= 0].tolist()),
            "samples": len(points)}
    return points, face, col, info


def crop_keep(points, polygon, axis, axis_min, axis_max):
    """bool [n]: CROP. polygon float32 [p,2] (U, V); the crossings of every edge i -> (i + 1) mod p in float64."""
    p = np.asarray(points, F).reshape(-1, 3)
    poly = np.asarray(polygon, F).reshape(-1, 2).astype(np.float64)
    iu, iv = {0: (1, 2), 1: (0, 2), 2: (0, 1)}[int(axis)]
    u, v, w = p[:, iu].astype(np.float64), p[:, iv].astype(np.float64), p[:, int(axis)]
    crossings = np.zeros(len(p), np.int64)
    with np.errstate(all="ignore"):
        for i in range(len(poly)):
            (ui, vi), (uj, vj) = poly[i], poly[(i + 1) % len(poly)]
            lhs, rhs = (u - ui) * (vj - vi), (v - vi) * (uj - ui)
            crossings += ((vi > v) != (vj > v)) & ((lhs < rhs) if vj > vi else (lhs > rhs))
        return np.isfinite(p).all(1) & (F(axis_min) <= w) & (w <= F(axis_max)) & (crossings % 2 == 1)


def winding_inside(u, v, polygon):
    """bool [n]: the winding number of the polygon around (u, v) is not zero, in float64, from summed signed angles: an independent
    statement of 'inside' for points away from the edges."""
    poly = np.asarray(polygon, np.float64).reshape(-1, 2)
    du, dv = poly[None, :, 0] - np.asarray(u, np.float64)[:, None], poly[None, :, 1] - np.asarray(v, np.float64)[:, None]
    du2, dv2 = np.roll(du, -1, 1), np.roll(dv, -1, 1)
    angle = np.arctan2(du * dv2 - dv * du2, du * du2 + dv * dv2).sum(1)
    return np.abs(angle) > math.pi


def edge_distance(u, v, polygon):
    """float64 [n]: the distance of (u, v) to the nearest edge of the polygon."""
    poly = np.asarray(polygon, np.float64).reshape(-1, 2)
    q = np.stack([np.asarray(u, np.float64), np.asarray(v, np.float64)], 1)[:, None, :]
    a, b = poly[None, :, :], np.roll(poly, -1, 0)[None, :, :]
    ab = b - a
    s = np.clip(((q - a) * ab).sum(-1) / np.maximum((ab * ab).sum(-1), 1e-300), 0.0, 1.0)
    return np.linalg.norm(q - (a + s[..., None] * ab), axis=-1).min(1)
