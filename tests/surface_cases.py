"""Inputs for the surface tests (tests/test_surface_cpu.py, tests/test_surface_gpu.py): the box room as its exact surface, seeded
meshes with the edge cases of the face sampler, polygons and points for the crop. A helper module, not a test file."""
import numpy as np

from tests import fusion_cases as FC
from tests import surface_restated as SR

F = np.float32
SEEDS = (0, 1, 2019)


def box_room(half=FC.ROOM_HALF):
    """(vertices float32 [8,3], faces int32 [12,3]): the walls of the box room of tests/fusion_cases.py, two triangles per wall."""
    v = np.array([[sx * half[0], sy * half[1], sz * half[2]] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], F)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return v, np.array(faces, np.int32)


def unit_right_triangle():
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.array([[0, 1, 2]], np.int32)


def random_mesh(seed, k, m=None, colours=False):
    rng = np.random.default_rng(seed)
    m = m or max(3, k // 2 + 3)
    v = rng.uniform(-1, 1, (m, 3)).astype(F)
    f = rng.integers(0, m, (k, 3)).astype(np.int32)
    return v, f, rng.integers(0, 256, (m, 3), dtype=np.uint8) if colours else None


def mesh_cases():
    """name -> (vertices float32 [m,3], faces int32 [k,3], spacing, colours uint8 [m,3] or None)."""
    cases = {}
    for k in (0, 1, 63, 64, 65, 257):                              # some 13 samples per face: a workgroup's lanes span some 20 faces
        v, f, c = random_mesh(100 + k, k, colours=k in (1, 65, 257))
        cases[f"k{k}"] = (v, f, 0.15, c)
    # one face with 10^5 samples: 391 workgroups in one face
    v = np.array([[0, 0, 0], [1, 0.125, 0], [0.25, 1, 0.375]], F)
    cases["one_face_100k"] = (v, np.array([[0, 1, 2]], np.int32), 0.00225, np.array([[255, 0, 10], [0, 255, 20], [7, 0, 255]], np.uint8))
    # 5000 small faces with x of about 0.1: most get no sample, runs of empty faces between two samples
    rng = np.random.default_rng(7)
    a = rng.uniform(-1, 1, (5000, 1, 3))
    tri = np.concatenate([a, a + rng.uniform(-0.05, 0.05, (5000, 2, 3))], 1).reshape(-1, 3).astype(F)
    cases["sparse_5000"] = (tri, np.arange(15000, dtype=np.int32).reshape(5000, 3), 0.1, None)
    # what a file can hold: zero area (three points on a line, exactly), a repeated index, indices -1 and m, vertices that are not finite
    v, f, c = random_mesh(8, 60, m=40, colours=True)
    v[:3] = [[0, 0, 0], [0.5, 0.25, 0], [1, 0.5, 0]]
    v[37], v[38] = [np.nan, 0, 0], [0, np.inf, 0]
    f = np.where(f >= 37, f - 30, f)                                # the random faces use neither
    f[5], f[11], f[12], f[20], f[21], f[33], f[40], f[41] = (0, 1, 2), (7, 7, 9), (4, 4, 4), (-1, 3, 4), (3, 40, 4), (3, 4, 2 ** 31 - 1), (37, 5, 6), (5, 38, 6)
    cases["degenerate"] = (v, f.astype(np.int32), 0.15, c)
    v, f, _, c = cases["k257"]
    cases["k257_shuffled"] = (v, np.ascontiguousarray(f[shuffle()]), 0.15, c)
    return cases


def shuffle():
    """The order of k257's faces in k257_shuffled."""
    return np.random.default_rng(9).permutation(257)


def area_guard(vertices, faces, spacing, seed, ulps=4):
    """True where a face's count could change if its area moved by `ulps` ulp: x within that of an integer or of floor(x) + u0.
    Faces whose S is exactly 0 are exempt: the square root of 0 is 0 in every arithmetic."""
    counts, areas = SR.face_counts(vertices, faces, SR.density_of(spacing), seed)
    valid = areas > 0
    x = np.where(valid, areas, 1.0) * SR.density_of(spacing)
    tol = ulps * np.spacing(x) * 2                                 # the product's own rounding on top of the area's
    u0 = (SR.face_keys(seed, np.arange(len(areas))) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    near = (np.abs(x - np.rint(x)) <= tol) | (np.abs(x - (np.floor(x) + u0)) <= tol)
    return valid & near


# ------------------------------------------------------------------------------------------------------------------ crop
L_SHAPE = np.array([[0, 0], [1, 0], [1, 0.5], [0.5, 0.5], [0.5, 1], [0, 1]], F)
TRIANGLE = np.array([[-0.5, -0.25], [0.75, 0], [0, 0.875]], F)
CONVEX = np.array([[0, -1], [0.8, -0.5], [1, 0.3], [0.2, 1], [-0.7, 0.6], [-1, -0.4]], F)


def star(corners=1024):
    th = np.arange(corners) * (2 * np.pi / corners)
    r = 1.0 + 0.3 * np.sin(7 * th)
    return np.stack([r * np.cos(th), r * np.sin(th)], 1).astype(F)


def crop_points(seed, n, polygon, axis, lo, hi):
    """n points [n,3]: the first ones are special (the polygon's corners, exact edge midpoints, points exactly on the axis bounds and
    one float beyond them, NaN and infinity), the rest uniform over a box a quarter larger than the volume."""
    rng = np.random.default_rng(seed)
    poly = np.asarray(polygon, F)
    iu, iv = {0: (1, 2), 1: (0, 2), 2: (0, 1)}[axis]
    pmin, pmax = poly.min(0), poly.max(0)
    span = pmax - pmin
    p = np.zeros((n, 3), F)
    p[:, iu] = rng.uniform(pmin[0] - span[0] / 4, pmax[0] + span[0] / 4, n)
    p[:, iv] = rng.uniform(pmin[1] - span[1] / 4, pmax[1] + span[1] / 4, n)
    p[:, axis] = rng.uniform(lo - (hi - lo) / 4, hi + (hi - lo) / 4, n)
    mid = F(0.5) * (F(lo) + F(hi))
    inside = F(0.5) * (poly[0] + poly.mean(0))                     # between a corner and the centroid: inside all polygons used here
    special = []
    for i in range(min(len(poly), 8)):
        j = (i + 1) % len(poly)
        special.append((poly[i, 0], poly[i, 1], mid))
        special.append((F(0.5) * (poly[i, 0] + poly[j, 0]), F(0.5) * (poly[i, 1] + poly[j, 1]), mid))
    for w in (F(lo), F(hi), np.nextafter(F(lo), F(-np.inf)), np.nextafter(F(hi), F(np.inf))):
        special.append((inside[0], inside[1], w))
    special += [(np.nan, inside[1], mid), (inside[0], np.inf, mid), (inside[0], inside[1], -np.inf), (inside[0], inside[1], np.nan)]
    for row, (u, v, w) in enumerate(special[:n]):
        p[row, iu], p[row, iv], p[row, axis] = u, v, w
    return p


def crop_cases():
    """name -> (points [n,3], polygon float32 [p,2], axis, axis_min, axis_max)."""
    cases = {}
    for n in (0, 1, 63, 64, 65, 257):
        cases[f"triangle_z_{n}"] = (crop_points(n, n, TRIANGLE, 2, -0.5, 0.25), TRIANGLE, 2, -0.5, 0.25)
    for axis in (0, 1, 2):
        cases[f"l_shape_axis{axis}_1000"] = (crop_points(30 + axis, 1000, L_SHAPE, axis, 0.25, 0.75), L_SHAPE, axis, 0.25, 0.75)
        cases[f"l_shape_reversed_axis{axis}_257"] = (crop_points(40 + axis, 257, L_SHAPE[::-1], axis, -1.0, -1.0), np.ascontiguousarray(L_SHAPE[::-1]), axis, -1.0, -1.0)
    cases["star_1024_y_1000"] = (crop_points(50, 1000, star(), 1, -2.0, 3.0), star(), 1, -2.0, 3.0)
    return cases
