"""Meshes for the simplification tests (tests/test_simplify_cpu.py, tests/test_simplify_gpu.py): a cube and a sphere whose
simplified surface can be judged, a soup with everything the definition has a rule for, and the two ends of the per-cluster sums. A
helper module, not a test file. A case is (vertices float32 [m,3], colours uint8 [m,3], faces int32 [k,3], cell)."""
import functools

import numpy as np

F = np.float32
CUBE_MIN = -0.037                 # the cube is [CUBE_MIN, CUBE_MIN + 1]^3: section Q puts the grid's origin at the mesh's minimum
SPHERE_R = 0.3


def colours_for(m, seed=21):
    return np.random.default_rng(seed).integers(0, 256, (m, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def cube(n=32):
    """A unit cube of n x n quads per side, outward orientation, its vertices shared between the sides: 6 n^2 + 2 vertices, 12 n^2 faces."""
    ids, points, faces = {}, [], []

    def vertex(p):
        if p not in ids:
            ids[p] = len(points)
            points.append(p)
        return ids[p]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    quad = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        quad.append(vertex(tuple(p)))
                    if side == 0:                                   # (u, w, axis) is right-handed: at side 0 the outward normal is -axis
                        quad = quad[::-1]
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    v = (np.array(points, np.float64) / n + CUBE_MIN).astype(F)
    return v, colours_for(len(v)), np.array(faces, np.int32)


def cube_distance(points):
    """The distance of every point [n,3] to the surface of the cube, for points no further out than they are in."""
    p = np.asarray(points, np.float64) - (np.float64(F(CUBE_MIN)) + 0.5)
    outside = np.linalg.norm(np.maximum(np.abs(p) - 0.5, 0.0), axis=1)
    inside = np.maximum(0.5 - np.abs(p).max(1), 0.0)
    return np.maximum(outside, inside)


@functools.lru_cache(maxsize=None)
def sphere(segments=96, rings=48, radius=SPHERE_R):
    """A UV sphere about the origin, outward orientation: segments (rings - 1) + 2 vertices, 2 segments (rings - 1) faces."""
    theta = np.pi * np.arange(1, rings) / rings
    phi = 2.0 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.sin(theta)[:, None] * np.cos(phi)[None, :], np.sin(theta)[:, None] * np.sin(phi)[None, :],
                     np.repeat(np.cos(theta)[:, None], segments, 1)], -1).reshape(-1, 3)
    v = (radius * np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]])).astype(F)
    at = lambda r, s: 1 + r * segments + s % segments   # noqa: E731
    south = len(v) - 1
    faces = []
    for s in range(segments):
        faces.append([0, at(0, s), at(0, s + 1)])
        for r in range(rings - 2):
            faces += [[at(r, s), at(r + 1, s), at(r + 1, s + 1)], [at(r, s), at(r + 1, s + 1), at(r, s + 1)]]
        faces.append([south, at(rings - 2, s + 1), at(rings - 2, s)])
    return v, colours_for(len(v), 22), np.array(faces, np.int32)


@functools.lru_cache(maxsize=None)
def soup(m=300, k=600, seed=23):
    """Random vertices in the unit box; every face joins a vertex with two of its eight nearest, so that at a cell of 0.2 faces
    collapse and coincide. Planted: a NaN and an infinite vertex (and faces on them), indices out of range, degenerate faces, exact
    duplicates, a pair of opposite orientation, a vertex that nothing references."""
    g = np.random.default_rng(seed)
    v = g.uniform(0.0, 1.0, (m, 3)).astype(F)
    near = np.argsort(((v[:, None, :].astype(np.float64) - v[None, :, :]) ** 2).sum(-1), 1, kind="stable")[:, 1:9]
    a = g.integers(0, m - 1, k)                                      # vertex m - 1 is referenced by nothing
    pick = np.stack([g.permutation(8)[:2] for _ in range(k)])
    f = np.stack([a, near[a, pick[:, 0]], near[a, pick[:, 1]]], 1).astype(np.int32)
    f[f == m - 1] = 0
    v[17] = [np.nan, 0.5, 0.5]
    v[41] = [0.25, np.inf, 0.5]
    f[5] = [3, m, 9]
    f[6] = [-1, 4, 8]
    f[7] = [2 ** 31 - 1, 1, 2]
    f[30] = [12, 12, 40]
    f[31] = [7, 9, 7]
    f[100], f[200] = f[50], f[50]                                    # exact duplicates of a face, later in the input
    f[101] = f[51][[1, 2, 0]]                                        # the same face, rotated
    f[102] = f[52][[0, 2, 1]]                                        # the opposite orientation: another face
    return v, colours_for(m, 24), f, F(0.2)


def cone(rim=200):
    """A fan of `rim` faces about an apex: the apex's cluster has one vertex and `rim` corners (more than 64 x 3)."""
    phi = 2.0 * np.pi * np.arange(rim) / rim
    v = np.concatenate([[[0.0, 0.0, 0.7]], np.stack([np.cos(phi), np.sin(phi), np.zeros(rim)], 1)]).astype(F)
    i = np.arange(rim)
    f = np.stack([np.zeros(rim, np.int64), 1 + i, 1 + (i + 1) % rim], 1).astype(np.int32)
    return v, colours_for(len(v), 25), f, F(0.05)


def one_triangle():
    """Three vertices in three cells: every cluster has one vertex and one corner."""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 1.0, 0.3]], F)
    return v, colours_for(3, 26), np.array([[0, 1, 2]], np.int32), F(0.25)


def cases():
    """name -> (vertices, colours, faces, cell): every case the kernels are compared with the restatement on."""
    cv, cc, cf = cube()
    sv, sc, sf = sphere()
    pv, pc, pf, pcell = soup()
    none_v, none_f = np.zeros((0, 3), F), np.zeros((0, 3), np.int32)
    return {
        "cube_0.1": (cv, cc, cf, F(0.1)), "cube_0.13": (cv, cc, cf, F(0.13)), "sphere_0.03": (sv, sc, sf, F(0.03)),
        "soup": (pv, pc, pf, pcell), "soup_one_cell": (pv, pc, pf, F(10.0)), "cone": cone(), "one_triangle": one_triangle(),
        "empty": (none_v, colours_for(0), none_f, F(0.1)), "no_faces": (pv, pc, none_f, pcell),
        "no_vertices": (none_v, colours_for(0), pf[:20], pcell),
        "nothing_finite": (np.full((3, 3), np.nan, F), colours_for(3), np.array([[0, 1, 2]], np.int32), F(0.1)),
    }


def closedness(faces):
    """(open edges, edges with more than two faces, directed edges that occur more than once): (0, 0, 0) for a closed, consistently
    oriented surface."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    _, directed = np.unique(e, axis=0, return_counts=True)
    _, undirected = np.unique(np.sort(e, 1), axis=0, return_counts=True)
    return int((undirected == 1).sum()), int((undirected > 2).sum()), int((directed > 1).sum())
