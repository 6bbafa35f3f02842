"""Inputs for the cloud-distance tests (tests/test_geometry_cpu.py, tests/test_geometry_gpu.py): seeded clouds, the edge cases of the
grid search, the ground-truth lattice of the box room and similarity transforms. A helper module, not a test file."""
import numpy as np

from tests import fusion_cases as FC

F = np.float32
MARGIN = F(1.0 + 2.0 ** -10)


def uniform(seed, n, lo=0.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(F)


def surface(seed, n, noise=0.002):
    """A surface-like cloud: points on the unit sphere's upper half, with a little noise."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v[:, 2] = np.abs(v[:, 2])
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v + rng.normal(scale=noise, size=(n, 3))).astype(F)


def search_cases():
    """name -> (query [n,3], ref [m,3], radius, cell or None). Every case is compared with the brute-force scan bit for bit."""
    cases = {}
    rng = np.random.default_rng(11)
    cases["no_reference"] = (uniform(1, 10), np.zeros((0, 3), F), 0.2, None)
    cases["no_query"] = (np.zeros((0, 3), F), uniform(1, 10), 0.2, None)
    cases["one_and_one_found"] = (np.array([[0.5, 0.5, 0.5]], F), np.array([[0.5, 0.55, 0.5]], F), 0.1, None)
    cases["one_and_one_too_far"] = (np.array([[0.5, 0.5, 0.5]], F), np.array([[0.5, 0.75, 0.5]], F), 0.1, None)
    for n in (63, 64, 65, 257):
        # sparse: 257 queries over 6^3 cells, a workgroup's queries lie in many cells
        cases[f"uniform_{n}"] = (uniform(2 * n, n), uniform(2 * n + 1, n), 0.15, None)
    # dense: some 80 points per cell, a workgroup's queries lie in a few adjacent cells
    cases["dense_cube"] = (uniform(3, 3000), uniform(4, 5000), 0.25, None)
    cases["dense_surface"] = (surface(5, 4000), surface(6, 6000), 0.12, None)
    # some 240 queries and references per cell on a plane of 5 x 5 cells: a workgroup's queries lie in two or three adjacent cells,
    # also across the end of a row of cells
    flat, qflat = uniform(24, 6000), uniform(25, 6000)
    flat[:, 2], qflat[:, 2] = F(0.5), F(0.5) + rng.uniform(-0.05, 0.05, 6000).astype(F)
    cases["dense_plane"] = (qflat, flat, 0.2, None)
    # one cell with more points than any staging chunk, every query in it
    cases["one_cell_5000"] = (uniform(7, 300, 0.0, 0.015), uniform(8, 5000, 0.0, 0.015), 0.02, None)
    plane = uniform(9, 3000)
    plane[:, 2] = F(0.375)
    qplane = uniform(10, 1000)
    qplane[:, 2] = F(0.375) + (rng.uniform(-0.03, 0.03, 1000)).astype(F)
    cases["plane_nz_1"] = (qplane, plane, 0.06, None)
    line = uniform(12, 2000)
    line[:, 1:] = F(-1.25)
    qline = uniform(13, 700)
    qline[:, 1:] = F(-1.25) + rng.uniform(-0.02, 0.02, (700, 2)).astype(F)
    cases["line_ny_nz_1"] = (qline, line, 0.03, None)
    # references on the cell faces and at the box's corners: a lattice of the cell edge itself (0.25 and its multiples are exact)
    g = np.arange(5, dtype=F) * F(0.25)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    near = (lattice[rng.integers(0, len(lattice), 600)] + rng.uniform(-0.2, 0.2, (600, 3))).astype(F)
    cases["faces_and_corners"] = (np.concatenate([near, lattice]), lattice, 0.2, 0.25)
    # queries outside the reference's box: nearer than the radius to it, and farther
    box = uniform(14, 2000)
    shell = uniform(15, 1500, -0.3, 1.3)
    outside = shell[((shell < 0) | (shell > 1)).any(1)]
    far = uniform(16, 100, 5.0, 9.0) * np.where(rng.random((100, 3)) < 0.5, -1, 1).astype(F)
    huge = np.array([[3e38, 0.5, 0.5], [-3e38, -3e38, 0.5], [1e20, 1e20, 1e20]], F)
    cases["outside_the_box"] = (np.concatenate([outside, far, huge]), box, 0.15, None)
    # d2 == R * R exactly (found) and the next float above (none): R = 0.75, R * R = 0.5625 in [0.5, 1) where an ulp is 2^-24 = (2^-12)^2
    cases["exactly_the_radius"] = (np.array([[0.75, 0, 0], [0.75, 2.0 ** -12, 0], [0, -0.75, 0], [0, 2.0 ** -12, 0.75]], F),
                                   np.array([[0, 0, 0]], F), 0.75, None)
    # pairs at distance R * (1 - 2^-20) along an axis, the reference just below a cell face, at the smallest legal cell (coordinates
    # below 2, so that rounding the query, at most 2^-24 * 2, is well inside the R * 2^-20 = 2.4e-7 the pair has to spare)
    r = F(0.25)
    c = r * MARGIN
    base = uniform(17, 900, 0.0, 1.0)
    k = rng.integers(1, 5, (900, 3)).astype(F)
    eps = rng.choice([0.0, 1e-7, 1e-6, 1e-5], (900, 3)).astype(F)
    refs = np.where(rng.random((900, 3)) < 0.7, k * c - eps, base).astype(F)
    refs = np.concatenate([np.zeros((1, 3), F), np.full((1, 3), 5, F) * c, refs])          # pins the box: origin 0
    step = np.zeros((len(refs), 3), F)
    step[np.arange(len(refs)), rng.integers(0, 3, len(refs))] = rng.choice([-1, 1], len(refs)) * (r * F(1.0 - 2.0 ** -20))
    cases["straddling_a_face"] = ((refs + step).astype(F), refs, float(r), float(c))
    # equal d2: mirrored references, and duplicated points (the lower row wins)
    sym_q = uniform(18, 200)
    d = rng.uniform(0.01, 0.05, (200, 1)).astype(F) * np.eye(3, dtype=F)[rng.integers(0, 3, 200)]
    cases["ties"] = (sym_q, np.concatenate([sym_q + d, sym_q - d, sym_q - d, sym_q + d]).astype(F), 0.1, None)
    dup = uniform(19, 500)
    cases["duplicates"] = (uniform(20, 400), np.concatenate([dup, dup[::-1], dup]), 0.2, None)
    # queries and references that are not finite
    bad_q = uniform(21, 300)
    bad_q[[0, 17, 63, 64, 299], [0, 1, 2, 0, 1]] = [np.nan, np.inf, -np.inf, np.nan, np.nan]
    bad_r = uniform(22, 300)
    bad_r[[5, 100], [0, 2]] = [np.nan, np.inf]
    cases["not_finite"] = (bad_q, bad_r, 0.2, None)
    return cases


def downsample_cases():
    """name -> (points, voxel): a voxel with 3000 points, voxels with one, points on voxel faces, a point that is not finite."""
    rng = np.random.default_rng(23)
    crowd = rng.uniform(0.51, 0.59, (3000, 3)).astype(F)           # inside one voxel of 0.1 (the grid starts at the minimum, 0)
    lone = (np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(2, 5), indexing="ij"), -1).reshape(-1, 3) * 0.1 + 0.05).astype(F)
    few = rng.uniform(0, (0.4, 0.4, 0.19), (500, 3)).astype(F)       # below the lone points' layers
    mixed = np.concatenate([np.zeros((1, 3), F), crowd, lone, few])
    mixed = mixed[np.r_[0, 1 + rng.permutation(len(mixed) - 1)]]
    bad = mixed.copy()
    bad[7, 1] = np.nan
    faces = (rng.integers(0, 9, (800, 3)) * 0.125).astype(F)         # multiples of the voxel: exactly on faces, many duplicates
    return {"crowd_and_singles": (mixed, 0.1), "a_nan": (bad, 0.1), "on_faces": (faces, 0.125), "one_point": (np.ones((1, 3), F), 0.5)}


def room_lattice(step=0.005, half=FC.ROOM_HALF):
    """float32 [~357k,3]: a `step` lattice on the six walls of the box room, edges included (a point on an edge appears once per
    wall it lies on)."""
    axes = [np.arange(-int(round(h / step)), int(round(h / step)) + 1) * step for h in half]
    out = []
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        u, v = np.meshgrid(axes[b], axes[c], indexing="ij")
        for side in (-1.0, 1.0):
            p = np.zeros(u.shape + (3,))
            p[..., a], p[..., b], p[..., c] = side * half[a], u, v
            out.append(p.reshape(-1, 3))
    return np.concatenate(out).astype(F)


def similarity(scale=1.7, axis=(0.3, -0.5, 0.8), angle=0.9, t=(0.4, -1.1, 2.3)):
    """4 x 4 float64: x -> scale * R x + t."""
    from scipy.spatial.transform import Rotation
    axis = np.asarray(axis, np.float64)
    T = np.eye(4)
    T[:3, :3] = scale * Rotation.from_rotvec(angle * axis / np.linalg.norm(axis)).as_matrix()
    T[:3, 3] = t
    return T
