"""Scenes for the mesh-rendering tests (tests/test_meshrender_cpu.py, tests/test_meshrender_gpu.py): small meshes whose image has a
closed form or that exercise one route of include/acez.h section R. A helper module, not a test file."""
import numpy as np

from tests import fusion_cases as FC
from tests import meshrender_restated as MR

SMALL, LARGE = 16, 1024                  # ACEZ_MESHRENDER_SMALL, ACEZ_MESHRENDER_LARGE (the tests check them against acezero_amd._native)
IDENTITY = np.eye(4)


def quad(z=2.0, x0=-0.5, x1=0.5, y0=-0.3, y1=0.3):
    """(vertices, faces) of a fronto-parallel rectangle at depth z for the identity camera: two triangles sharing the diagonal 0-2."""
    v = np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def room_mesh():
    """The box [-ROOM_HALF, ROOM_HALF] as 8 vertices and 12 triangles (two per wall, wall order -x +x -y +y -z +z), and the walls' outward
    axis directions per face (float64 [12,3])."""
    h = FC.ROOM_HALF
    v = np.array([[sx * h[0], sy * h[1], sz * h[2]] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float32)   # index = sx + 2 sy + 4 sz
    walls = [(0, 2, 6, 4), (1, 3, 7, 5), (0, 1, 5, 4), (2, 3, 7, 6), (0, 1, 3, 2), (4, 5, 7, 6)]
    faces = np.array([t for a, b, c, d in walls for t in ((a, b, c), (a, c, d))], np.int32)
    axes = np.repeat(np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], np.float64), 2, 0)
    return v, faces, axes


def room_table(n=6, h=30, w=40, focal=40.0):
    c2w = FC.room_cameras(n)
    return c2w, MR.rows([(h, w)] * n, cam_to_world=c2w, focals=focal)


def grid_mesh(cells=16, pitch=0.11, depth=2.0, tilt=0.6, colours=True):
    """A tilted grid of cells x cells quads (two triangles each) in front of the identity camera: at focal 64 a quad of `pitch` metres
    at `depth` is pitch * 64 / depth px wide, and the tilt (radians about the y axis) stretches the near side and shrinks the far
    one, so the boxes' sample counts straddle a threshold."""
    u = (np.arange(cells + 1) - cells / 2.0) * pitch
    gx, gy = np.meshgrid(u, u)
    x, z = gx * np.cos(tilt), depth + gx * np.sin(tilt)
    v = np.stack([x, gy, z], -1).reshape(-1, 3).astype(np.float32)
    idx = lambda i, j: j * (cells + 1) + i
    faces = np.array([t for j in range(cells) for i in range(cells)
                      for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))], np.int32)
    rgb = np.stack([(37 * np.arange(len(v))) % 256, (91 * np.arange(len(v)) + 5) % 256, (13 * np.arange(len(v)) + 100) % 256], 1).astype(np.uint8)
    return v, faces, rgb if colours else None


def mixed_mesh():
    """One mesh with boxes on both sides of both thresholds for the identity camera at 96 x 128, focal 100: a background rectangle
    that fills the image (two large triangles), a coarse grid in front of it (medium) and a fine grid in front of that (small)."""
    parts = [quad(4.0, -3.0, 3.0, -2.5, 2.5), grid_mesh(6, 0.2, 3.0, 0.3, False)[:2], grid_mesh(12, 0.04, 2.0, 0.5, False)[:2]]
    # a triangle just above and one just below each threshold, side by side: right triangles with legs of a whole number of pixels
    # whose boxes hold (legs + 1)^2 samples when a vertex sits on a pixel
    for k, legs in enumerate((3, 4, 31, 32)):                       # boxes of 16 | 25 and 1024 | 1089 samples
        x = -0.6 + 0.1 * k
        parts.append((np.array([[x, -0.45, 1.0], [x + legs / 100.0, -0.45, 1.0], [x, -0.45 + legs / 100.0, 1.0]], np.float32), np.array([[0, 1, 2]], np.int32)))
    vs, fs, at = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + at)
        at += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def mixed_table():
    return MR.rows([(96, 128)], cam_to_world=IDENTITY[None], focals=100.0)


def box_counts(vertices, faces, table, min_depth=0.05):
    """The largest box (samples) of every drawn triangle-frame, and whether it was clipped: what picks the route."""
    counts, clipped = [], []
    for row in table:
        q, ids, c = MR.camera_triangles(vertices, faces, row, min_depth)
        s = MR.setup(q, row)
        for t in np.unique(ids):
            counts.append(int(s["count"][ids == t].max()))
            clipped.append(bool(c[ids == t].any()))
    return np.array(counts), np.array(clipped)


def routes(vertices, faces, table, min_depth=0.05):
    """(small, medium, large): how many triangle-frames take each route."""
    n, c = box_counts(vertices, faces, table, min_depth)
    large = n > LARGE
    medium = ~large & ((n > SMALL) | (c & (n > 0)))
    small = ~large & ~medium & (n > 0)
    return int(small.sum()), int(medium.sum()), int(large.sum())


# ties and degenerate triangles, for the identity camera at 24 x 32, focal 30
BASE = np.array([[-0.8, -0.6, 2.0], [0.8, -0.6, 2.0], [0.0, 0.7, 2.0]], np.float32)
NEAR = np.array([[-0.2, -0.2, 1.5], [0.2, -0.2, 1.5], [0.0, 0.2, 1.5]], np.float32)
DROPPED = {
    "zero_area": np.array([[-0.5, 0.0, 1.0], [0.0, 0.0, 1.0], [0.5, 0.0, 1.0]], np.float32),
    "nan_vertex": np.array([[-0.5, 0.0, 1.0], [np.nan, 0.3, 1.0], [0.5, 0.0, 1.0]], np.float32),
    "behind": np.array([[-0.5, -0.5, -1.0], [0.5, -0.5, -1.0], [0.0, 0.5, -0.5]], np.float32),
    "guard": np.array([[-0.5, -0.5, 1.0], [0.5, -0.5, 1.0], [1.0e6, 0.0, 0.06]], np.float32),       # 30 * 1e6 / 0.06 px off the centre
}


def small_table(h=24, w=32, focal=30.0):
    return MR.rows([(h, w)], cam_to_world=IDENTITY[None], focals=focal)


def soup(*triangles):
    """(vertices, faces) of triangles float32 [3,3] that share no vertex."""
    return np.concatenate(triangles).astype(np.float32), np.arange(3 * len(triangles), dtype=np.int32).reshape(-1, 3)
