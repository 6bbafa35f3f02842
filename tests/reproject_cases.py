"""Inputs of the reprojection-score tests, shared by tests/test_benchmark_cpu.py (the numpy restatement against hand-written
expectations) and tests/test_benchmark_gpu.py (the HIP passes against the restatement, bit for bit). Every case is
(points float32 [M,3], colours uint8 [M,3], views float32 [T,15], targets uint8 [T,6,8,3], depth_band)."""
import math

import numpy as np

OH, OW = 6, 8
BAND = 0.05
F32 = np.float32


def view_record(m12, f=4.0, cx=4.0, cy=3.0):
    return np.array(list(m12) + [f, cx, cy], np.float32)


IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def band_limit():
    """The largest depth that still counts for a cell whose nearest point is at depth 2."""
    return F32(2.0) * F32(np.float64(1.0) + np.float64(F32(BAND)))


def constructed_scene():
    """Scene A. View 0 is the identity camera with f = 4 cells and the principal point at (4, 3): a point (x, y, 2) lands at
    u = 4 + 2x, v = 3 + 2y. View 1 looks away from everything, view 2 is view 0 moved sideways.
    Returns the case and what view 0 must show: {(row, col): colour}."""
    lim = band_limit()
    pts = [((0, 0, -1), (9, 9, 9)),                                       # behind the camera
           ((0, 0, F32(0.1)), (1, 2, 3)),                                  # exactly on the 0.1 plane: kept, cell (3, 4)
           ((0.05, 0, np.nextafter(F32(0.1), F32(0))), (9, 9, 9)),         # a last place in front of it: dropped (would be cell (3, 6))
           ((0.5, -0.5, 2), (40, 50, 60)),                                 # u = 5.0, v = 2.0 exactly: cell (2, 5)
           ((-1.0, -1.0, 2), (10, 20, 30)),                                # two points of equal depth in cell (1, 2): both count,
           ((-0.9, -0.9, 2), (51, 60, 71)),                                # (61 + 1) // 2 = 31 (30.5 goes up), 40, 51
           ((-1.5, 0.1, 2), (100, 100, 100)),                              # cell (3, 1): the nearest,
           ((-1.5, 0.1, lim), (200, 200, 200)),                            # one exactly on the band limit (counts),
           ((-1.5, 0.1, np.nextafter(lim, F32(np.inf))), (0, 0, 0))]       # one a last place above it (does not)
    pts += [((1, 1, 4), (255, 255, 255))] * 300                            # cell (4, 5): 300 x 255 = 76500 per channel
    points = np.array([p for p, _ in pts], np.float32)
    colours = np.array([c for _, c in pts], np.uint8)
    away = [-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, -100]                       # turned round and 100 m off: every zc < 0
    moved = [1, 0, 0, 0.25, 0, 1, 0, 0, 0, 0, 1, 0]
    views = np.stack([view_record(IDENTITY), view_record(away), view_record(moved)])
    targets = np.full((3, OH, OW, 3), 7, np.uint8)
    expect0 = {(3, 4): (1, 2, 3), (2, 5): (40, 50, 60), (1, 2): (31, 40, 51), (3, 1): (150, 150, 150), (4, 5): (255, 255, 255)}
    return (points, colours, views, targets, BAND), expect0


def edge_scene():
    """Scene B: a camera whose principal point is (-0.0, -0.0) and whose zero matrix entries are -0.0, so that a point with
    x = -0.0 projects to u = -0.0 (inside: cell 0). A point (x, y, 2) lands at u = 2x, v = 2y."""
    nz = -0.0
    m = [1, nz, nz, nz, nz, 1, nz, nz, 0, 0, 1, 0]
    pts = [((nz, 1, 2), (10, 10, 10)),                                     # u = -0.0: cell (2, 0)
           ((-1e-30, 1, 2), (99, 99, 99)),                                 # u < 0: outside
           ((4, 1, 2), (99, 99, 99)),                                      # u = 8 = ow: outside
           ((np.nextafter(F32(4), F32(0)), 1, 2), (20, 20, 20)),           # u a last place below 8: cell (2, 7)
           ((1, 3, 2), (99, 99, 99)),                                      # v = 6 = oh: outside
           ((1, np.nextafter(F32(3), F32(0)), 2), (30, 30, 30)),           # v a last place below 6: cell (5, 2)
           ((1, -1e-30, 2), (99, 99, 99))]                                 # v < 0: outside
    points = np.array([p for p, _ in pts], np.float32)
    colours = np.array([c for _, c in pts], np.uint8)
    views = view_record(m, cx=nz, cy=nz)[None]
    targets = np.zeros((1, OH, OW, 3), np.uint8)
    expect = {(2, 0): (10, 10, 10), (2, 7): (20, 20, 20), (5, 2): (30, 30, 30)}
    return (points, colours, views, targets, BAND), expect


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def random_case(n_points, n_views=3, seed=0, quantise_depth=False):
    """A cloud in front of n_views slightly different cameras; quantise_depth: depths on a grid of 1/4, so that cells hold points of
    equal depth (index ties) and points exactly on a band limit are common."""
    rng = np.random.default_rng([seed, n_points, n_views])
    points = np.stack([rng.uniform(-2.5, 2.5, n_points), rng.uniform(-2, 2, n_points), rng.uniform(0.5, 5, n_points)], 1)
    if quantise_depth:
        points[:, 2] = np.round(points[:, 2] * 4) / 4
    colours = rng.integers(0, 256, (n_points, 3)).astype(np.uint8)
    views = []
    for _ in range(n_views):
        m = np.eye(4)[:3]
        m[:, :3] = _rot(*rng.normal(0, 0.05, 3))
        m[:, 3] = rng.normal(0, 0.2, 3)
        views.append(view_record(m.reshape(-1), f=float(rng.uniform(3, 5)), cx=float(rng.uniform(3.5, 4.5)), cy=float(rng.uniform(2.5, 3.5))))
    targets = rng.integers(0, 256, (n_views, OH, OW, 3)).astype(np.uint8)
    return points.astype(np.float32), colours, np.stack(views), targets, BAND


# ------------------------------------------------------------------------------------------------------- sensitivity
def sensitivity_scene(turn_deg=2.0):
    """The textured room of acezero_amd.synth seen by 12 cameras on an arc (192 x 256 px frames, 24 x 32 cells): every 8th frame from
    index 4 on is held out (frame 4). Sources: the other frames' cells, each a point at its centre's true depth coloured with its
    cell mean. Returns (points, colours, views_true, views_turned, targets): the turned views are the held-out cameras rotated by
    turn_deg about their vertical axis. Known geometry, no training."""
    from acezero_amd import synth
    from tests import reproject_restated as rr
    h, w, focal = 192, 256, 210.0
    seq = synth.render_room_sequence(seed=2089, n_frames=12, h=h, w=w, focal=focal, arc_deg=24.0, device="cpu")
    grey = ((seq["images"][:, 0] * 0.25 + 0.4).clamp(0, 1) * 255).round().numpy().astype(np.uint8)
    means = rr.cell_means(np.repeat(grey[..., None], 3, axis=3))          # [12,24,32,3]
    poses = seq["poses"].numpy().astype(np.float64)                       # camera -> world
    depth = seq["depth"].numpy().astype(np.float64)
    test = list(range(12))[4::8]
    train = [i for i in range(12) if i not in test]
    oh, ow = h // 8, w // 8
    gx, gy = np.meshgrid(np.arange(ow) * 8 + 4.0, np.arange(oh) * 8 + 4.0)
    pts, clr = [], []
    for i in train:
        cam = np.stack([(gx - w / 2.0) / focal * depth[i], (gy - h / 2.0) / focal * depth[i], depth[i]], -1).reshape(-1, 3)
        pts.append(cam @ poses[i, :3, :3].T + poses[i, :3, 3])
        clr.append(means[i].reshape(-1, 3))
    a = math.radians(turn_deg)
    turn = np.array([[math.cos(a), 0, math.sin(a), 0], [0, 1, 0, 0], [-math.sin(a), 0, math.cos(a), 0], [0, 0, 0, 1.0]])
    w2c_true = np.stack([np.linalg.inv(poses[i]) for i in test])
    w2c_turn = np.stack([np.linalg.inv(poses[i] @ turn) for i in test])
    views_true = rr.make_views(w2c_true, focal, w / 2.0, h / 2.0)
    views_turn = rr.make_views(w2c_turn, focal, w / 2.0, h / 2.0)
    return np.concatenate(pts).astype(np.float32), np.concatenate(clr).astype(np.uint8), views_true, views_turn, means[test]
