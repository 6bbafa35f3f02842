"""Scenes for the tracking tests (tests/test_track_cpu.py, tests/test_track_gpu.py) on tests/fusion_cases.py's box room: the
wide-lens room with its seeded pose perturbation, and the small mixed call of the parity tests. A helper module, not a test file."""
import functools

import numpy as np

from tests import fusion_cases as FC

# ------------------------------------------------------------------------------------------------------------- the wide-lens room
ROOM_FRAMES, ROOM_H, ROOM_W, ROOM_FOCAL = 24, 60, 80, 30.0
VOXEL, TRUNCATION = 0.02, 0.08
SIGMA_T, SIGMA_R_DEG = 0.01, 0.5


def snapped_box(half, voxel_size=VOXEL, truncation=TRUNCATION):
    """dict(origin, dims, voxel_size, truncation) of the volume around the box [-half, half], padded by the truncation and snapped
    outwards to multiples of the voxel size (acezero_amd.fusion.bounds_from_frames' rule), so that the room's walls lie midway
    between voxel planes as tests/fusion_cases.py says."""
    half = np.asarray(half, np.float64)
    lo = np.floor((-half - truncation) / voxel_size).astype(np.int64)
    hi = np.ceil((half + truncation) / voxel_size).astype(np.int64)
    return dict(origin=tuple((lo * voxel_size).astype(np.float32)), dims=tuple(int(d) for d in hi - lo + 1), voxel_size=voxel_size,
                truncation=truncation)


ROOM_VOLUME = snapped_box(FC.ROOM_HALF)


def rotation(rotvec):
    """Rodrigues' formula: the rotation matrix of a rotation vector (radians)."""
    rotvec = np.asarray(rotvec, np.float64)
    angle = np.linalg.norm(rotvec)
    if angle == 0.0:
        return np.eye(3)
    k = rotvec / angle
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def perturb(c2w, seed, sigma_t=SIGMA_T, sigma_r_deg=SIGMA_R_DEG):
    """The poses moved about each camera centre by N(0, sigma_t) metres and N(0, sigma_r_deg) degrees per axis."""
    g = np.random.default_rng(seed)
    out = np.array(c2w, np.float64)
    for T in out:
        T[:3, :3] = rotation(np.deg2rad(g.normal(scale=sigma_r_deg, size=3))) @ T[:3, :3]
        T[:3, 3] += g.normal(scale=sigma_t, size=3)
    return out


@functools.lru_cache(maxsize=None)
def room(n=ROOM_FRAMES, h=ROOM_H, w=ROOM_W, focal=ROOM_FOCAL, seed=11):
    """(depths: list of uint16 [h,w], true camera -> world [n,4,4], perturbed camera -> world [n,4,4], focal). Treat as read-only."""
    truth = FC.room_cameras(n)
    return [FC.room_depth(T, h, w, focal) for T in truth], truth, perturb(truth, seed), focal


# What tests/track_restated.py gives on this room, run on the CPU (tests/test_track_cpu.py prints the figures it asserts): the bounds of
# the CPU and the GPU tests are 1.25 x these, as DESIGN.md section 4j does for the sphere and the room; DESIGN.md section 4q lists them.
HEADROOM = 1.25
MEASURED = dict(
    recovery_t_mean=0.000719, recovery_t_max=0.001553,             # metres, against the truth-pose volume, from 16.5 mm mean
    recovery_r_mean=0.02429, recovery_r_max=0.04420,               # degrees, from 0.69 mean
    round_rpe=(0.006438, 0.005006, 0.004116),                      # metres: mean relative pose error after rounds 1, 2, 3, from 25.1 mm
    round_rms=(0.003048, 0.001821, 0.001648))                      # metres: mean rms residual at the end of rounds 1, 2, 3
MIN_USED = 0.9                                                     # fixed, not measured: the share of its non-zero pixels a frame uses


# ------------------------------------------------------------------------------------------------------------- the parity call
SMALL_VOLUME = dict(origin=(-0.24, -0.2, -0.28), dims=(24, 20, 28), voxel_size=VOXEL, truncation=TRUNCATION)
# A box room whose + walls lie in the LAST cell of SMALL_VOLUME on every axis (its last voxel centres are at 0.22, 0.18, 0.26).
SMALL_HALF = np.array([0.21, 0.17, 0.25])
SMALL_MIN_WEIGHT = 2.0


@functools.lru_cache(maxsize=None)
def analytic_volume():
    """(tsdf, weight float32 [28,20,24]) of SMALL_VOLUME: the exact truncated distance to SMALL_HALF's walls (positive inside the
    room) in units of the truncation; every voxel is observed, with weight 2 = SMALL_MIN_WEIGHT except a lattice of voxels of weight
    1, just below it, so that about one cell in eight has an unknown corner. Treat as read-only."""
    nx, ny, nz = SMALL_VOLUME["dims"]
    o = np.asarray(SMALL_VOLUME["origin"], np.float32).astype(np.float64)
    k, j, i = np.mgrid[0:nz, 0:ny, 0:nx]
    p = np.stack([o[0] + i * VOXEL, o[1] + j * VOXEL, o[2] + k * VOXEL], -1)
    tsdf = np.clip((SMALL_HALF - np.abs(p)).min(-1) / TRUNCATION, -1.0, 1.0).astype(np.float32)
    weight = np.where((i % 5 == 0) & (j % 4 == 0) & (k % 3 == 0), 1.0, 2.0).astype(np.float32)
    return tsdf, weight


@functools.lru_cache(maxsize=None)
def mixed_call():
    """The frames of the parity tests, tracked against analytic_volume(): dict(depths, poses, focals).
      0  60 x 80, perturbed
      1  45 x 61 (2745 pixels: a partial last tile, ragged rows), another focal, perturbed
      2  all zero (no sample: degenerate, the input pose kept)
      3  posed to look away, its points 3 m outside the volume (no sample)
      4  a plane of points through the volume's last voxel centre: they straddle the last cell on every axis (the i0 <= n - 2 edge)
      5  frame 0's image at its true pose (it converges early)
    Treat as read-only."""
    eye = np.array([0.01, -0.005, 0.015])
    T0 = FC.look_at(eye, eye + np.array([1.0, 0.2, 0.4]))
    T1 = FC.look_at(-eye, -eye + np.array([-0.6, -0.3, 1.0]))
    d0 = FC.room_depth(T0, 60, 80, 28.0, SMALL_HALF)
    d1 = FC.room_depth(T1, 45, 61, 23.5, SMALL_HALF)
    away = FC.look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    d3 = np.full((20, 24), 3000, np.uint16)
    corner = np.asarray(SMALL_VOLUME["origin"], np.float64) + (np.asarray(SMALL_VOLUME["dims"]) - 1) * VOXEL
    T4 = FC.look_at(corner - 0.3 * np.ones(3) / np.sqrt(3.0), corner)
    iy, ix = np.mgrid[0:24, 0:32]
    d4 = (280 + (7 * ix + 3 * iy) % 29).astype(np.uint16)           # 2 cm before the corner to 1 cm beyond it
    depths = [d0, d1, np.zeros((33, 47), np.uint16), d3, d4, d0.copy()]
    poses = np.stack([perturb(T0[None], 3, 0.004, 0.3)[0], perturb(T1[None], 4, 0.004, 0.3)[0], T0, away, T4, T0])
    return dict(depths=depths, poses=poses, focals=np.array([28.0, 23.5, 30.0, 20.0, 200.0, 28.0]))


# ------------------------------------------------------------------------------------------------------------- the sparse scene
SPARSE_HALF = np.array([0.17, 0.15, 0.21])        # a room whose walls lie in the outer blocks of SMALL_VOLUME: its middle gets no block


@functools.lru_cache(maxsize=None)
def sparse_scene():
    """dict(depths, truth, poses, focal): 10 frames of 30 x 40 from the middle of SPARSE_HALF's room, their true and perturbed poses,
    and one more frame (the last) whose points float 3 cm before the camera, in the room's middle, where no block is allocated."""
    truth = FC.room_cameras(10, radius=0.02)
    truth[:, 1, 3] *= 0.2
    depths = [FC.room_depth(T, 30, 40, 14.0, SPARSE_HALF) for T in truth]
    return dict(depths=depths + [np.full((30, 40), 30, np.uint16)], truth=np.concatenate([truth, truth[:1]]),
                poses=np.concatenate([perturb(truth, 5, 0.004, 0.3), truth[:1]]), focal=14.0)
