"""Scenes for the plane-sweep stereo tests (tests/test_mvs_cpu.py, tests/test_mvs_gpu.py). A helper module, not a test file.

The scene: a back wall z = WALL_Z and a box in front of its middle third (front face z = BOX_Z, |x| <= BOX_X, |y| <= BOX_Y, its sides
running back to the wall), so there is a depth step and, from cameras off the axis, occlusion. The texture is multi-octave value
noise in WORLD coordinates, so every camera sees the same surface. Depth is exact: the z-depth of the ray through pixel (x, y),
direction ((x - ppx) / f, (y - ppy) / f, 1), the pixel convention of include/acez.h sections K and L. All in numpy float64."""
import numpy as np

from tests.fusion_cases import look_at
from tests.mvs_restated import Row

WALL_Z, BOX_Z, BOX_X, BOX_Y = 2.0, 1.5, 0.35, 0.6
H, W, FOCAL = 96, 128, 110.0
Z_NEAR, Z_FAR = 1.0, 3.0
OCTAVES = ((0.30, 1.0), (0.15, 0.8), (0.075, 0.6), (0.04, 0.4))  # (wavelength in metres, amplitude); a pixel is 0.014 - 0.018 m
PLANES, SOURCES = 32, 4


def _lattice(ix, iy, iz, seed):
    """A fixed pseudo-random number in [0, 1) per integer lattice point (32-bit integer hash)."""
    h = (ix.astype(np.int64) * 73856093) ^ (iy.astype(np.int64) * 19349663) ^ (iz.astype(np.int64) * 83492791) ^ (seed * 2654435761)
    h &= 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 2246822519) & 0xFFFFFFFF
    h = ((h ^ (h >> 13)) * 3266489917) & 0xFFFFFFFF
    h ^= h >> 16
    return h.astype(np.float64) / 4294967296.0


def texture(p):
    """Grey value 0 .. 255 (float64) of the world points p [..., 3]: trilinear value noise, smoothstep weights, three octaves."""
    out, total = np.zeros(p.shape[:-1]), 0.0
    for o, (wavelength, amp) in enumerate(OCTAVES):
        q = p / wavelength
        i = np.floor(q)
        f = q - i
        f = f * f * (3.0 - 2.0 * f)
        i = i.astype(np.int64)
        acc = np.zeros(p.shape[:-1])
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    wgt = (f[..., 0] if dx else 1 - f[..., 0]) * (f[..., 1] if dy else 1 - f[..., 1]) * (f[..., 2] if dz else 1 - f[..., 2])
                    acc += wgt * _lattice(i[..., 0] + dx, i[..., 1] + dy, i[..., 2] + dz, o + 1)
        out += amp * acc
        total += amp
    return 255.0 * out / total


def render(c2w, h=H, w=W, focal=FOCAL, ppx=None, ppy=None):
    """(grey uint8 [h,w], exact z-depth float64 [h,w]) of the scene from the camera -> world pose c2w."""
    ppx, ppy = (w / 2.0 if ppx is None else ppx), (h / 2.0 if ppy is None else ppy)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    d_cam = np.stack([(xs - ppx) / focal, (ys - ppy) / focal, np.ones((h, w))], -1)
    d, o = d_cam @ c2w[:3, :3].T, c2w[:3, 3]
    best = (WALL_Z - o[2]) / d[..., 2]                            # the wall; every camera of these tests looks towards +z
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (BOX_Z - o[2]) / d[..., 2]                            # the box's front face
        p = o + t[..., None] * d
        hit = (t > 0) & (np.abs(p[..., 0]) <= BOX_X) & (np.abs(p[..., 1]) <= BOX_Y)
        best = np.where(hit & (t < best), t, best)
        for axis, half, other, other_half in ((0, BOX_X, 1, BOX_Y), (1, BOX_Y, 0, BOX_X)):      # its four sides
            for sign in (-1.0, 1.0):
                t = (sign * half - o[axis]) / d[..., axis]
                p = o + t[..., None] * d
                hit = (t > 0) & (np.abs(p[..., other]) <= other_half) & (p[..., 2] >= BOX_Z) & (p[..., 2] <= WALL_Z)
                best = np.where(hit & (t < best), t, best)
    point = o + best[..., None] * d
    grey = np.clip(np.rint(texture(point)), 0, 255).astype(np.uint8)
    return grey, best                                             # d_cam has z = 1: the ray parameter is the z-depth


def cameras(n=6, spacing=0.15):
    """n camera -> world poses on a line along x, each turned a little towards the box and tilted in turn."""
    out = []
    for k in range(n):
        x = (k - (n - 1) / 2.0) * spacing
        eye = np.array([x, 0.02 * ((k % 3) - 1), 0.0])
        out.append(look_at(eye, (0.3 * x, 0.05 * ((k % 2) - 0.5), WALL_Z)))
    return np.stack(out)


def scene(n=6):
    """(images list of uint8 [H,W], exact depth list of float64 [H,W], c2w [n,4,4], rows) of the test scene."""
    c2w = cameras(n)
    pairs = [render(T) for T in c2w]
    rows = [Row(np.linalg.inv(T), FOCAL, W / 2.0, H / 2.0, H, W) for T in c2w]
    return [p[0] for p in pairs], [p[1] for p in pairs], c2w, rows


def nearest_sources(n, k):
    """For each of n cameras on the line the k nearest others, nearest first, ties to the lower index."""
    return [sorted((j for j in range(n) if j != i), key=lambda j: (abs(j - i), j))[:k] for i in range(n)]


def silhouette(depth, margin=6):
    """Pixels within `margin` px (horizontally) of a depth step of more than 0.2 m in a row: the box's vertical silhouette."""
    jump = np.abs(np.diff(depth, axis=1)) > 0.2
    out = np.zeros(depth.shape, bool)
    ys, xs = np.nonzero(jump)
    for y, x in zip(ys, xs):
        out[y, max(0, x - margin + 1):x + margin + 1] = True
    return out


# ---------------------------------------------------------------------------------------------------- edge cases for the GPU parity
def random_frames(seed, sizes, focals, eyes, targets, smooth=3):
    """Frames of smoothed noise (so that costs vary from plane to plane and ties are rare) with look_at poses: (images, rows)."""
    rng = np.random.default_rng(seed)
    images, rows = [], []
    for (h, w), f, eye, target in zip(sizes, focals, eyes, targets):
        a = rng.uniform(0, 255, (h + 2 * smooth, w + 2 * smooth))
        k = 2 * smooth + 1
        ii = np.zeros((a.shape[0] + 1, a.shape[1] + 1))
        ii[1:, 1:] = a.cumsum(0).cumsum(1)
        box = (ii[k:, k:] - ii[:-k, k:] - ii[k:, :-k] + ii[:-k, :-k]) / (k * k)
        box = (box - box.min()) / (box.max() - box.min()) * 255.0
        images.append(np.rint(box).astype(np.uint8))
        rows.append(Row(np.linalg.inv(look_at(eye, target)), f, w / 2.0 + 0.3, h / 2.0 - 0.2, h, w))
    return images, rows


def write_scene(folder, n=6, confidence=5000):
    """The scene's frames as PNGs (grey replicated to RGB) and a pose file with the ground-truth poses: (pose file, image glob)."""
    import os
    from PIL import Image
    from acezero_amd.session import write_pose_file
    images, _, c2w, _ = scene(n)
    names = []
    for k, im in enumerate(images):
        names.append(os.path.join(folder, f"frame_{k:03d}.png"))
        Image.fromarray(np.stack([im] * 3, -1)).save(names[-1])
    write_pose_file(os.path.join(folder, "poses.txt"), names, c2w, [confidence] * n, FOCAL)
    return os.path.join(folder, "poses.txt"), os.path.join(folder, "frame_*.png")
