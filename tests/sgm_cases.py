"""The scene of tests/mvs_cases.py with a textureless region, for the aggregation tests (tests/test_sgm_cpu.py,
tests/test_sgm_gpu.py). A helper module, not a test file.

A band of the back wall, 0.05 < y < 0.75 and |x| > 0.4 in world coordinates (0.7 m high, to both sides of the box), is painted a
constant grey. It is far wider than the 9 x 9 prefilter plus the 5 x 5 window (0.7 m is about 38 px at this focal), so most of it is
truly flat to the matcher. 64 planes: with mvs_cases.PLANES = 32 the plane step at the wall (1.6 %) exceeds the check's 1 %
tolerance, and flat pixels quantised to neighbouring planes vote each other out."""
import numpy as np

from tests import mvs_cases as MC
from tests.mvs_restated import Row

N, PLANES, SOURCES, KEEP, WINDOW = 6, 64, 4, 2, 2
BAND_Y, BAND_X, GREY = (0.05, 0.75), 0.4, 128


def band_of(depth, c2w, h=MC.H, w=MC.W, focal=MC.FOCAL):
    """bool [h,w]: the pixels whose world point, from the exact depth and the pose, lies on the back wall inside the band."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    cam = np.stack([(xs - w / 2.0) / focal * depth, (ys - h / 2.0) / focal * depth, depth], -1)
    p = cam @ c2w[:3, :3].T + c2w[:3, 3]
    return (np.abs(p[..., 2] - MC.WALL_Z) < 1e-6) & (p[..., 1] > BAND_Y[0]) & (p[..., 1] < BAND_Y[1]) & (np.abs(p[..., 0]) > BAND_X)


def scene(n=N):
    """(images list of uint8 [H,W], exact depth list of float64 [H,W], c2w [n,4,4], rows, band masks list of bool [H,W])."""
    c2w = MC.cameras(n)
    images, depths, bands = [], [], []
    for T in c2w:
        grey, depth = MC.render(T)
        band = band_of(depth, T)
        images.append(np.where(band, np.uint8(GREY), grey))
        depths.append(depth)
        bands.append(band)
    rows = [Row(np.linalg.inv(T), MC.FOCAL, MC.W / 2.0, MC.H / 2.0, MC.H, MC.W) for T in c2w]
    return images, depths, c2w, rows, bands


def in_band_region(points):
    """bool [n]: points [n,3] within 5 cm of the wall and inside the band's x and y: the mesh vertices that fill the band."""
    p = np.asarray(points, np.float64)
    return (np.abs(p[:, 2] - MC.WALL_Z) < 0.05) & (p[:, 1] > BAND_Y[0]) & (p[:, 1] < BAND_Y[1]) & (np.abs(p[:, 0]) > BAND_X)


def write_scene(folder, n=N, confidence=5000):
    """The band scene's frames as PNGs and a pose file with the ground-truth poses: (pose file, image glob)."""
    import os
    from PIL import Image
    from acezero_amd.session import write_pose_file
    images, _, c2w, _, _ = scene(n)
    names = []
    for k, im in enumerate(images):
        names.append(os.path.join(folder, f"frame_{k:03d}.png"))
        Image.fromarray(np.stack([im] * 3, -1)).save(names[-1])
    write_pose_file(os.path.join(folder, "poses.txt"), names, c2w, [confidence] * n, MC.FOCAL)
    return os.path.join(folder, "poses.txt"), os.path.join(folder, "frame_*.png")
