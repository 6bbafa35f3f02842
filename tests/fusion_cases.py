"""Scenes for the TSDF fusion tests (tests/test_fusion_cpu.py, tests/test_fusion_gpu.py): analytic z-depth of a sphere and of the
inside of a box room, rendered in numpy float64, quantised to uint16 millimetres, rays that hit nothing set to 0. A helper module,
not a test file. The pixel index is the image coordinate and the principal point the image centre (w / 2, h / 2), the project's
convention."""
import numpy as np

SPHERE_R = 0.3
# The room is the box [-half, +half]; the cameras stand inside. Volumes are snapped to multiples of the 0.02 m voxel, so these walls
# lie midway between voxel planes. (At a concave edge a surface-net vertex is the mean of crossings on two walls and lies off both by
# up to half the distance of the free voxel from the wall: v / 4 here, v / 2 for a wall that passes through voxel centres.)
ROOM_HALF = np.array([0.61, 0.51, 0.71])


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """Camera -> world 4x4 of an OpenCV camera (x right, y down, z forward) at `eye` looking at `target`."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    upv = np.asarray(up, np.float64)
    if abs(np.dot(z, upv)) > 0.99:
        upv = np.array([0.0, 0.0, 1.0])
    x = np.cross(-upv, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
    return T


def _rays(h, w, focal):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([(xs - w / 2.0) / focal, (ys - h / 2.0) / focal, np.ones((h, w))], -1)       # z component 1: the ray parameter is z-depth


def _quantise(z):
    return np.where(np.isfinite(z) & (z > 0), np.rint(z * 1000.0), 0).clip(0, 65535).astype(np.uint16)


def sphere_depth(c2w, h, w, focal, radius=SPHERE_R):
    """uint16 millimetres [h,w] of the sphere of `radius` at the world origin."""
    d = _rays(h, w, focal)
    c = np.linalg.inv(c2w)[:3, 3]                                                               # the sphere's centre in the camera
    a, b, cc = (d * d).sum(-1), -2.0 * (d @ c), c @ c - radius * radius
    disc = b * b - 4.0 * a * cc
    with np.errstate(invalid="ignore"):
        s = (-b - np.sqrt(disc)) / (2.0 * a)
    return _quantise(np.where(disc > 0, s, np.nan))


def sphere_cameras(distance=1.0):
    """14 inward-looking cameras: on the 6 axes and the 8 diagonals."""
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    dirs += [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    return np.stack([look_at(distance * np.asarray(d, np.float64) / np.linalg.norm(d), (0, 0, 0)) for d in dirs])


def sphere_scene(h=60, w=80, focal=80.0):
    """(depths list of uint16 [h,w], c2w [14,4,4], focal) of the sphere test: v = 0.02, tau = 4 v, volume 48^3 around the origin."""
    c2w = sphere_cameras()
    return [sphere_depth(T, h, w, focal) for T in c2w], c2w, focal


SPHERE_VOLUME = dict(origin=(-0.47, -0.47, -0.47), dims=(48, 48, 48), voxel_size=0.02, truncation=0.08)


def room_depth(c2w, h, w, focal, half=ROOM_HALF):
    """uint16 millimetres [h,w] of the inside of the box [-half, half] seen from a camera inside it."""
    d = _rays(h, w, focal) @ c2w[:3, :3].T                                                      # world directions, per unit of z-depth
    o = c2w[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (half - o) / d, np.where(d < 0, (-half - o) / d, np.inf))
    return _quantise(t.min(-1))


def room_rgb(c2w, h, w, focal, half=ROOM_HALF):
    """uint8 [h,w,3]: a colour per wall, so that the colour path sees different values."""
    d = _rays(h, w, focal) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (half - o) / d, np.where(d < 0, (-half - o) / d, np.inf))
    wall = t.argmin(-1) * 2 + (np.take_along_axis(d, t.argmin(-1)[..., None], -1)[..., 0] > 0)
    palette = np.array([[220, 60, 60], [60, 220, 60], [60, 60, 220], [220, 220, 60], [60, 220, 220], [220, 60, 220]], np.uint8)
    return palette[wall]


def room_cameras(n, radius=0.1):
    """n cameras on a small circle around the room's centre, looking outwards and slightly up and down in turn."""
    out = []
    for k in range(n):
        a = 2.0 * np.pi * k / n
        eye = np.array([radius * np.cos(a), 0.05 * ((k % 3) - 1), radius * np.sin(a)])
        out.append(look_at(eye, eye + np.array([np.cos(a), 0.35 * ((k % 3) - 1), np.sin(a)])))
    return np.stack(out)


def write_room_scene(folder, n, h, w, focal, rgb_scale=2, confidence=5000):
    """n frames of the box room as 16-bit depth PNGs of h x w, RGB PNGs rgb_scale times as large and a pose file with the ground-truth
    poses and the focal length in pixels of the RGB images (session.write_pose_file); returns fuse_depth.py's arguments."""
    import os
    from PIL import Image
    from acezero_amd.session import write_pose_file
    c2w = room_cameras(n)
    os.makedirs(os.path.join(folder, "depth"), exist_ok=True)
    names = []
    for k in range(n):
        names.append(os.path.join(folder, f"frame_{k:03d}.png"))
        Image.fromarray(room_rgb(c2w[k], h * rgb_scale, w * rgb_scale, focal * rgb_scale)).save(names[-1])
        Image.fromarray(room_depth(c2w[k], h, w, focal)).save(os.path.join(folder, "depth", f"frame_{k:03d}.png"))
    write_pose_file(os.path.join(folder, "poses.txt"), names, c2w, [confidence] * n, focal * rgb_scale)
    return [os.path.join(folder, "poses.txt"), os.path.join(folder, "frame_*.png"), os.path.join(folder, "mesh.ply"), "--depth_files",
            os.path.join(folder, "depth", "*.png")]


def read_mesh_ply(path):
    """(vertices float32 [V,3], colours uint8 [V,3], faces int32 [F,3]) of a file formats.write_ply wrote."""
    import re
    blob = open(path, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    n_v, n_f = int(re.search(rb"element vertex (\d+)", head).group(1)), int(re.search(rb"element face (\d+)", head).group(1))
    assert len(body) == n_v * 16 + n_f * 13
    vrec = np.frombuffer(body[:n_v * 16], dtype=[("xyz", "<f4", (3,)), ("rgba", "u1", (4,))])
    frec = np.frombuffer(body[n_v * 16:], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    assert (frec["n"] == 3).all()
    return vrec["xyz"].copy(), vrec["rgba"][:, :3].copy(), frec["v"].copy()


def wall_distance(points, half=ROOM_HALF):
    """Distance of every point [n,3] to the nearest wall plane of the room."""
    p = np.asarray(points, np.float64)
    return np.abs(half[None, :] - np.abs(p)).min(-1)


def mesh_edge_counts(faces):
    """(number of faces at every undirected edge, number of times every DIRECTED edge occurs): a closed, consistently oriented
    manifold has 2 everywhere in the first and 1 everywhere in the second."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    _, directed = np.unique(e, axis=0, return_counts=True)
    _, undirected = np.unique(np.sort(e, 1), axis=0, return_counts=True)
    return undirected, directed


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)
