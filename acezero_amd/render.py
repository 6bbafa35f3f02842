"""Reconstruction video (train_ace.py / register_mapping.py / ace_zero.py --render_visualization True, render_final_sweep.py,
export_cameras.py): the behaviour of the reference's ace_visualizer.py / ace_vis_util.py, drawn by the HIP rasteriser of
csrc/render_api.hip (acez_render_frame) instead of pyrender on OpenGL.

Every frame is two layers drawn on the device: the point cloud (2 x 2 px points, depth-tested) and the camera geometry (flat RGBA
triangles and, in the registration phase, the query's image as a textured quad inside its frustum, depth-tested among themselves),
on top of the points. Only the finished frame crosses to the host, where histograms and captions are drawn with matplotlib and the
PNG is written with PIL as frame_%05d.png."""
import ctypes as C
import logging
import math
import os
import pickle

import numpy as np
import torch

from . import _native as N
from .formats import read_ace_pose_file, read_pose_file, write_ply

_logger = logging.getLogger("acezero_amd")

WIDTH, HEIGHT = 1280, 720          # output resolution (ace_visualizer.py render_width / render_height)
ZNEAR, ZFAR = 0.05, 1000.0         # clip planes of the observing camera
THICKNESS = 0.005                  # half-width of the bars of frustums and camera paths (metres)
FRAMECOUNT_TRANSITION = 10         # frames that grow the fully trained map at the end of mapping
PAN_ANGLE_COVERAGE = 60            # degrees: opening angle of the mapping pan
MAPPING_FRAME_COUNT = 100          # length of one mapping pan (ace_trainer.py passes 100)
SWEEP_FRAME_COUNT = 150            # render_final_sweep.py
RELOC_DURATION = 60                # at most this many registration frames (longer query sets are sub-sampled)
CONFIDENCE_THRESHOLD = 1000
SWEEP_ITERATIONS_THRESHOLD = 10

GL_FROM_CV = np.array([[1, -1, -1, 1], [-1, 1, 1, -1], [-1, 1, 1, -1], [1, 1, 1, 1]], np.float64)


def cv_to_gl(pose):
    """Camera pose OpenCV <-> OpenGL convention (the same element-wise sign flip both ways)."""
    return GL_FROM_CV * np.asarray(pose, np.float64)


# ------------------------------------------------------------------------------------------------------------- colour maps
def retro_colors():
    """Dark magenta to bright cyan, 256 x 3 in [0, 1]: the reference's map for reprojection errors."""
    from matplotlib.colors import LinearSegmentedColormap
    nodes = [0.0, 0.4, 0.7, 0.85, 0.95, 1.0]
    red = [0.073, 0.325, 0.286, 0.266, 0.0, 1.0]
    green = [0.0, 0.058, 0.470, 0.827, 1.0, 1.0]
    blue = [0.057, 0.223, 0.752, 0.988, 1.0, 1.0]
    seg = {k: [[x, c, c] for x, c in zip(nodes, ch)] for k, ch in (("red", red), ("green", green), ("blue", blue))}
    return LinearSegmentedColormap("retro", segmentdata=seg, N=256)(np.linspace(0, 1, 257))[1:, :3]


def colormap(name, lo, hi, n):
    import matplotlib
    return matplotlib.colormaps[name](np.linspace(lo, hi, n))[:, :3]


def errors_to_colors(errors, max_error, cmap):
    """Reprojection errors -> (colours [n,3] in 0..255, normalised errors in [0,1], 1 = no error)."""
    norm = 1 - (np.asarray(errors, np.float64) / max_error).clip(0, 1)
    return cmap[(norm * 255).astype(int)] * 255, norm


def reloc_color_map(confidence_threshold=CONFIDENCE_THRESHOLD, conf_vis_threshold=5000):
    neg = int(confidence_threshold / conf_vis_threshold * 256)
    return np.concatenate([colormap("cool", 1, 0, neg), colormap("summer", 1, 0, 256 - neg)])


# ------------------------------------------------------------------------------------------------------------------ geometry
class Mesh:
    """Flat-coloured triangles: vertices [k,3], faces [f,3] and one RGBA per face."""

    def __init__(self, verts=None, faces=None, rgba=None):
        self.verts = np.zeros((0, 3)) if verts is None else np.asarray(verts, np.float64)
        self.faces = np.zeros((0, 3), np.int64) if faces is None else np.asarray(faces, np.int64)
        self.rgba = np.zeros((0, 4), np.uint8) if rgba is None else np.asarray(rgba, np.uint8)

    @staticmethod
    def concatenate(meshes):
        out, off = Mesh(), 0
        vs, fs, cs = [], [], []
        for m in meshes:
            vs.append(m.verts); fs.append(m.faces + off); cs.append(m.rgba)
            off += len(m.verts)
        if vs:
            out.verts, out.faces, out.rgba = np.concatenate(vs), np.concatenate(fs), np.concatenate(cs)
        return out

    def triangles(self):
        """float32 [f,3,3] vertex coordinates and uint8 [f,4] colours, as acez_render_frame takes them."""
        return np.ascontiguousarray(self.verts[self.faces], np.float32), np.ascontiguousarray(self.rgba, np.uint8)


def _quads_to_tris(quads):
    q = np.asarray(quads, np.int64)
    return np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])


def _rgba(color, n):
    c = np.asarray(color, np.float64).reshape(-1)
    c = np.concatenate([c[:3], [255]]) if len(c) == 3 else c[:4]
    return np.tile(np.clip(c, 0, 255).astype(np.uint8), (n, 1))


def cuboid_from_line(start, end, color=(255, 0, 255), thickness=THICKNESS):
    """A long box of square cross-section 2 * thickness along the segment start -> end: 8 vertices, 12 triangles. The cross-section's
    orientation is fixed by the world axis least aligned with the segment (the reference draws a random one)."""
    a, b = np.asarray(start, np.float64), np.asarray(end, np.float64)
    d = b - a
    d = d / np.linalg.norm(d)
    helper = np.eye(3)[int(np.argmin(np.abs(d)))]
    px = np.cross(d, helper)
    px /= np.linalg.norm(px)
    py = np.cross(d, px)
    verts = [node + thickness * (py * oy + px * ox) for node in (a, b) for ox in (-1, 1) for oy in (-1, 1)]
    quads = [(4, 5, 1, 0), (5, 7, 3, 1), (7, 6, 2, 3), (6, 4, 0, 2), (0, 1, 3, 2), (6, 7, 5, 4)]
    faces = _quads_to_tris(quads)
    return Mesh(np.array(verts), faces, _rgba(color, len(faces)))


def frustum_marker(pose_gl, color=(255, 0, 255), size=1.0):
    """Small solid pyramid at a camera (4x4 cam->world, OpenGL): apex at the camera centre, base 3 * size in front of it (-z): 5
    vertices, 6 triangles."""
    v = np.array([[0, 0, 0], [1, 1, 3], [-1, 1, 3], [-1, -1, 3], [1, -1, 3]], np.float64) * size
    v[:, 2] *= -1
    P = np.asarray(pose_gl, np.float64)
    verts = v @ P[:3, :3].T + P[:3, 3]
    faces = np.array([[0, 4, 1], [0, 1, 2], [0, 2, 3], [0, 3, 4], [4, 2, 1], [4, 3, 2]])
    return Mesh(verts, faces, _rgba(color, len(faces)))


FRUSTUM_VERTS = np.array([(0., 0., 0.), (0.375, -0.375, -1.0), (0.375, 0.375, -1.0), (-0.375, 0.375, -1.0), (-0.375, -0.375, -1.0)])
FRUSTUM_EDGES = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 3), (3, 4), (4, 1)]


def image_box(pose_gl, aspect_ratio, size, flip=True):
    """The image quad inside a frustum (ace_vis_util.get_image_box's geometry): (xyz float64 [2,3,3] world, uv float64 [2,3,2]).

    In the camera frame (OpenGL) the quad lies at z = -size, 0.75 * size high and 0.75 * aspect_ratio * size wide; with `flip` the
    width is negated (the reference mirrors the image left/right at the same time). UVs follow the acez_tex_triangle convention: u
    across the image's columns from the left, v down its rows from the top. The reference's uvs (1,0) (1,1) (0,1) (0,0) at the four
    corners index the image after its top/bottom flip (and the mirror with `flip`), counted from the bottom left: in the image as it
    is stored that is the same v, and u = 1 - u with the mirror. Either way the image's top left lands at the camera's upper left."""
    height = 0.75
    width = height * aspect_ratio * size
    height = height * size
    if flip:
        width = -width
    corners = np.array([[width / 2, height / 2, -size], [width / 2, -height / 2, -size], [-width / 2, -height / 2, -size],
                        [-width / 2, height / 2, -size]], np.float64)
    uv = np.array([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.0, 0.0]])
    if flip:
        uv[:, 0] = 1.0 - uv[:, 0]
    hom = np.asarray(pose_gl, np.float64) @ np.concatenate([corners, np.ones((4, 1))], 1).T
    world = (hom[:3] / hom[3]).T
    faces = np.array([[0, 1, 2], [2, 3, 0]])
    return world[faces], uv[faces]


def frustum_outline(pose_gl, color=(255, 255, 255), size=0.3, aspect_ratio=4 / 3):
    """Camera frustum drawn as its 8 edges, each a cuboid_from_line: 64 vertices, 96 triangles."""
    v = FRUSTUM_VERTS.copy()
    v[:, 0] *= aspect_ratio
    P = np.asarray(pose_gl, np.float64)
    w = size * v @ P[:3, :3].T + P[:3, 3]
    return Mesh.concatenate([cuboid_from_line(w[i], w[j], color) for i, j in FRUSTUM_EDGES])


def box_marker(pose_gl, color=(125, 125, 125), extent=0.015):
    """Axis-aligned (in the camera's frame) cube of side `extent` centred at the camera: 8 vertices, 12 triangles."""
    h = extent / 2
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)])
    P = np.asarray(pose_gl, np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = _quads_to_tris(quads)
    return Mesh(v @ P[:3, :3].T + P[:3, 3], faces, _rgba(color, len(faces)))


class CameraTrajectory:
    """Trajectory geometry: position markers, camera-path segments (a cuboid per step, skipped across jumps of more than 10 x the
    median step) and frustums placed at least frustum_skip metres apart (unless sparse=False); a frustum added with its image also
    gets the image quad (frustum_images: (xyz [2,3,3], uv [2,3,2], uint8 image [h,w,3]) per frustum, what Renderer takes as
    `textured`)."""

    def __init__(self, frustum_skip=0.0, frustum_scale=0.3):
        self.frustum_skip, self.frustum_scale = frustum_skip, frustum_scale
        self.trajectory, self.frustums, self.frustum_positions, self.frustum_images = [], [], [], []
        self.previous, self.distances = None, []
        self.color = (255, 255, 255)
        self.aspect_ratio = 4 / 3

    def grow_camera_path(self, pose_gl):
        pos = np.asarray(pose_gl, np.float64)[:3, 3]
        if self.previous is not None:
            dist = float(np.linalg.norm(pos - self.previous))
            self.distances.append(dist)
            self.distances.sort()
            skip = 10 * self.distances[len(self.distances) // 2]
            if 0.0001 < dist < skip:
                self.trajectory.append(cuboid_from_line(self.previous, pos, self.color))
        self.previous = pos

    def add_position_marker(self, pose_gl, color, extent=0.015, frustum_marker_=False):
        self.trajectory.append(frustum_marker(pose_gl, color, extent) if frustum_marker_ else box_marker(pose_gl, color, extent))

    def add_camera_frustum(self, pose_gl, sparse=True, color=None, image=None):
        """image: the camera's uint8 RGB frame [h,w,3] (numpy or a device tensor), drawn inside the frustum; its w / h becomes the
        aspect ratio of this frustum and of the ones after it (the reference's aspect_ratio_buffer)."""
        pos = np.asarray(pose_gl, np.float64)[:3, 3]
        near = min((np.linalg.norm(p - pos) for p in self.frustum_positions), default=self.frustum_skip + 1)
        if not sparse or near > self.frustum_skip:
            if image is not None:
                h, w = int(image.shape[0]), int(image.shape[1])
                self.aspect_ratio = w / h
                xyz, uv = image_box(pose_gl, self.aspect_ratio, self.frustum_scale, flip=True)
                self.frustum_images.append((xyz, uv, image))
            self.frustums.append(frustum_outline(pose_gl, self.color if color is None else color, self.frustum_scale, self.aspect_ratio))
            self.frustum_positions.append(pos)

    def clear_frustums(self):
        self.frustums.clear()
        self.frustum_images.clear()

    def mesh(self):
        return Mesh.concatenate(self.trajectory + self.frustums)


# --------------------------------------------------------------------------------------------------------- observing camera
def _orthonormalize(T):
    """Nearest rotation (SVD, determinant +1) of the upper-left 3x3; the fourth row is reset to 0 0 0 1."""
    U, _, Vt = np.linalg.svd(T[:3, :3])
    Z = np.eye(3)
    Z[2, 2] = np.sign(np.linalg.det(U @ Vt))
    out = np.eye(4)
    out[:3, :3] = U @ Z @ Vt
    out[:3, 3] = T[:3, 3]
    return out


class LazyCamera:
    """Smoothed, slightly delayed observing camera: each view is pushed back along its own +z by `backwards_offset` metres, the
    last `buffer_size` of them are averaged and re-orthonormalised."""

    def __init__(self, buffer_size=40, backwards_offset=4, camera_buffer=None):
        self.buffer = [] if camera_buffer is None else list(camera_buffer)
        self.buffer_size, self.backwards_offset = buffer_size, backwards_offset

    def update(self, view):
        cam = np.array(view, np.float64)
        cam[:3, 3] += cam[:3, :3] @ np.array([0, 0, 1.0]) * self.backwards_offset
        self.buffer.append(cam)
        if len(self.buffer) > self.buffer_size:
            self.buffer = self.buffer[1:]

    def current_view(self):
        return _orthonormalize(sum(self.buffer) / len(self.buffer))


def generate_pan(n_cams, poses_gl, angle_coverage, anchor=None, flipped_portrait=False):
    """Views panning around the mapping cameras (OpenGL cam->world): centred at their mean position, oriented like the middle camera
    (or the one nearest to `anchor`), radius half the mean of the two largest extents, sweeping `angle_coverage` degrees."""
    poses = [np.asarray(p, np.float64) for p in poses_gl if np.all(np.isfinite(p))]
    if anchor is None:
        center = poses[len(poses) // 2].copy()
    else:
        d = [np.linalg.norm(p[:3, 3] - np.asarray(anchor)[:3, 3]) for p in poses]
        center = poses[int(np.argmin(d))].copy()
    pos = np.stack([p[:3, 3] for p in poses], axis=-1)
    center[:3, 3] = pos.mean(axis=1)
    ext = sorted(pos.max(axis=1) - pos.min(axis=1), reverse=True)
    radius = 0.5 * 0.5 * (ext[0] + ext[1])
    start, inc = -90 - angle_coverage / 2, angle_coverage / n_cams
    cams = []
    for i in range(n_cams):
        P = np.eye(4)
        a = math.radians(start + inc * i)
        P[1 if flipped_portrait else 0, 3] = radius * math.cos(a)
        P[2, 3] = -radius * math.sin(a)
        if flipped_portrait:
            r = math.radians(angle_coverage / 2 - inc * i)
            P[1, 1], P[1, 2], P[2, 1], P[2, 2] = math.cos(r), -math.sin(r), math.sin(r), math.cos(r)
        else:
            r = math.radians(-angle_coverage / 2 + inc * i)
            P[0, 0], P[0, 2], P[2, 0], P[2, 2] = math.cos(r), math.sin(r), -math.sin(r), math.cos(r)
        cams.append(center @ P)
    return cams


def pan_camera(pan_cams, frame_idx):
    """Back and forth through the pan: forwards on even cycles, backwards on odd ones."""
    n = len(pan_cams)
    i = frame_idx % n
    return pan_cams[n - i - 1 if (frame_idx // n) % 2 == 1 else i]


class PointCloudBuffer:
    """The last `size` point-cloud updates (size <= 0: no cap). Chunks are numpy arrays or tensors (the Visualizer keeps its chunks on
    the device: xyz float32 [k,3], colours uint8 [k,3]); get() joins them in the same kind."""

    def __init__(self, size=5):
        self.size, self.xyz, self.clr, self.err = size, [], [], []

    def update(self, xyz, clr, err=None):
        self.xyz.append(xyz.reshape(-1, 3) if torch.is_tensor(xyz) else np.asarray(xyz, np.float32).reshape(-1, 3))
        self.clr.append(clr.reshape(-1, 3) if torch.is_tensor(clr) else np.asarray(clr).reshape(-1, 3))
        if err is not None:
            self.err.append(np.asarray(err))
        if 0 < self.size < len(self.xyz):
            self.xyz, self.clr = self.xyz[1:], self.clr[1:]
        if 0 < self.size < len(self.err):
            self.err = self.err[1:]

    def disable_cap(self):
        self.size = -1

    @staticmethod
    def _join(parts, empty):
        if not parts:
            return empty
        if len(parts) == 1:
            return parts[0]
        return torch.cat(parts) if torch.is_tensor(parts[0]) else np.concatenate(parts)

    def get(self):
        return (self._join(self.xyz, np.zeros((0, 3), np.float32)), self._join(self.clr, np.zeros((0, 3))),
                np.concatenate(self.err) if self.err else None)


# ------------------------------------------------------------------------------------------------------------------ renderer
def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


class Renderer:
    """ctypes wrapper of acez_render_frame / acez_render_frame_tex: device scratch and output frame are allocated once per frame
    size; the textures' mip chains share one device block that grows only when a larger set of images arrives."""

    def __init__(self, width=WIDTH, height=HEIGHT, flipped_portrait=False, device=None, znear=ZNEAR, zfar=ZFAR):
        if not torch.cuda.is_available():
            raise RuntimeError("Renderer needs a GPU: the rasteriser is HIP only (no CPU fallback)")
        self.lib = N.lib()
        self.flipped = bool(flipped_portrait)
        # a flipped portrait frame is rendered sideways (height x width swapped) and rotated back at the end
        self.rw, self.rh = (height, width) if self.flipped else (width, height)
        self.znear, self.zfar = float(znear), float(zfar)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.work = torch.empty(2 * self.rw * self.rh, dtype=torch.int64, device=self.device)
        self.frame = torch.empty(self.rw * self.rh * 3, dtype=torch.uint8, device=self.device)
        self.chains = torch.empty(0, dtype=torch.uint8, device=self.device)

    def _textures(self, textured):
        """(acez_tex_triangle array, acez_texture array, texture count): every distinct image uploaded (unless it is a device
        tensor already) and its mip chain built into self.chains, on the current stream."""
        dev = self.device
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        images, index, tris = [], {}, []
        for xyz, uv, img in textured:
            if id(img) not in index:
                index[id(img)] = len(images)
                images.append(img)
            xyz, uv = np.asarray(xyz, np.float32).reshape(-1, 3, 3), np.asarray(uv, np.float32).reshape(-1, 3, 2)
            if len(xyz) != len(uv):
                raise ValueError("one uv triple per textured triangle")
            tris += [(a, b, index[id(img)]) for a, b in zip(xyz, uv)]
        if len(tris) > N.RENDER_MAX_TEX_TRIANGLES or len(images) > N.RENDER_MAX_TEXTURES:
            raise ValueError(f"at most {N.RENDER_MAX_TEX_TRIANGLES} textured triangles over {N.RENDER_MAX_TEXTURES} images per frame")
        dimg, sizes, total = [], [], 0
        for img in images:
            t = torch.as_tensor(img)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise ValueError("a texture is a uint8 RGB image [h, w, 3]")
            dimg.append(t.to(dev).contiguous())
            levels, nbytes = C.c_int(), C.c_int64()
            N.check(self.lib.acez_render_texture_size(int(t.shape[1]), int(t.shape[0]), C.byref(levels), C.byref(nbytes)))
            sizes.append((total, int(t.shape[1]), int(t.shape[0])))
            total += nbytes.value
        if total > self.chains.numel():
            self.chains = torch.empty(total, dtype=torch.uint8, device=dev)
        table = (N.Texture * max(1, len(images)))()
        for k, (img, (off, w, h)) in enumerate(zip(dimg, sizes)):
            N.check(self.lib.acez_render_texture_build(_ptr(img), w, h, C.c_void_p(self.chains.data_ptr() + off), self.chains.numel() - off,
                                                       stream))
            table[k].offset, table[k].width, table[k].height = off, w, h
        arr = (N.TexTriangle * max(1, len(tris)))()
        for k, (a, b, ti) in enumerate(tris):
            for i in range(3):
                arr[k].xyz[i][:] = [float(x) for x in a[i]]
                arr[k].uv[i][:] = [float(x) for x in b[i]]
            arr[k].texture = ti
        self._keep = dimg                                    # the uploads stay alive until the next frame
        return arr, len(tris), table, len(images)

    def render_device(self, xyz, rgb, tri=None, tri_rgba=None, cam_to_world=None, textured=None):
        """Device tensors in, device frame out: uint8 [H][W][3] (the frame buffer is reused by the next call). textured: a list of
        (xyz [k,3,3] world, uv [k,3,2], uint8 RGB image [h,w,3], numpy or device) drawn with acez_render_frame_tex; None or empty:
        acez_render_frame."""
        dev = self.device
        xyz = torch.as_tensor(xyz, dtype=torch.float32).to(dev).reshape(-1, 3).contiguous()
        rgb = torch.as_tensor(rgb, dtype=torch.uint8).to(dev).reshape(-1, 3).contiguous()
        tri = torch.zeros((0, 3, 3), dtype=torch.float32, device=dev) if tri is None else torch.as_tensor(tri, dtype=torch.float32).to(dev).contiguous()
        tri_rgba = torch.zeros((0, 4), dtype=torch.uint8, device=dev) if tri_rgba is None else torch.as_tensor(tri_rgba, dtype=torch.uint8).to(dev).contiguous()
        if xyz.shape[0] != rgb.shape[0] or tri.shape[0] != tri_rgba.shape[0]:
            raise ValueError("one colour per point and per triangle")
        cam = (C.c_double * 16)(*np.asarray(cam_to_world, np.float64).reshape(16).tolist())
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if textured:
            arr, n_tex_tris, table, n_textures = self._textures(textured)
            N.check(self.lib.acez_render_frame_tex(_ptr(xyz), _ptr(rgb), int(xyz.shape[0]), _ptr(tri), _ptr(tri_rgba), int(tri.shape[0]), arr,
                                                   n_tex_tris, table, n_textures, _ptr(self.chains), self.chains.numel(), cam, self.znear,
                                                   self.zfar, self.rw, self.rh, int(self.flipped), _ptr(self.work), _ptr(self.frame), stream))
        else:
            N.check(self.lib.acez_render_frame(_ptr(xyz), _ptr(rgb), int(xyz.shape[0]), _ptr(tri), _ptr(tri_rgba), int(tri.shape[0]), cam,
                                               self.znear, self.zfar, self.rw, self.rh, int(self.flipped), _ptr(self.work), _ptr(self.frame),
                                               stream))
        shape = (self.rw, self.rh, 3) if self.flipped else (self.rh, self.rw, 3)
        return self.frame.view(*shape)

    def render(self, xyz, rgb, tri=None, tri_rgba=None, cam_to_world=None, textured=None):
        """The frame on the host: uint8 numpy [H][W][3] (the one device -> host copy of a frame)."""
        return self.render_device(xyz, rgb, tri, tri_rgba, cam_to_world, textured).cpu().numpy()


# ------------------------------------------------------------------------------------------------------ overlays and files
def draw_hist(image, values, colors, x, y, w, h, vmax, min_height=3):
    """Histogram bars as the reference places them: bar i starts at row x, column y + i * (h // bins), is h // bins wide and grows
    downwards by w * value / vmax rows (at least min_height)."""
    n = len(values)
    bar = int(h / n)
    H, W = image.shape[:2]
    for i in range(n):
        bw = max(min_height, int(w * (values[i] / vmax))) if vmax > 0 else min_height
        by = int(y + i * bar)
        r0, r1, c0, c1 = max(0, int(x)), min(H, int(x) + bw), max(0, by), min(W, by + bar)
        if r1 > r0 and c1 > c0:
            image[r0:r1, c0:c1, :3] = np.asarray(colors[i])[:3]
    return image


def write_captions(image, captions, color=(1, 1, 1)):
    """Text drawn with matplotlib (Agg) over the frame; returns the RGB frame."""
    import matplotlib
    matplotlib.use("Agg", force=False)
    from matplotlib.figure import Figure
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    h, w = image.shape[:2]
    fig = Figure(figsize=(w / 100, h / 100), dpi=100)
    canvas = FigureCanvasAgg(fig)
    fig.figimage(image, resize=False)
    for c in captions:
        fig.text(c["x"], c["y"], c["text"], fontsize=c["fs"], va="top", color=color)
    canvas.draw()
    return np.asarray(canvas.buffer_rgba())[:h, :w, :3].copy()


def save_frame(folder, frame_idx, image):
    from PIL import Image
    path = os.path.join(str(folder), f"frame_{frame_idx:05d}.png")
    Image.fromarray(np.ascontiguousarray(image, np.uint8)).save(path)
    return path


# ---------------------------------------------------------------------------------------------------------- the visualiser
class Visualizer:
    """The three phases of the reconstruction video: mapping (render_mapping_frame / finalize_mapping), registration
    (setup_reloc / render_reloc_frame / save_reloc_state) and the final sweep (render_final_sweep)."""

    def __init__(self, target_path, flipped_portrait=False, map_depth_filter=10, mapping_error_threshold=10, reloc_conf_threshold=5000,
                 confidence_threshold=CONFIDENCE_THRESHOLD, state_file_name="mapping_state.pkl", marker_size=0.03, camera_z_offset=4,
                 renderer=None, every=300, existing_state=None, frame_rgb=None):
        """every: a mapping frame every `every` training steps (--iterations_output); existing_state: the state file (in target_path)
        a mapping run resumes from (--use_existing_vis_buffer); frame_rgb: the frames' uint8 RGB images ([n,H,W,3] or a list), colours
        of the final map's points (None: grey)."""
        self.every, self.existing_state, self.frame_rgb = int(every), existing_state, frame_rgb
        self.target_path = str(target_path)
        os.makedirs(self.target_path, exist_ok=True)
        self.state_file = os.path.join(self.target_path, state_file_name)
        self.flipped = bool(flipped_portrait)
        self.map_depth_filter = map_depth_filter
        self.mapping_error_threshold = mapping_error_threshold
        self.reloc_conf_threshold = reloc_conf_threshold
        self.confidence_threshold = confidence_threshold
        self.marker_size = marker_size
        self.camera_z_offset = camera_z_offset
        self.renderer = renderer if renderer is not None else Renderer(flipped_portrait=self.flipped)
        self.rw, self.rh = self.renderer.rw, self.renderer.rh
        ref = min(self.rw, self.rh)
        self.hist_bins = 40
        self.hist_x, self.hist_y, self.hist_h = int(0.05 * ref), int(1.35 * ref), int(0.4 * ref)
        self.hist_w_reloc, self.hist_w_mapping = int(0.6 * ref), int(0.2 * ref)
        self.mapping_cmap = retro_colors()
        self.pose_cmap = colormap("plasma", 0, 1, 256)
        self.reloc_cmap = reloc_color_map(confidence_threshold, reloc_conf_threshold)
        self.sweep_cmap = colormap("cool", 0, 1, 10)
        self.frame_idx = 0
        self.mapping_iteration, self.mapping_done_idx = 0, -1
        self.pan_cams, self.camera, self.trajectory, self.cloud = None, None, None, None
        self.reloc_conf, self.reloc_count, self.reloc_counter, self.reloc_success = [], 0, 0, 0
        self.reloc_prev = None

    # ---- rendering
    def _to_device(self, xyz, clr):
        """A point-cloud chunk as device tensors (float32 xyz, uint8 colours): uploaded once, then drawn from the device every frame."""
        dev = self.renderer.device
        xyz = torch.as_tensor(np.ascontiguousarray(xyz, np.float32)).reshape(-1, 3).to(dev)
        clr = torch.as_tensor(np.clip(np.asarray(clr, np.float64), 0, 255).astype(np.uint8)).reshape(-1, 3).to(dev)
        return xyz, clr

    def _render(self):
        xyz, clr, _ = self.cloud.get()
        tri, rgba = self.trajectory.mesh().triangles()
        return self.renderer.render(xyz, clr, tri, rgba, self.camera.current_view(), self.trajectory.frustum_images)

    def _save(self, image):
        path = save_frame(self.target_path, self.frame_idx, image)
        _logger.info(f"Rendered and saved frame: {path}")

    def _captions(self, image, title, line, legend):
        h = image.shape[0]
        return write_captions(image, [{"x": 0.15, "y": 0.13, "fs": 0.04 * h, "text": title},
                                      {"x": 0.15, "y": 0.063, "fs": 0.02 * h, "text": line},
                                      {"x": 0.76, "y": 0.975, "fs": 0.015 * h, "text": legend}])

    # ---- mapping
    def setup_mapping(self, poses_c2w_cv, frame_count=MAPPING_FRAME_COUNT, existing_state=None):
        c2w = np.asarray(poses_c2w_cv, np.float64).reshape(-1, 4, 4)
        self.poses_w2c_orig = np.linalg.inv(c2w)[:, :3]
        poses = [cv_to_gl(p) for p in c2w]
        poses = [p for p in poses if np.all(np.isfinite(p))]
        self.mapping_poses = poses
        self.pan_cams = generate_pan(frame_count + FRAMECOUNT_TRANSITION, poses, PAN_ANGLE_COVERAGE, flipped_portrait=self.flipped)
        self.trajectory = CameraTrajectory(frustum_skip=0.5, frustum_scale=0.3)
        for p in poses:
            self.trajectory.add_position_marker(p, (125, 125, 125))
        self.frame_idx = 0
        self.camera = LazyCamera(backwards_offset=self.camera_z_offset)
        self.cloud = PointCloudBuffer()
        if existing_state is not None:
            with open(os.path.join(self.target_path, str(existing_state)), "rb") as f:
                st = pickle.load(f)
            self.frame_idx = st["frame_idx"]
            self.camera = LazyCamera(backwards_offset=self.camera_z_offset, camera_buffer=st["camera_buffer"])
            anchor = st["pan_cameras"][len(st["pan_cameras"]) // 2]
            self.pan_cams = generate_pan(frame_count + FRAMECOUNT_TRANSITION, poses, PAN_ANGLE_COVERAGE, anchor=anchor,
                                         flipped_portrait=self.flipped)

    def render_mapping_frame_from_trainer(self, tr, rows, iteration):
        """render_mapping_frame for the batch a HeadTrainer has just stepped on: its predicted scene coordinates (the step's own output,
        read once: the frame's only synchronisation) and their reprojection errors under the current poses."""
        xyz = tr.last_scene_coords(int(rows.numel()))
        poses = tr.current_poses()
        self.render_mapping_frame(xyz, trainer_batch_errors(tr, rows, xyz, poses), poses, self.poses_w2c_orig, iteration)

    def _camera_markers(self, poses_w2c, poses_w2c_orig):
        for p, q in zip(poses_w2c, poses_w2c_orig):
            a, b = np.eye(4), np.eye(4)
            a[:3], b[:3] = p, q
            a, b = np.linalg.inv(a), np.linalg.inv(b)
            idx = int(min(np.linalg.norm(a[:3, 3] - b[:3, 3]), 1.0) * 255)
            self.trajectory.add_position_marker(cv_to_gl(a), self.pose_cmap[idx] * 255, self.marker_size, frustum_marker_=True)

    def _mapping_frame(self):
        self.camera.update(pan_camera(self.pan_cams, self.frame_idx))
        img = self._render()
        _, _, errs = self.cloud.get()
        idx = [int(i / self.hist_bins * 255) for i in range(self.hist_bins)]
        if errs is not None and len(errs):
            hv, _ = np.histogram(errs, bins=self.hist_bins, range=(0, 1))
            draw_hist(img, hv, [self.mapping_cmap[i] * 255 for i in idx], self.hist_x, self.hist_y, self.hist_w_mapping, self.hist_h,
                      hv.max())
        draw_hist(img, np.zeros(self.hist_bins), [self.pose_cmap[i] * 255 for i in idx], self.hist_x, 0.1 * min(self.rw, self.rh),
                  self.hist_w_mapping, self.hist_h, 1, min_height=10)
        it = self.mapping_done_idx if self.mapping_done_idx > 0 else self.mapping_iteration
        img = self._captions(img, "Neural Mapping", f"Iteration: {it}",
                             f">{self.mapping_error_threshold}px       Reprojection Error       0px")
        self._save(img)
        self.frame_idx += 1

    def render_mapping_frame(self, scene_coords_cv, errors, poses_w2c, poses_w2c_orig, iteration):
        """One mapping frame: the batch's scene coordinates (OpenCV) coloured by reprojection error, the current cameras coloured by how
        far pose refinement moved them."""
        self.mapping_iteration = iteration
        xyz = np.array(scene_coords_cv, np.float32).reshape(-1, 3)
        xyz[:, 1:] *= -1
        clr, norm = errors_to_colors(errors, self.mapping_error_threshold, self.mapping_cmap)
        self.cloud.update(*self._to_device(xyz, clr), norm)
        keep = len(self.trajectory.trajectory)
        self._camera_markers(poses_w2c, poses_w2c_orig)
        self._mapping_frame()
        self.trajectory.trajectory = self.trajectory.trajectory[:keep]

    def finalize_mapping(self, map_xyz_gl, map_clr, poses_w2c, poses_w2c_orig):
        """The transition frames that grow the full map (OpenGL points, colours 0..255), then the `_mapping.pkl` state."""
        self._camera_markers(poses_w2c, poses_w2c_orig)
        map_xyz_gl, map_clr = np.asarray(map_xyz_gl, np.float32).reshape(-1, 3), np.asarray(map_clr).reshape(-1, 3)
        chunk = map_xyz_gl.shape[0] // FRAMECOUNT_TRANSITION
        self.mapping_done_idx = self.mapping_iteration
        dxyz, dclr = self._to_device(map_xyz_gl, map_clr)               # the whole map crosses to the device once
        for t in range(FRAMECOUNT_TRANSITION):
            self.cloud.update(dxyz[t * chunk:(t + 1) * chunk], dclr[t * chunk:(t + 1) * chunk])
            if t == self.cloud.size:
                self.cloud.disable_cap()
            self._mapping_frame()
        state = {"map_xyz": map_xyz_gl, "map_clr": map_clr, "frame_idx": self.frame_idx, "camera_buffer": self.camera.buffer,
                 "pan_cameras": self.pan_cams}
        with open(self.state_file, "wb") as f:
            pickle.dump(state, f)
        _logger.info(f"Stored rendering buffer to {self.state_file}.")

    # ---- registration
    def setup_reloc(self, frame_count):
        with open(self.state_file, "rb") as f:
            st = pickle.load(f)
        self.frame_idx = st["frame_idx"]
        self.camera = LazyCamera(backwards_offset=self.camera_z_offset, camera_buffer=st["camera_buffer"])
        self.pan_cams = st["pan_cameras"]
        self.cloud = PointCloudBuffer()
        self.cloud.update(*self._to_device(st["map_xyz"], st["map_clr"]))
        self.trajectory = CameraTrajectory(frustum_skip=0, frustum_scale=0.3)
        self.reloc_conf, self.reloc_count, self.reloc_counter, self.reloc_success = [], frame_count, 0, 0

    def render_reloc_frame(self, est_pose_c2w_cv, confidence, image=None):
        """One registration frame: the query's frustum coloured by confidence, with the query's uint8 RGB frame `image` [h,w,3] inside
        it (None: the outline alone); earlier registered queries stay as markers. At most RELOC_DURATION frames per run: with more
        queries every k-th one is rendered (k = count // RELOC_DURATION)."""
        pose = cv_to_gl(est_pose_c2w_cv)
        self.reloc_conf.append(confidence)
        color = self.reloc_cmap[min(int(confidence / self.reloc_conf_threshold * 255), 255)] * 255
        self.trajectory.clear_frustums()
        self.trajectory.add_camera_frustum(pose, sparse=False, color=color, image=image)
        if confidence > self.confidence_threshold:
            self.reloc_success += 1
            if self.reloc_prev is not None:
                self.trajectory.add_position_marker(self.reloc_prev[0], self.reloc_prev[1], self.marker_size, frustum_marker_=True)
            self.reloc_prev = (pose, color)
        if self.reloc_counter % max(1, self.reloc_count // RELOC_DURATION) == 0:
            self.camera.update(pan_camera(self.pan_cams, self.frame_idx))
            img = self._render()
            hv, _ = np.histogram(np.clip(self.reloc_conf, 0, self.reloc_conf_threshold), bins=self.hist_bins,
                                 range=(0, self.reloc_conf_threshold))
            draw_hist(img, hv, [self.reloc_cmap[int(i / self.hist_bins * 255)] * 255 for i in range(self.hist_bins)], self.hist_x,
                      self.hist_y, self.hist_w_reloc, self.hist_h, self.reloc_count)
            n = self.reloc_counter + 1
            img = self._captions(img, "Registering Mapping Frames",
                                 f"Successfully Registered: {self.reloc_success}/{n} frames ({self.reloc_success / n * 100:.1f}%)",
                                 f"0   {int(self.confidence_threshold)}            Confidence             {self.reloc_conf_threshold // 1000}k")
            self._save(img)
            self.frame_idx += 1
        self.reloc_counter += 1

    def save_reloc_state(self, out_file):
        with open(self.state_file, "rb") as f:
            st = pickle.load(f)
        st["frame_idx"], st["camera_buffer"] = self.frame_idx, self.camera.buffer
        with open(out_file, "wb") as f:
            pickle.dump(st, f)
        _logger.info(f"Stored rendering buffer to {out_file}.")

    # ---- final sweep
    def render_final_sweep(self, poses_c2w_cv, pose_iterations, total_poses, frame_count=SWEEP_FRAME_COUNT):
        """A 90-degree pan of frame_count frames over the final map, every registered camera coloured by the iteration that first
        registered it."""
        with open(self.state_file, "rb") as f:
            st = pickle.load(f)
        self.frame_idx = st["frame_idx"]
        self.camera = LazyCamera(backwards_offset=self.camera_z_offset, camera_buffer=st["camera_buffer"])
        anchor = st["pan_cameras"][len(st["pan_cameras"]) // 2]
        self.cloud = PointCloudBuffer()
        self.cloud.update(*self._to_device(st["map_xyz"], st["map_clr"]))
        self.trajectory = CameraTrajectory(frustum_skip=0, frustum_scale=0.3)
        poses = [cv_to_gl(p) for p in poses_c2w_cv]
        its = []
        for p, it in zip(poses, pose_iterations):
            c = self.sweep_cmap[min(it, SWEEP_ITERATIONS_THRESHOLD - 1)] * 255
            self.trajectory.add_position_marker(p, c, self.marker_size, frustum_marker_=True)
            its.append(min(it, SWEEP_ITERATIONS_THRESHOLD))
        for cam in generate_pan(frame_count, poses, 90, anchor=anchor, flipped_portrait=self.flipped):
            self.camera.update(cam)
            img = self._render()
            hv, _ = np.histogram(its, bins=10, range=(0, SWEEP_ITERATIONS_THRESHOLD))
            draw_hist(img, hv, [self.sweep_cmap[i] * 255 for i in range(10)], self.hist_x, self.hist_y, self.hist_w_reloc, self.hist_h,
                      max(len(its), 1))
            img = self._captions(img, "Mapping Done",
                                 f"Successfully Registered: {len(poses)}/{total_poses} frames ({len(poses) / max(total_poses, 1) * 100:.1f}%)",
                                 f"0          Registered in Iteration        >{SWEEP_ITERATIONS_THRESHOLD}")
            self._save(img)
            self.frame_idx += 1


def trainer_batch_errors(tr, rows, xyz, poses_w2c):
    """Reprojection error in px (Euclidean) of scene coordinates xyz [k,3] predicted for the training-buffer rows `rows` (device
    int64) of a HeadTrainer, under the poses [n_images,3,4] world -> camera and each row's view augmentation and intrinsics
    (ace_trainer.py:530-552). Only the k rows of the device buffer are read."""
    b = tr._buf
    v = b["view_idx"][rows].long()
    img = b["view_image"][v].long().cpu().numpy()
    aug = b["view_aug_inv"][v].double().cpu().numpy().reshape(-1, 3, 4)
    K = b["view_K"][v].double().cpu().numpy().reshape(-1, 3, 3)
    px = b["target_px"][rows].double().cpu().numpy().reshape(-1, 2)
    P = np.tile(np.eye(4), (len(poses_w2c), 1, 1))
    P[:, :3] = poses_w2c
    M = aug @ P[img]
    Xc = np.einsum("kij,kj->ki", M, np.concatenate([np.asarray(xyz, np.float64).reshape(-1, 3), np.ones((len(img), 1))], 1))
    pp = np.einsum("kij,kj->ki", K, Xc)
    z = np.maximum(pp[:, 2], 0.1)
    return np.linalg.norm(pp[:, :2] / z[:, None] - px, axis=1)


def rendering_target_path(base, map_file):
    """<base>/<map file stem>, created."""
    p = os.path.join(str(base), os.path.splitext(os.path.basename(str(map_file)))[0])
    os.makedirs(p, exist_ok=True)
    return p


# ---------------------------------------------------------------------------------------------------------- final sweep
def pose_iteration_table(last_pose_file, max_iteration, confidence_threshold=CONFIDENCE_THRESHOLD):
    """{image file: first iteration that registered it above the threshold} from poses_iteration<k>.txt next to the last pose file
    (iteration 0: the seed's poses_iteration0_seed<k>.txt). Images never registered keep max_iteration."""
    from pathlib import Path
    last = Path(last_pose_file)
    table = {e.file: max_iteration for e in read_pose_file(last, strict=False)}
    for it in reversed(range(max_iteration)):
        stem = last.stem.split("_")
        stem[-1] = f"iteration{it}"
        name = "_".join(stem)
        if it == 0:
            found = sorted(last.parent.glob(f"{name}_seed[0-9].txt"))
            if not found:
                continue
            path = found[0]
        else:
            path = last.parent / f"{name}.txt"
            if not path.exists():
                continue
        for e in read_pose_file(path, strict=False):
            if e.confidence > confidence_threshold:
                table[e.file] = it
    return table


def render_final_sweep_main(argv=None):
    """render_final_sweep.py: render_folder [--render_camera_z_offset] [--render_marker_size]."""
    import argparse
    from pathlib import Path
    p = argparse.ArgumentParser(description="Renders additional frames at the end of a reconstruction visualisation.",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("render_folder", type=Path)
    p.add_argument("--render_camera_z_offset", type=int, default=4, help="zoom out of the scene by moving render camera backwards, in meters")
    p.add_argument("--render_marker_size", type=float, default=0.03)
    opt = p.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    state = None
    for it in reversed(range(100)):
        cand = opt.render_folder / f"iteration{it}_register.pkl"
        if cand.is_file():
            state = cand
            break
    if state is None:
        _logger.error(f"Could not find a state file in {opt.render_folder}")
        return 1
    pose_file = opt.render_folder.parent / f"poses_iteration{it}.txt"
    if not pose_file.is_file():
        _logger.error(f"Could not find a pose file: {pose_file} does not exist.")
        return 1
    table = pose_iteration_table(pose_file, it, CONFIDENCE_THRESHOLD)
    files, c2w, _ = read_ace_pose_file(pose_file, CONFIDENCE_THRESHOLD)
    vis = Visualizer(opt.render_folder, state_file_name=state.name, marker_size=opt.render_marker_size,
                     camera_z_offset=opt.render_camera_z_offset)
    vis.render_final_sweep(list(c2w), [table[f] for f in files], len(table))
    return 0


# -------------------------------------------------------------------------------------------------------------- export_cameras
def camera_mesh(poses_c2w_cv, confidences, frustum_scale=0.1, frustum_markers=False, draw_non_confident=True,
                confidence_threshold=CONFIDENCE_THRESHOLD, confidence_max=5000):
    """Mesh of the cameras of a pose file (OpenGL), coloured by confidence with the registration map (cool below the threshold,
    summer above; a single pose, the seed, is grey): frustum outlines, or solid frustum markers of size frustum_scale."""
    cmap = reloc_color_map(confidence_threshold, confidence_max)
    traj = CameraTrajectory(frustum_skip=0, frustum_scale=frustum_scale)
    for p, c in zip(poses_c2w_cv, confidences):
        c = min(float(c), confidence_max)
        if not (c > confidence_threshold or draw_non_confident):
            continue
        color = (100, 100, 100) if len(poses_c2w_cv) == 1 else cmap[min(int(c / confidence_max * 255), 255)] * 255
        pose = cv_to_gl(p)
        if frustum_markers:
            traj.add_position_marker(pose, color, frustum_scale, frustum_marker_=True)
        else:
            traj.add_camera_frustum(pose, color=color)
    return traj.mesh()


def export_cameras_main(argv=None):
    """export_cameras.py: pose_file output_file [--frustum_scale] [--frustum_markers] [--draw_non_confident] [--confidence_threshold]."""
    import argparse
    from pathlib import Path
    from .formats import _strtobool
    p = argparse.ArgumentParser(description="Export the cameras of an ACE pose file as a mesh (PLY).",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("pose_file", type=Path, help="ACE pose file (file qw qx qy qz tx ty tz focal confidence)")
    p.add_argument("output_file", type=Path, help="output mesh (.ply)")
    p.add_argument("--frustum_scale", type=float, default=0.1, help="size of the camera frustums")
    p.add_argument("--frustum_markers", type=_strtobool, default=False, help="solid frustum markers instead of outlines")
    p.add_argument("--draw_non_confident", type=_strtobool, default=True, help="also draw cameras below the confidence threshold")
    p.add_argument("--confidence_threshold", type=int, default=CONFIDENCE_THRESHOLD, help="confidence threshold of the colour coding")
    opt = p.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    entries = read_pose_file(opt.pose_file, strict=False)        # a line that does not have ten fields is skipped
    poses, conf = [np.linalg.inv(e.w2c) for e in entries], [e.confidence for e in entries]
    mesh = camera_mesh(poses, conf, opt.frustum_scale, opt.frustum_markers, opt.draw_non_confident, opt.confidence_threshold)
    # a vertex takes its face's colour: every face gets three vertices of its own
    write_ply(opt.output_file, mesh.verts[mesh.faces], np.repeat(mesh.rgba[:, :3], 3, axis=0),
              np.arange(3 * len(mesh.faces), dtype=np.int32), alpha=False)
    _logger.info(f"Done. {len(mesh.faces)} triangles of {len(poses)} cameras stored as: {opt.output_file}")
    return 0
