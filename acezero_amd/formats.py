"""The files that carry results from one command line to the next, each read and written in one place: the ACE pose file
(`file qw qx qy qz tx ty tz focal confidence`, world->camera), binary little-endian PLY (point clouds, fused meshes, camera
meshes) and the 16-bit depth PNG that estimate_depth.py writes and fuse_depth.py reads. Host code only."""
import os
from collections import namedtuple

import numpy as np


# ----------------------------------------------------------------------------------------------------------- pose files
# one line of a pose file: w2c is the world->camera 4x4 float64, confidence the float of the field confidence_text
PoseEntry = namedtuple("PoseEntry", ["file", "w2c", "focal", "confidence", "confidence_text"])


def quat_wxyz_to_matrix(q_wxyz):
    """Rotation matrix of a pose file's (qw, qx, qy, qz) (dataset_io.py:130-134, eval_poses.py:77)."""
    from scipy.spatial.transform import Rotation
    q = list(q_wxyz)
    return Rotation.from_quat(q[1:] + [q[0]]).as_matrix()


def pose_matrix(q_wxyz, t):
    """World->camera 4x4 float64 of a pose file's quaternion and translation."""
    T = np.eye(4)
    T[:3, :3] = quat_wxyz_to_matrix(q_wxyz)
    T[:3, 3] = t
    return T


def write_pose_line(f, rgb_file, pose_w2c, confidence, focal_length):
    """dataset_io.py:159-186: `file qw qx qy qz tx ty tz focal confidence`, world->cam."""
    from scipy.spatial.transform import Rotation
    q = Rotation.from_matrix(np.asarray(pose_w2c, np.float64)[:3, :3]).as_quat()
    t = np.asarray(pose_w2c)[:3, 3]
    f.write(f"{rgb_file} {q[3]} {q[0]} {q[1]} {q[2]} {t[0]} {t[1]} {t[2]} {focal_length} {confidence}\n")


def parse_pose_line(line):
    tok = line.split()
    assert len(tok) == 10, f"Expected 10 tokens per line in pose file, got {len(tok)}"
    return PoseEntry(tok[0], pose_matrix([float(t) for t in tok[1:5]], [float(t) for t in tok[5:8]]), float(tok[8]), float(tok[9]), tok[9])


def read_pose_file(path, strict=True):
    """The PoseEntry of every line, in file order. A line that does not have ten fields (a blank one included) is an AssertionError,
    or with strict=False is skipped."""
    with open(path) as f:
        lines = f.read().splitlines()
    return [parse_pose_line(line) for line in lines if strict or len(line.split()) == 10]


def read_ace_pose_file(path, confidence_threshold):
    """dataset_io.load_dataset_ace (:96-156): (files, cam->world 4x4 float64 [k,4,4], focal lengths) of the entries whose confidence
    is not below the threshold."""
    kept = [e for e in read_pose_file(path) if not e.confidence < confidence_threshold]
    return [e.file for e in kept], np.stack([np.linalg.inv(e.w2c) for e in kept]) if kept else np.zeros((0, 4, 4)), [e.focal for e in kept]


def match_poses(names, files):
    """For every file the row of the pose file (names: its file column) or None: the full name first, then the basename; of rows
    that share a name the last one."""
    by_name = {n: k for k, n in enumerate(names)}
    by_base = {os.path.basename(n): k for k, n in enumerate(names)}
    return [by_name.get(f, by_base.get(os.path.basename(f))) for f in files]


# ------------------------------------------------------------------------------------------------------------------ PLY
# the vertex element: (PLY type, property, numpy type); write_ply leaves alpha out on request, read_ply_vertices expects all of it
PLY_VERTEX = (("float", "x", "<f4"), ("float", "y", "<f4"), ("float", "z", "<f4"),
              ("uchar", "red", "u1"), ("uchar", "green", "u1"), ("uchar", "blue", "u1"), ("uchar", "alpha", "u1"))
_PLY_MAGIC = ["ply", "format binary_little_endian 1.0"]
_PLY_END = b"end_header\n"


def write_ply(path, xyz, rgb, faces=None, alpha=True):
    """Binary little-endian PLY: float vertices [m,3] with uchar colours [m,3] (and alpha 255), then, if given, int32 triangles [k,3]
    as (uchar count, int vertex indices) lists. Host arrays."""
    xyz, rgb = np.asarray(xyz).astype(np.float32).reshape(-1, 3), np.asarray(rgb).astype(np.uint8).reshape(-1, 3)
    props = PLY_VERTEX if alpha else PLY_VERTEX[:-1]
    vrec = np.zeros(len(xyz), dtype=[(name, dt) for _, name, dt in props])
    for (_, name, _), column in zip(props, [*xyz.T, *rgb.T, 255]):
        vrec[name] = column
    head = _PLY_MAGIC + [f"element vertex {len(xyz)}"] + [f"property {t} {name}" for t, name, _ in props]
    body = vrec.tobytes()
    if faces is not None:
        tri = np.asarray(faces).reshape(-1, 3)
        frec = np.zeros(len(tri), dtype=[("n", "u1"), ("v", "<i4", (3,))])
        frec["n"], frec["v"] = 3, tri
        head += [f"element face {len(tri)}", "property list uchar int vertex_indices"]
        body += frec.tobytes()
    with open(str(path), "wb") as fh:
        fh.write("\n".join(head).encode("ascii") + b"\n" + _PLY_END + body)


def read_ply_vertices(path):
    """float32 [m,3] of a binary little-endian .ply whose vertex element is PLY_VERTEX (what write_ply writes with alpha); further
    elements (a mesh's faces) are ignored."""
    blob = open(str(path), "rb").read()
    head, sep, body = blob.partition(_PLY_END)
    lines = head.decode("ascii", "replace").splitlines()
    if not sep or lines[:2] != _PLY_MAGIC:
        raise SystemExit(f"{path}: not a binary little-endian .ply")
    count, props, element = 0, [], None
    for line in lines:
        tok = line.split()
        if tok[:1] == ["element"]:
            element = tok[1]
            if element == "vertex":
                count = int(tok[2])
        elif tok[:1] == ["property"] and element == "vertex":
            props.append(tuple(tok[1:]))
    if props != [(t, name) for t, name, _ in PLY_VERTEX]:
        raise SystemExit(f"{path}: expected the vertex layout export_point_cloud.py writes (float x y z, uchar red green blue alpha)")
    vertex = np.dtype([(name, dt) for _, name, dt in PLY_VERTEX])
    if len(body) < vertex.itemsize * count:
        raise SystemExit(f"{path}: truncated")
    rec = np.frombuffer(body[:vertex.itemsize * count], dtype=vertex)
    return np.stack([rec["x"], rec["y"], rec["z"]], axis=1)


# PLY scalar type -> numpy type without byte order (both spellings of the format's type names)
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_points(path):
    """float32 [m,3]: the x, y, z of the vertex element of a binary little-endian or ASCII .ply, whatever else the element carries
    (normals, colours with or without alpha, doubles): ground-truth scans and other tools' clouds. The vertex element must come
    first (it does in every file met so far) and have scalar properties only; further elements (faces) are ignored."""
    blob = open(str(path), "rb").read()
    head, sep, body = blob.partition(_PLY_END)
    lines = [line.strip() for line in head.decode("ascii", "replace").splitlines()]
    if not sep or lines[:1] != ["ply"]:
        raise SystemExit(f"{path}: not a .ply file")
    fmt = [line.split()[1] for line in lines if line.split()[:1] == ["format"]]
    if fmt not in (["binary_little_endian"], ["ascii"]):
        raise SystemExit(f"{path}: only binary little-endian and ASCII .ply files are read")
    count, props, elements = 0, [], []
    for line in lines:
        tok = line.split()
        if tok[:1] == ["element"] and len(tok) == 3:
            elements.append(tok[1])
            if tok[1] == "vertex":
                count = int(tok[2])
        elif tok[:1] == ["property"] and elements[-1:] == ["vertex"]:
            if len(tok) != 3 or tok[1] not in _PLY_TYPES:
                raise SystemExit(f"{path}: vertex property '{line}' is not a scalar of a known type")
            props.append((tok[2], _PLY_TYPES[tok[1]]))
    if elements[:1] != ["vertex"]:
        raise SystemExit(f"{path}: the first element is not 'vertex'")
    names = [name for name, _ in props]
    if not all(axis in names for axis in "xyz") or len(set(names)) != len(names):
        raise SystemExit(f"{path}: the vertex element has no x, y, z (properties: {' '.join(names)})")
    if fmt == ["ascii"]:
        tok = body.split()
        if len(tok) < count * len(props):
            raise SystemExit(f"{path}: truncated")
        try:
            table = np.array(tok[:count * len(props)], dtype=np.float64).reshape(count, len(props))
        except ValueError:
            raise SystemExit(f"{path}: a vertex line holds something that is not a number")
        return np.ascontiguousarray(np.stack([table[:, names.index(axis)] for axis in "xyz"], axis=1).astype(np.float32))
    vertex = np.dtype([(name, "<" + dt) for name, dt in props])
    if len(body) < vertex.itemsize * count:
        raise SystemExit(f"{path}: truncated")
    rec = np.frombuffer(body[:vertex.itemsize * count], dtype=vertex)
    return np.ascontiguousarray(np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ depth PNG
def write_depth_png(path, depth_u16):
    """A uint16 [h,w] depth map as a 16-bit single-channel PNG."""
    from PIL import Image
    Image.fromarray(depth_u16).save(path)


def read_depth_png(path):
    """uint16 [h,w] of a single-channel depth image."""
    from PIL import Image
    d = np.asarray(Image.open(path))
    if d.ndim != 2:
        raise SystemExit(f"{path}: a depth map must have one channel")
    return np.ascontiguousarray(np.clip(d, 0, 65535).astype(np.uint16))
