"""The files that carry results from one command line to the next, each read and written in one place: the ACE pose file
(`file qw qx qy qz tx ty tz focal confidence`, world->camera), binary little-endian PLY (point clouds, fused meshes, camera
meshes; read_ply_mesh also reads other tools' meshes), the Tanks and Temples crop file (JSON) and the 16-bit depth PNG that
estimate_depth.py writes and fuse_depth.py reads. Host code only."""
import argparse
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


def read_posed_images(pose_file, files, confidence_threshold):
    """The posed images of fuse_depth.py and estimate_depth.py: (cam->world [k,4,4], focals [k], for every file its row of the two or
    None) from the pose file's entries that are not below the threshold. ValueError if no entry is left or no file has one."""
    names, c2w, focals = read_ace_pose_file(pose_file, confidence_threshold)
    if not names:
        raise ValueError("no pose above the confidence threshold")
    rows = match_poses(names, files)
    if all(k is None for k in rows):
        raise ValueError("no image of the glob has a pose above the confidence threshold in the pose file")
    return c2w, focals, rows


def write_poses_like(path, pose_file, confidence_threshold, rows, cam_to_world):
    """A pose file of the entries `rows` of pose_file (indices into what read_ace_pose_file keeps at this threshold, as
    read_posed_images returns them), in the order given, with their poses replaced by cam_to_world [k,4,4]; file names, focal lengths
    and confidences are the input's."""
    kept = [e for e in read_pose_file(pose_file) if not e.confidence < confidence_threshold]
    with open(path, "w") as f:
        for k, T in zip(rows, cam_to_world):
            write_pose_line(f, kept[k].file, np.linalg.inv(np.asarray(T, np.float64)), kept[k].confidence_text, kept[k].focal)


def focal_at_height(focal, h, image_h):
    """A pose file's focal is in pixels of the original image (image_h rows); a depth map or working image of h rows is that image at
    another scale."""
    return focal * h / image_h


# -------------------------------------------------------------------------------------------------------- flag values
def _strtobool(x):
    v = str(x).lower()
    if v in ("y", "yes", "t", "true", "on", "1"):
        return True
    if v in ("n", "no", "f", "false", "off", "0"):
        return False
    raise argparse.ArgumentTypeError(f"invalid truth value {x!r}")


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


def _ply_header(path, blob):
    """(format, [(element, count, [property tokens after 'property'])], body) of a binary little-endian or ASCII .ply."""
    head, sep, body = blob.partition(_PLY_END)
    lines = [line.strip() for line in head.decode("ascii", "replace").splitlines()]
    if not sep or lines[:1] != ["ply"]:
        raise SystemExit(f"{path}: not a .ply file")
    fmt = [line.split()[1] for line in lines if line.split()[:1] == ["format"] and len(line.split()) > 1]
    if fmt not in (["binary_little_endian"], ["ascii"]):
        raise SystemExit(f"{path}: only binary little-endian and ASCII .ply files are read")
    elements = []
    for line in lines:
        tok = line.split()
        if tok[:1] == ["element"] and len(tok) == 3:
            try:
                elements.append((tok[1], int(tok[2]), []))
            except ValueError:
                raise SystemExit(f"{path}: '{line}' does not give a count")
        elif tok[:1] == ["property"] and elements:
            elements[-1][2].append(tok[1:])
    return fmt[0], elements, body


def _fan(rows, width):
    """int64 [len(rows) * (width - 2), 3]: every polygon (row of `width` indices) split as the fan (0, i, i + 1)."""
    tri = np.stack([np.stack([rows[:, 0], rows[:, i], rows[:, i + 1]], 1) for i in range(1, width - 1)], 1)
    return tri.reshape(-1, 3)


def read_ply_mesh(path):
    """(vertices float32 [m,3], colours uint8 [m,3] or None, triangles int32 [k,3]) of a binary little-endian or ASCII .ply: the x, y,
    z of the vertex element as read_ply_points reads them, its uchar red, green, blue where it has them, and the face element's
    `vertex_indices` (or `vertex_index`) list, of any integer count and index type. A polygon of more than three vertices is split
    as the fan (0, i, i + 1) in file order. The vertex element comes first; elements between it and the faces, and further scalar
    properties of a face, are skipped; elements after the faces are ignored. A file without a face element, or with `element face
    0`, gives triangles [0,3]. An index that does not fit int32 becomes -1 (the sampler counts such a face as invalid)."""
    blob = open(str(path), "rb").read()
    fmt, elements, body = _ply_header(path, blob)
    if [e[0] for e in elements[:1]] != ["vertex"]:
        raise SystemExit(f"{path}: the first element is not 'vertex'")
    vertices = read_ply_points(path)
    _, count, vprops = elements[0]
    names = [p[1] for p in vprops]
    has_rgb = all(c in names and _PLY_TYPES.get(vprops[names.index(c)][0]) == "u1" for c in ("red", "green", "blue"))
    ascii_ = fmt == "ascii"
    tokens = body.split() if ascii_ else None
    at = 0                                                           # position in tokens (ASCII) or in body (binary)

    def scalars(props, what):
        for p in props:
            if len(p) != 2 or p[0] not in _PLY_TYPES:
                raise SystemExit(f"{path}: property '{' '.join(p)}' of element '{what}' is not a scalar of a known type")
        return np.dtype([(f"f{i}", "<" + _PLY_TYPES[p[0]]) for i, p in enumerate(props)])

    colours = None
    vertex = scalars(vprops, "vertex")
    if has_rgb:
        if ascii_:
            table = np.array(tokens[:count * len(names)], dtype=np.float64).reshape(count, len(names))
            colours = np.stack([table[:, names.index(c)] for c in ("red", "green", "blue")], 1).astype(np.uint8)
        else:
            rec = np.frombuffer(body[:vertex.itemsize * count], dtype=vertex)
            colours = np.ascontiguousarray(np.stack([rec[f"f{names.index(c)}"] for c in ("red", "green", "blue")], 1))
    at = count * len(names) if ascii_ else vertex.itemsize * count
    empty = np.zeros((0, 3), np.int32)
    for name, n, props in elements[1:]:
        if name != "face":
            dt = scalars(props, name)                                # an element with a list before the faces cannot be skipped
            at += n * len(props) if ascii_ else n * dt.itemsize
            continue
        lists = [i for i, p in enumerate(props) if p[:1] == ["list"]]
        if len(lists) != 1 or len(props[lists[0]]) != 4 or props[lists[0]][3] not in ("vertex_indices", "vertex_index"):
            raise SystemExit(f"{path}: the face element needs one list property, vertex_indices or vertex_index")
        li = lists[0]
        _, ct, it, _ = props[li]
        if _PLY_TYPES.get(ct, "f")[0] not in "iu" or _PLY_TYPES.get(it, "f")[0] not in "iu":
            raise SystemExit(f"{path}: the face list 'property {' '.join(props[li])}' needs integer count and index types")
        before, after = scalars(props[:li], "face"), scalars(props[li + 1:], "face")
        if n == 0:
            return vertices, colours, empty
        if ascii_:
            rest = tokens[at:]
            nb, na = len(props[:li]), len(props[li + 1:])
            try:
                width = int(rest[nb]) if len(rest) > nb else -1
                row = nb + 1 + width + na
                rows = None
                if width >= 3 and len(rest) >= n * row:              # every face the same size: one table
                    table = np.array(rest[:n * row], dtype=np.float64).reshape(n, row)
                    if (table[:, nb] == width).all():
                        rows = table[:, nb + 1:nb + 1 + width].astype(np.int64)
                if rows is not None:
                    tri = _fan(rows, width)
                else:
                    out, pos = [], 0
                    for _ in range(n):
                        if pos + nb >= len(rest):
                            raise SystemExit(f"{path}: truncated")
                        w = int(rest[pos + nb])
                        if w < 3:
                            raise SystemExit(f"{path}: a face with {w} vertices")
                        if pos + nb + 1 + w + na > len(rest):
                            raise SystemExit(f"{path}: truncated")
                        out.append(_fan(np.array([rest[pos + nb + 1:pos + nb + 1 + w]], dtype=np.float64).astype(np.int64), w))
                        pos += nb + 1 + w + na
                    tri = np.concatenate(out)
            except ValueError:
                raise SystemExit(f"{path}: a face line holds something that is not a number")
        else:
            rest = body[at:]
            cdt, idt = np.dtype("<" + _PLY_TYPES[ct]), np.dtype("<" + _PLY_TYPES[it])
            if len(rest) < before.itemsize + cdt.itemsize:
                raise SystemExit(f"{path}: truncated")
            width = int(np.frombuffer(rest, cdt, 1, before.itemsize)[0])
            rows = None
            if width >= 3:                                           # every face the same size: one record type
                face = np.dtype([("b", before), ("n", cdt), ("v", idt, (width,)), ("a", after)])
                if len(rest) >= n * face.itemsize:
                    rec = np.frombuffer(rest[:n * face.itemsize], dtype=face)
                    if (rec["n"] == width).all():
                        rows = rec["v"].astype(np.int64)
            if rows is not None:
                tri = _fan(rows, width)
            else:
                out, pos = [], 0
                for _ in range(n):
                    if pos + before.itemsize + cdt.itemsize > len(rest):
                        raise SystemExit(f"{path}: truncated")
                    w = int(np.frombuffer(rest, cdt, 1, pos + before.itemsize)[0])
                    if w < 3:
                        raise SystemExit(f"{path}: a face with {w} vertices")
                    start = pos + before.itemsize + cdt.itemsize
                    if start + w * idt.itemsize + after.itemsize > len(rest):
                        raise SystemExit(f"{path}: truncated")
                    out.append(_fan(np.frombuffer(rest, idt, w, start).astype(np.int64)[None, :], w))
                    pos = start + w * idt.itemsize + after.itemsize
                tri = np.concatenate(out)
        tri = np.where((tri >= -2 ** 31) & (tri < 2 ** 31), tri, -1)
        return vertices, colours, np.ascontiguousarray(tri.astype(np.int32))
    return vertices, colours, empty


# ----------------------------------------------------------------------------------------------------------- crop files
# read_crop_file's result: the polygon's corners (U, V) in the plane orthogonal to `axis` (0, 1, 2 = X, Y, Z) as float32 [p,2], the
# bounds along the axis as float32; the fields acezero_amd.geometry.crop_to_polygon takes
CropVolume = namedtuple("CropVolume", ["polygon", "axis", "axis_min", "axis_max"])
CROP_PLANE = {0: (1, 2), 1: (0, 2), 2: (0, 1)}                        # the in-plane axes (u, v): (y, z) for X, (x, z) for Y, (x, y) for Z
CROP_MAX_CORNERS = 1024


def read_crop_file(path):
    """The crop volume of a Tanks and Temples crop file (a JSON object, the layout of Open3D's SelectionPolygonVolume): a polygon,
    `bounding_polygon` (3 .. 1024 rows of three numbers, of which the two in the plane orthogonal to `orthogonal_axis` count), swept
    along `orthogonal_axis` ("X", "Y" or "Z") from `axis_min` to `axis_max`. Returns a CropVolume, polygon and bounds rounded to
    float32 once. Other keys are ignored; `class_name`, if present, must be "SelectionPolygonVolume". Anything else is a SystemExit
    that names the file and the key."""
    import json
    import math

    def refuse(key, what):
        raise SystemExit(f"{path}: {key}: {what}")

    try:
        with open(str(path)) as f:
            doc = json.load(f)
    except (OSError, ValueError) as e:
        raise SystemExit(f"{path}: not a JSON crop file ({e})")
    if not isinstance(doc, dict):
        raise SystemExit(f"{path}: not a JSON object")
    for key in ("bounding_polygon", "orthogonal_axis", "axis_min", "axis_max"):
        if key not in doc:
            refuse(key, "missing")
    if "class_name" in doc and doc["class_name"] != "SelectionPolygonVolume":
        refuse("class_name", f"expected 'SelectionPolygonVolume', got {doc['class_name']!r}")
    axis = doc["orthogonal_axis"]
    if not isinstance(axis, str) or axis.upper() not in ("X", "Y", "Z"):
        refuse("orthogonal_axis", f"expected 'X', 'Y' or 'Z', got {axis!r}")
    axis = "XYZ".index(axis.upper())
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)
    for key in ("axis_min", "axis_max"):
        if not number(doc[key]):
            refuse(key, f"expected a finite number, got {doc[key]!r}")
    with np.errstate(over="ignore"):
        lo, hi = np.float32(doc["axis_min"]), np.float32(doc["axis_max"])
    if not (np.isfinite(lo) and np.isfinite(hi)):
        refuse("axis_min" if not np.isfinite(lo) else "axis_max", "overflows float32")
    if doc["axis_min"] > doc["axis_max"]:
        refuse("axis_min", f"{doc['axis_min']} is above axis_max {doc['axis_max']}")
    rows = doc["bounding_polygon"]
    if not isinstance(rows, list) or not 3 <= len(rows) <= CROP_MAX_CORNERS:
        refuse("bounding_polygon", f"expected 3 .. {CROP_MAX_CORNERS} rows" + (f", got {len(rows)}" if isinstance(rows, list) else ""))
    for k, row in enumerate(rows):
        if not isinstance(row, list) or len(row) != 3 or not all(number(v) for v in row):
            refuse("bounding_polygon", f"row {k} is not three finite numbers")
    with np.errstate(over="ignore"):
        polygon = np.array(rows, dtype=np.float64).astype(np.float32)[:, list(CROP_PLANE[axis])]
    if not np.isfinite(polygon).all():
        refuse("bounding_polygon", "overflows float32")
    return CropVolume(np.ascontiguousarray(polygon), axis, lo, hi)


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
