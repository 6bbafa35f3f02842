"""CPU: acezero_amd/formats.py, the one reader and writer of pose files, binary PLY and 16-bit depth PNGs, and the callers' views
over the one pose-file reader. Every expected value is assembled here from literals."""
import math
import os
import struct

import numpy as np
import pytest

from acezero_amd import benchmark, evaluate, formats
from acezero_amd.pointcloud import write_point_cloud

XYZ = [(0.5, -1.25, 2.0), (3.0, 4.5, -6.75), (1e-3, 0.0, -0.0)]
RGB = [(1, 2, 3), (40, 50, 60), (255, 0, 128)]
FACES = [(0, 1, 2), (2, 1, 0)]
VERTEX_HEAD = b"property float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
FACE_HEAD = b"property list uchar int vertex_indices\n"


def ply_bytes(xyz, rgb, faces=None, alpha=True):
    head = b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(xyz) + VERTEX_HEAD
    if alpha:
        head += b"property uchar alpha\n"
    if faces is not None:
        head += b"element face %d\n" % len(faces) + FACE_HEAD
    body = b"".join(struct.pack("<fffBBB", *p, *c) + (b"\xff" if alpha else b"") for p, c in zip(xyz, rgb))
    return head + b"end_header\n" + body + b"".join(struct.pack("<Biii", 3, *f) for f in faces or [])


# ------------------------------------------------------------------------------------------------------------------ PLY
def test_ply_cloud_mesh_and_camera_layouts_are_these_bytes(tmp_path):
    formats.write_ply(tmp_path / "cloud.ply", np.array(XYZ), np.array(RGB))
    assert (tmp_path / "cloud.ply").read_bytes() == ply_bytes(XYZ, RGB)
    formats.write_ply(tmp_path / "mesh.ply", np.array(XYZ, np.float32), np.array(RGB, np.uint8), np.array(FACES, np.int32))
    assert (tmp_path / "mesh.ply").read_bytes() == ply_bytes(XYZ, RGB, FACES)
    # the camera layout of export_cameras.py: a colour per face; every face gets three vertices of its own that carry it
    face_rgba = np.array([(10, 20, 30, 255), (200, 100, 0, 255)], np.uint8)
    verts, faces = np.array(XYZ), np.array(FACES)
    formats.write_ply(tmp_path / "cams.ply", verts[faces], np.repeat(face_rgba[:, :3], 3, axis=0), np.arange(6, dtype=np.int32), alpha=False)
    spread_xyz = [XYZ[0], XYZ[1], XYZ[2], XYZ[2], XYZ[1], XYZ[0]]
    spread_rgb = [(10, 20, 30)] * 3 + [(200, 100, 0)] * 3
    assert (tmp_path / "cams.ply").read_bytes() == ply_bytes(spread_xyz, spread_rgb, [(0, 1, 2), (3, 4, 5)], alpha=False)
    formats.write_ply(tmp_path / "empty.ply", np.zeros((0, 3)), np.zeros((0, 3)))
    assert (tmp_path / "empty.ply").read_bytes() == ply_bytes([], [])
    formats.write_ply(tmp_path / "no_faces.ply", np.array(XYZ), np.array(RGB), np.zeros((0, 3), np.int32))
    assert (tmp_path / "no_faces.ply").read_bytes() == ply_bytes(XYZ, RGB, [])


def test_point_cloud_colours_round_half_to_even_and_clip(tmp_path):
    xyz = [(float(i), 0.0, -1.0) for i in range(5)]
    write_point_cloud(tmp_path / "pc.ply", xyz, [[c] * 3 for c in (-0.6, 0.5, 1.5, 254.5, 300.0)])
    assert (tmp_path / "pc.ply").read_bytes() == ply_bytes(xyz, [[c] * 3 for c in (0, 0, 2, 254, 255)])
    write_point_cloud(tmp_path / "pc.txt", xyz[:2], [(0.4, 1.5, 2.5), (254.6, 9.0, 10.0)])
    assert (tmp_path / "pc.txt").read_text() == "0.0 0.0 -1.0 0 2 2\n1.0 0.0 -1.0 255 9 10\n"
    with pytest.raises(ValueError, match="use .txt or .ply"):
        write_point_cloud(tmp_path / "pc.obj", xyz, np.zeros((5, 3)))


def test_ply_vertices_read_back_exactly(tmp_path):
    (tmp_path / "cloud.ply").write_bytes(ply_bytes(XYZ, RGB))
    (tmp_path / "mesh.ply").write_bytes(ply_bytes(XYZ, RGB, FACES))
    (tmp_path / "empty.ply").write_bytes(ply_bytes([], []))
    for name in ("cloud.ply", "mesh.ply"):
        back = formats.read_ply_vertices(tmp_path / name)
        assert back.dtype == np.float32 and np.array_equal(back, np.array(XYZ, np.float32))
    assert formats.read_ply_vertices(tmp_path / "empty.ply").shape == (0, 3)
    (tmp_path / "text.ply").write_bytes(b"ply\nformat ascii 1.0\nend_header\n")
    with pytest.raises(SystemExit, match="not a binary little-endian .ply"):
        formats.read_ply_vertices(tmp_path / "text.ply")
    (tmp_path / "no_end.ply").write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 0\n")
    with pytest.raises(SystemExit, match="not a binary little-endian .ply"):
        formats.read_ply_vertices(tmp_path / "no_end.ply")
    (tmp_path / "short.ply").write_bytes(ply_bytes(XYZ, RGB)[:-1])
    with pytest.raises(SystemExit, match="truncated"):
        formats.read_ply_vertices(tmp_path / "short.ply")
    (tmp_path / "cams.ply").write_bytes(ply_bytes(XYZ, RGB, FACES, alpha=False))
    with pytest.raises(SystemExit, match="expected the vertex layout export_point_cloud.py writes"):
        formats.read_ply_vertices(tmp_path / "cams.ply")


# ----------------------------------------------------------------------------------------------------------- pose files
GOLDEN_CONFIDENCES = [math.inf, 499, 500, 2139, 323, 1837, 513, 2823, 2032, 2975, 1850, 2171]


def test_golden_pose_file_reads_exactly_in_every_view(golden_dir, tmp_path):
    """pose_file_ref.npz is what the reference reads from pose_file_ref.txt at threshold 500: float32 matrices, so the float64
    matrices read here must round to exactly them. At threshold 0 every line comes back."""
    path = os.path.join(golden_dir, "pose_file_ref.txt")
    ref = np.load(os.path.join(golden_dir, "pose_file_ref.npz"))
    files, c2w, focals = formats.read_ace_pose_file(path, 0)
    assert files == [f"scene/frame_{i:03d}.png" for i in range(12)] and focals == [525.0 + i for i in range(12)]
    assert c2w.dtype == np.float64 and c2w.shape == (12, 4, 4)
    rows = [files.index(str(f)) for f in ref["files"]]
    assert rows == [0, 2, 3, 5, 6, 7, 8, 9, 10, 11]
    assert np.array_equal(c2w[rows].astype(np.float32), ref["c2w"]) and np.array_equal(np.array(focals)[rows], ref["focals"])
    # the dict of eval_poses.py and the poses export_cameras.py draws are the same entries
    by_name = evaluate.read_pose_file_with_confidence(path)
    assert list(by_name) == files and [by_name[f][1] for f in files] == GOLDEN_CONFIDENCES
    assert all(np.array_equal(by_name[f][0], c2w[i]) for i, f in enumerate(files))
    entries = formats.read_pose_file(path, strict=False)
    assert [e.file for e in entries] == files and all(np.array_equal(np.linalg.inv(e.w2c), c2w[i]) for i, e in enumerate(entries))
    # a confidence equal to the threshold is kept; inf is a float
    assert formats.read_ace_pose_file(path, 500)[0] == [str(f) for f in ref["files"]]
    assert entries[0].confidence == math.inf and isinstance(entries[0].confidence, float) and entries[0].confidence_text == "inf"
    # the benchmark keeps integer confidences: inf is no integer literal
    with pytest.raises(ValueError):
        benchmark.parse_pose_file(path)
    (tmp_path / "ints.txt").write_text(open(path).read().replace(" inf\n", " 4000\n"))
    rows = benchmark.parse_pose_file(tmp_path / "ints.txt")
    assert [r[3] for r in rows] == [4000] + GOLDEN_CONFIDENCES[1:] and all(type(r[3]) is int for r in rows)
    assert all(np.array_equal(np.linalg.inv(r[1]), c2w[i]) and r[2] == 525.0 + i for i, r in enumerate(rows))


def test_pose_line_from_literals(tmp_path):
    """An identity rotation (exact in float64) and a quarter turn about z (to 1e-15)."""
    e = formats.parse_pose_line("a/b_c.png 1 0 0 0 0.5 -2 4 500.5 1e3")
    assert (e.file, e.focal, e.confidence, e.confidence_text) == ("a/b_c.png", 500.5, 1000.0, "1e3")
    assert np.array_equal(e.w2c, [[1, 0, 0, 0.5], [0, 1, 0, -2], [0, 0, 1, 4], [0, 0, 0, 1]])
    (tmp_path / "p.txt").write_text("x.png 1 0 0 0 0.5 -2 4 500.5 7\nx.png 1 0 0 0 1 1 1 300 9\n")
    files, c2w, focals = formats.read_ace_pose_file(tmp_path / "p.txt", 8)
    assert files == ["x.png"] and focals == [300.0] and np.array_equal(c2w, [[[1, 0, 0, -1], [0, 1, 0, -1], [0, 0, 1, -1], [0, 0, 0, 1]]])
    by_name = evaluate.read_pose_file_with_confidence(tmp_path / "p.txt")              # the later line of a name replaces the earlier one
    assert list(by_name) == ["x.png"] and by_name["x.png"][1] == 9.0 and np.array_equal(by_name["x.png"][0], c2w[0])
    s = math.sqrt(0.5)
    w2c = formats.parse_pose_line(f"q.png {s} 0 0 {s} 0 0 0 1 1").w2c                 # x -> y, y -> -x
    assert np.allclose(w2c, [[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], rtol=0, atol=1e-15)
    empty = formats.read_ace_pose_file(tmp_path / "p.txt", 10)
    assert empty[0] == [] and empty[1].shape == (0, 4, 4) and empty[2] == []


@pytest.mark.parametrize("bad", ["x.png 1 0 0 0 1 2 3 500\n", "\n"], ids=["nine_fields", "blank"])
def test_malformed_lines_are_refused_or_skipped(tmp_path, bad):
    good = "a.png 1 0 0 0 1 2 3 500 2000\n"
    (tmp_path / "p.txt").write_text(good + bad + good.replace("a.png", "b.png"))
    for strict_view in (lambda p: formats.read_ace_pose_file(p, 0), formats.read_pose_file, evaluate.read_pose_file_with_confidence,
                        benchmark.parse_pose_file):
        with pytest.raises(AssertionError, match="Expected 10 tokens per line in pose file"):
            strict_view(tmp_path / "p.txt")
    assert [e.file for e in formats.read_pose_file(tmp_path / "p.txt", strict=False)] == ["a.png", "b.png"]


def test_written_pose_line_reads_back(tmp_path):
    a, b = 0.3, -1.1
    rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = rz @ rx, [1.5, -2.0, 0.25]
    with open(tmp_path / "p.txt", "w") as f:
        formats.write_pose_line(f, "a/b.png", w2c, 1234, 525.25)
        formats.write_pose_line(f, "seed.png", np.eye(4), float("inf"), 0.1)
    first, seed = formats.read_pose_file(tmp_path / "p.txt")
    assert np.abs(first.w2c - w2c).max() <= 1e-12
    assert (first.file, first.focal, first.confidence, first.confidence_text) == ("a/b.png", 525.25, 1234.0, "1234")
    assert np.array_equal(seed.w2c, np.eye(4)) and (seed.focal, seed.confidence) == (0.1, math.inf)


def test_match_poses():
    names = ["scene/a.png", "b.png", "other/c.png", "again/c.png", "a.png"]
    files = ["scene/a.png", "elsewhere/a.png", "x/b.png", "y/c.png", "d.png", "again/c.png", "other/c.png"]
    #        full name wins  basename: last a  basename  last c      absent   full name      full name beats the later basename
    assert formats.match_poses(names, files) == [0, 4, 1, 3, None, 3, 2]
    assert formats.match_poses([], ["a.png"]) == [None] and formats.match_poses(names, []) == []


# ------------------------------------------------------------------------------------------------------------ depth PNG
def test_depth_png_round_trip(tmp_path):
    from PIL import Image
    depth = np.array([[0, 1, 1000], [65535, 1000, 0]], np.uint16)
    formats.write_depth_png(tmp_path / "d.png", depth)
    with Image.open(tmp_path / "d.png") as im:
        assert im.size == (3, 2) and im.mode.startswith("I;16")
    back = formats.read_depth_png(tmp_path / "d.png")
    assert back.dtype == np.uint16 and back.flags["C_CONTIGUOUS"] and np.array_equal(back, [[0, 1, 1000], [65535, 1000, 0]])
    Image.fromarray(np.zeros((2, 3, 3), np.uint8)).save(tmp_path / "rgb.png")
    with pytest.raises(SystemExit, match="one channel"):
        formats.read_depth_png(tmp_path / "rgb.png")
