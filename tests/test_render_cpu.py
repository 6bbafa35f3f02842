"""CPU: the rasteriser's restatement (tests/render_oracle.py) on hand-worked cases, the camera set-up of libacez.so against it, the
geometry builders, the observing camera, the pose-iteration table of the final sweep, the `_mapping.pkl` round trip through
export_point_cloud.py and export_cameras.py's PLY."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import render_oracle as R
from acezero_amd import render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_TRI = (np.zeros((0, 3, 3), np.float32), np.zeros((0, 4), np.uint8))


def _frame(xyz, rgb, tri=None, rgba=None, T=None, W=16, H=12, flipped=False):
    tri, rgba = (NO_TRI if tri is None else (tri, rgba))
    return R.render(np.asarray(xyz, np.float32), np.asarray(rgb, np.uint8), tri, rgba, np.eye(4) if T is None else T, 0.05, 100.0, W, H,
                    flipped)


def test_point_lands_on_hand_computed_pixels():
    # f = (12/2) sqrt(3); (x, y, z) = (1, 0.5, -4): u = 8 + f / 4 = 10.598, v = 6 - f / 8 = 4.701 -> columns 10, 11, rows 4, 5
    img = _frame([[1.0, 0.5, -4.0]], [[10, 20, 30]])
    hit = np.argwhere(img.any(axis=2))
    assert hit.tolist() == [[4, 10], [4, 11], [5, 10], [5, 11]]
    assert (img[4, 10] == [10, 20, 30]).all()


def test_points_behind_camera_and_outside_planes_are_dropped():
    img = _frame([[0, 0, 4.0], [0, 0, -0.01], [0, 0, -200.0]], [[255, 255, 255]] * 3)
    assert not img.any()
    img = _frame([[0, 0, -0.05]], [[255, 255, 255]])      # on the near plane: drawn
    assert img.any()


def test_nearer_point_wins_and_ties_go_to_lower_index():
    img = _frame([[0, 0, -3.0], [0, 0, -2.0]], [[255, 0, 0], [0, 255, 0]])
    assert (img[5, 7] == [0, 255, 0]).all()
    img = _frame([[0, 0, -2.0], [0, 0, -2.0]], [[255, 0, 0], [0, 255, 0]])
    assert (img[5, 7] == [255, 0, 0]).all()


def _quad(z=-2.0, s=1.0):
    a, b, c, d = [-s, -s, z], [s, -s, z], [s, s, z], [-s, s, z]
    return np.array([[a, b, c], [a, c, d]], np.float32)


def test_quad_shared_edge_has_no_gap_and_no_double_coverage():
    m, f = R.camera(np.eye(4), 0.05, 100.0, 64, 48)
    for s in (0.3, 0.37, 0.5):
        keys = R.triangle_keys(_quad(-2.0, s), m, f, 0.05, 100.0, 64, 48)
        cover = keys != R.EMPTY
        ys, xs = np.nonzero(cover.reshape(48, 64))
        # the union is exactly a rectangle: every pixel of the bounding box covered once (a gap would leave a hole)
        assert cover.sum() == (ys.max() - ys.min() + 1) * (xs.max() - xs.min() + 1)
        # each triangle alone: their counts add up to the union (no pixel of the diagonal taken by both)
        n0 = (R.triangle_keys(_quad(-2.0, s)[:1], m, f, 0.05, 100.0, 64, 48) != R.EMPTY).sum()
        n1 = (R.triangle_keys(_quad(-2.0, s)[1:], m, f, 0.05, 100.0, 64, 48) != R.EMPTY).sum()
        assert n0 + n1 == cover.sum()


def test_blend_rounding_is_float_then_truncate():
    bg = np.array([[[100, 7, 255]]], np.uint8)
    fg = np.array([[[200, 8, 0, 128]]], np.uint8)
    a = 128 / 255
    expect = [int(200 * a + 100 * (1 - a)), int(8 * a + 7 * (1 - a)), int(0 * a + 255 * (1 - a))]
    assert R.blend(bg, fg)[0, 0].tolist() == expect == [150, 7, 127]      # 7.502 -> 7: truncated, not rounded


def test_triangle_layer_is_blended_over_points_without_depth_test():
    tri = np.array([[[-5, -5, -10.0], [5, -5, -10.0], [0, 5, -10.0]]], np.float32)
    img = _frame([[0, 0, -1.0]], [[0, 0, 255]], tri, np.array([[255, 0, 0, 255]], np.uint8))
    assert (img[5, 7] == [255, 0, 0]).all()                  # the far triangle covers the near point


def test_triangle_crossing_the_near_plane_is_clipped():
    tri = np.array([[[-1, -0.5, -2.0], [1, -0.5, -2.0], [0, -0.5, 1.0]]], np.float32)
    img = _frame([], [], tri, np.array([[0, 255, 0, 255]], np.uint8), W=64, H=48)
    assert img[..., 1].any() and not img[..., 0].any()


def test_portrait_rotation():
    flat = _frame([[1.0, 0.5, -4.0]], [[9, 9, 9]], W=12, H=16)
    rot = _frame([[1.0, 0.5, -4.0]], [[9, 9, 9]], W=12, H=16, flipped=True)
    assert rot.shape == (12, 16, 3)
    assert np.array_equal(rot, np.rot90(flat, -1))
    # a pixel at (row r, column c) of the render goes to (row c, column H - 1 - r)
    r, c = np.argwhere(flat.any(axis=2))[0]
    assert rot[c, 16 - 1 - r].any()


def test_library_camera_matches_restatement():
    from acezero_amd import _native as N
    lib = N.lib()
    rng = np.random.default_rng(3)
    from scipy.spatial.transform import Rotation
    for k in range(5):
        T = np.eye(4)
        T[:3, :3] = Rotation.from_rotvec(rng.normal(size=3)).as_matrix()
        T[:3, 3] = rng.normal(size=3) * 3
        w2c, f = np.zeros(12, np.float32), C.c_float(0)
        cam = (C.c_double * 16)(*T.reshape(16).tolist())
        assert lib.acez_render_camera(cam, 0.05, 100.0, 1280, 720, w2c.ctypes.data_as(C.POINTER(C.c_float)), C.byref(f)) == 0
        m, fo = R.camera(T, 0.05, 100.0, 1280, 720)
        assert np.array_equal(w2c.view(np.uint32), m.reshape(12).view(np.uint32)) and np.float32(f.value) == fo
    w2c, f = np.zeros(12, np.float32), C.c_float(0)
    assert lib.acez_render_camera(cam, 0.5, 0.1, 1280, 720, w2c.ctypes.data_as(C.POINTER(C.c_float)), C.byref(f)) == -1
    assert b"znear" in lib.acez_last_error()


def test_geometry_builders():
    m = render.cuboid_from_line([0, 0, 0], [1, 2, 3])
    assert m.verts.shape == (8, 3) and m.faces.shape == (12, 3)
    P = np.eye(4)
    P[:3, 3] = [1, 2, 3]
    fm = render.frustum_marker(P, size=0.1)
    assert fm.verts.shape == (5, 3) and fm.faces.shape == (6, 3)
    assert np.allclose(fm.verts[0], [1, 2, 3])                       # apex at the camera centre
    assert np.all(fm.verts[1:, 2] < 3)                               # base in front of the camera: -z in OpenGL
    fo = render.frustum_outline(P, size=0.3)
    assert fo.verts.shape == (64, 3) and fo.faces.shape == (96, 3)
    bx = render.box_marker(P, extent=0.2)
    assert bx.verts.shape == (8, 3) and bx.faces.shape == (12, 3) and np.allclose(bx.verts.mean(0), [1, 2, 3])
    tr = render.CameraTrajectory()
    for x in (0.0, 0.1, 0.2, 5.0, 5.1):                              # the jump 0.2 -> 5.0 draws no segment
        Q = np.eye(4)
        Q[0, 3] = x
        tr.grow_camera_path(Q)
    assert len(tr.trajectory) == 3
    tri, rgba = tr.mesh().triangles()
    assert tri.shape == (36, 3, 3) and rgba.shape == (36, 4) and tri.dtype == np.float32


def test_pan_cameras_look_at_the_scene():
    poses = []
    for i in range(20):                                             # cameras on a line along x, looking down -z (OpenGL)
        P = np.eye(4)
        P[:3, 3] = [i * 0.2, 0, 0]
        poses.append(P)
    pan = render.generate_pan(30, poses, 60)
    center = np.mean([p[:3, 3] for p in poses], axis=0)
    for P in pan:
        view = -P[:3, 2]                                             # viewing direction
        to_center = center - P[:3, 3]
        assert np.dot(view, to_center) > 0.8 * np.linalg.norm(to_center)
        assert np.allclose(P[:3, :3] @ P[:3, :3].T, np.eye(3))
    assert render.pan_camera(pan, 0) is pan[0] and render.pan_camera(pan, 30) is pan[29] and render.pan_camera(pan, 61) is pan[1]
    cam = render.LazyCamera(backwards_offset=4)
    for P in pan[:5]:
        cam.update(P)
    V = cam.current_view()
    assert np.allclose(V[:3, :3] @ V[:3, :3].T, np.eye(3)) and np.isclose(np.linalg.det(V[:3, :3]), 1)
    assert V[2, 3] > max(P[2, 3] for P in pan[:5])                    # pushed backwards along +z


def test_point_cloud_buffer_keeps_last_five():
    b = render.PointCloudBuffer()
    for i in range(7):
        b.update(np.full((2, 3), i), np.zeros((2, 3)), np.zeros(2))
    xyz, _, err = b.get()
    assert xyz[:, 0].tolist() == [2, 2, 3, 3, 4, 4, 5, 5, 6, 6] and len(err) == 10
    b.disable_cap()
    b.update(np.full((2, 3), 7), np.zeros((2, 3)))
    assert len(b.get()[0]) == 12


def test_colour_maps():
    retro = render.retro_colors()
    assert retro.shape == (256, 3) and np.allclose(retro[-1], 1) and retro[0, 2] < 0.1
    clr, norm = render.errors_to_colors(np.array([0.0, 5.0, 50.0]), 10, retro)
    assert np.allclose(norm, [1, 0.5, 0]) and np.allclose(clr[0], retro[255] * 255) and np.allclose(clr[2], retro[0] * 255)
    assert render.reloc_color_map().shape == (256, 3)


def _pose_line(name, conf):
    return f"{name} 1 0 0 0 0 0 0 500 {conf}\n"


def test_pose_iteration_table(tmp_path):
    names = ["a.png", "b.png", "c.png", "d.png"]
    confs = {"poses_iteration0_seed2.txt": [2000, 0, 0, 0], "poses_iteration1.txt": [2000, 1500, 0, 0],
             "poses_iteration2.txt": [900, 1800, 1200, 0], "poses_iteration3.txt": [3000, 3000, 3000, 10]}
    for fn, cs in confs.items():
        (tmp_path / fn).write_text("".join(_pose_line(n, c) for n, c in zip(names, cs)))
    table = render.pose_iteration_table(tmp_path / "poses_iteration3.txt", 3)
    assert table == {"a.png": 0, "b.png": 1, "c.png": 2, "d.png": 3}


def test_mapping_state_round_trips_through_export_point_cloud(tmp_path):
    xyz = np.random.default_rng(1).normal(size=(100, 3)).astype(np.float32)
    clr = np.random.default_rng(2).integers(0, 256, size=(100, 3)).astype(np.float64)
    st = {"map_xyz": xyz, "map_clr": clr, "frame_idx": 110, "camera_buffer": [np.eye(4)], "pan_cameras": [np.eye(4)] * 3}
    pkl = tmp_path / "map_mapping.pkl"
    with open(pkl, "wb") as f:
        pickle.dump(st, f)
    out = tmp_path / "pc.txt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "export_point_cloud.py"), str(out), "--visualization_buffer", str(pkl)],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    back = np.loadtxt(out)
    assert back.shape[0] == 100 and np.allclose(back[:, :3], xyz, atol=1e-5)


def _read_ply(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode().splitlines()
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in head if l.startswith("element face")][0].split()[-1])
    v = np.frombuffer(data, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")], count=nv, offset=end)
    f = np.frombuffer(data, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=nf, offset=end + v.nbytes)
    assert end + v.nbytes + f.nbytes == len(data)
    return v, f


def test_export_cameras_writes_ply(tmp_path):
    pf = tmp_path / "poses.txt"
    pf.write_text("".join(f"img{i}.png 1 0 0 0 {i * 0.1} 0 0 500 {c}\n" for i, c in enumerate([2000, 3000, 100])))
    out = tmp_path / "cams.ply"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "export_cameras.py"), str(pf), str(out)], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    v, f = _read_ply(out)
    assert len(f) == 3 * 96 and len(v) == 3 * len(f) and (f["n"] == 3).all() and f["v"].max() == len(v) - 1
    out2 = tmp_path / "markers.ply"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "export_cameras.py"), str(pf), str(out2), "--frustum_markers", "True",
                        "--draw_non_confident", "False"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    v, f = _read_ply(out2)
    assert len(f) == 2 * 6
