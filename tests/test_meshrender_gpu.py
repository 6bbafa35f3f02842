"""GPU: acez_meshrender (acezero_amd/csrc/meshrender_api.hip) against the numpy restatement of include/acez.h section R
(tests/meshrender_restated.py), BIT FOR BIT on every plane: depth, face, depth_u16, normal, colour, and the status count. Every route
(one lane, one wavefront, one workgroup per triangle-frame) and both sides of both thresholds are held to the same restatement, so no
tolerance appears here; tests/test_meshrender_cpu.py judges the restatement itself."""
import functools
import logging
import os
import re

import numpy as np
import pytest
import torch

from tests import fusion_cases as FC
from tests import meshrender_cases as MC
from tests import meshrender_restated as MR

pytestmark = pytest.mark.gpu
ALL = ("depth", "face", "depth_u16", "normal", "colour")


def _colours(n):
    k = np.arange(n)
    return np.stack([(37 * k) % 256, (91 * k + 5) % 256, (13 * k + 100) % 256], 1).astype(np.uint8)


def _device(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _render(v, f, colours, outputs=ALL, **kw):
    from acezero_amd.meshrender import render_mesh
    info = {}
    planes = render_mesh(_device(v), _device(f), colours=_device(colours), outputs=outputs, info=info, **kw)
    return {name: [t.cpu().numpy() for t in planes[name]] for name in outputs}, info["guard_dropped"]


def _check(v, f, sizes, c2w, focals, min_depth=0.05, max_depth=10.0, depth_unit=0.001, colours=None, routes=None):
    """Render on the device and with the restatement; every plane of every frame must be the same bits. routes: which of (small,
    medium, large) the case must exercise (from the restatement's boxes)."""
    colours = _colours(len(v)) if colours is None else colours
    table = MR.rows(sizes, cam_to_world=c2w, focals=focals)
    if routes is not None:
        taken = MC.routes(v, f, table, min_depth)
        assert all(t > 0 for t, wanted in zip(taken, routes) if wanted), f"routes taken (small, medium, large): {taken}"
    expect, status = MR.render(v, f, table, colours=colours, min_depth=min_depth, max_depth=max_depth, depth_unit=depth_unit, outputs=ALL)
    got, dropped = _render(v, f, colours, cam_to_world=c2w, focals=focals, sizes=sizes, min_depth=min_depth, max_depth=max_depth, depth_unit=depth_unit)
    assert dropped == status
    for name in ALL:
        for k, (a, b) in enumerate(zip(got[name], [fr[name] for fr in expect])):
            assert a.shape == b.shape and a.dtype == b.dtype, (name, k, a.shape, b.shape, a.dtype, b.dtype)
            same = a.view(np.uint32) == b.view(np.uint32) if name == "depth" else a == b
            assert same.all(), f"{name}, frame {k}: {(~same).sum()} of {same.size} elements differ, first at {np.argwhere(~same)[0].tolist()}"
    return expect


def test_room_large_route_and_clipping():
    v, f, _ = MC.room_mesh()
    c2w = FC.room_cameras(6)
    expect = _check(v, f, [(30, 40)] * 6, c2w, 40.0, routes=(False, True, True))
    assert all((fr["face"] >= 0).all() for fr in expect)


@functools.lru_cache(maxsize=None)
def _sphere_mesh():
    from acezero_amd.fusion import TSDFVolume
    depths, c2w, focal = FC.sphere_scene()
    vol = TSDFVolume(device="cuda", **FC.SPHERE_VOLUME)
    vol.integrate(depths, cam_to_world=c2w, focals=focal)
    v, c, f = vol.extract_mesh(min_weight=1.0)
    return v.cpu().numpy(), c.cpu().numpy(), f.cpu().numpy()


def test_sphere_small_route_mixed_sizes_and_offsets():
    v, c, f = _sphere_mesh()
    assert len(f) == 8912
    c2w = FC.sphere_cameras()[[0, 7, 12]]
    _check(v, f, [(60, 80), (45, 60), (80, 60)], c2w, [80.0, 60.0, 80.0], max_depth=4.0, colours=_colours(len(v)), routes=(True, False, False))


def test_grid_medium_route():
    v, f, c = MC.grid_mesh()
    table = MR.rows([(48, 64)], cam_to_world=MC.IDENTITY[None], focals=64.0)
    n, _ = MC.box_counts(v, f, table)
    assert (n == MC.SMALL).any() and ((n > MC.SMALL) & (n <= MC.LARGE)).any() and ((n > 0) & (n < MC.SMALL)).any()
    _check(v, f, [(48, 64)], MC.IDENTITY[None], 64.0, colours=c, routes=(True, True, False))


def test_both_thresholds_in_one_mesh():
    v, f = MC.mixed_mesh()
    n, _ = MC.box_counts(v, f, MC.mixed_table())
    for edge in (MC.SMALL, MC.LARGE):                               # a box of exactly the threshold, and one beyond it
        assert (n == edge).any() and (n > edge).any()
    _check(v, f, [(96, 128)], MC.IDENTITY[None], 100.0, routes=(True, True, True))


def test_ties_and_degenerate_triangles():
    v, f = MC.soup(MC.BASE, MC.BASE, MC.NEAR, *[MC.DROPPED[k] for k in sorted(MC.DROPPED)])
    with np.errstate(invalid="ignore"):
        expect = _check(v, f, [(24, 32)], MC.IDENTITY[None], 30.0)
    assert set(np.unique(expect[0]["face"])) == {-1, 0, 2}          # the copy (id 1) owns nothing, the dropped ones nothing


def test_guard_drop_is_counted(caplog):
    v, f = MC.soup(MC.BASE, MC.DROPPED["guard"])
    with caplog.at_level(logging.WARNING, logger="acezero_amd"):
        _, dropped = _render(v, f, None, outputs=("depth",), cam_to_world=MC.IDENTITY[None], focals=30.0, sizes=(24, 32))
    assert dropped == 1 and "2^21" in caplog.text


def test_empty_mesh_and_a_frame_that_sees_nothing():
    empty_v, empty_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    got, dropped = _render(empty_v, empty_f, np.zeros((0, 3), np.uint8), cam_to_world=MC.IDENTITY[None], focals=30.0, sizes=(24, 32))
    assert dropped == 0 and not got["depth"][0].any() and (got["face"][0] == -1).all()
    assert not got["depth_u16"][0].any() and not got["normal"][0].any() and not got["colour"][0].any()
    v, f = MC.soup(MC.BASE)
    away = FC.look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    c2w = np.stack([MC.IDENTITY, away])
    expect = _check(v, f, [(24, 32)] * 2, c2w, 30.0)
    assert (expect[0]["face"] == 0).any() and (expect[1]["face"] == -1).all() and not expect[1]["depth"].any()


def test_bad_face_index_is_refused():
    from acezero_amd import _native as N
    v, f = MC.soup(MC.BASE)
    f[0, 1] = 3
    with pytest.raises(N.AcezError, match="ACEZ_ERR_INVALID"):
        _render(v, f, None, outputs=("depth",), cam_to_world=MC.IDENTITY[None], focals=30.0, sizes=(24, 32))


def test_257_frames_are_chunked_and_equal_single_renders():
    v, f, _ = MC.room_mesh()
    n = 257
    c2w = np.stack([FC.room_cameras(n)[k] for k in range(n)])
    outputs = ("depth", "face", "depth_u16")
    got, _ = _render(v, f, None, outputs=outputs, cam_to_world=c2w, focals=8.0, sizes=(6, 8))
    assert all(len(got[name]) == n for name in outputs)
    vd, fd = _device(v), _device(f)
    from acezero_amd.meshrender import render_mesh
    singles = [render_mesh(vd, fd, cam_to_world=c2w[k:k + 1], focals=8.0, sizes=(6, 8), outputs=outputs) for k in range(n)]
    for name in outputs:
        one_by_one = torch.stack([s[name][0] for s in singles]).cpu().numpy()
        assert np.array_equal(np.stack(got[name]).view(np.uint8), one_by_one.view(np.uint8)), name
    assert (np.stack(got["face"]) >= 0).all()


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_fuse_depth_and_render_mesh_write_the_restatements_maps(tmp_path, caplog):
    from acezero_amd import cli, formats
    n, h, w, focal = 6, 60, 80, 80.0
    args = FC.write_room_scene(str(tmp_path), n=n, h=h, w=w, focal=focal)
    model_dir = tmp_path / "model"
    with caplog.at_level(logging.INFO):
        assert cli.fuse_depth_main(args + ["--model_depth_dir", str(model_dir), "--model_depth_compare", "True", "--min_component_faces", "50",
                                           "--simplify_cell", "0.06", "--min_weight", "1"]) == 0     # (the six views do not overlap)
    log = caplog.text
    # the restatement applied to the mesh that was written, under the pose file's poses
    v, _, f = FC.read_mesh_ply(os.path.join(str(tmp_path), "mesh.ply"))
    assert len(f) > 100
    names = sorted(os.listdir(tmp_path / "depth"))
    rgb_files = [os.path.join(str(tmp_path), s) for s in names]
    c2w_all, focals_all, rows = formats.read_posed_images(os.path.join(str(tmp_path), "poses.txt"), rgb_files, 1000)
    c2w = np.stack([c2w_all[k] for k in rows])
    focals = [formats.focal_at_height(focals_all[k], h, 2 * h) for k in rows]
    expect, status = MR.render(v, f, MR.rows([(h, w)] * n, cam_to_world=c2w, focals=focals), min_depth=0.05, max_depth=4.0, depth_unit=0.001)
    assert status == 0
    total = np.zeros(5, np.int64)
    for k, name in enumerate(names):
        written = _png(model_dir / name)
        assert written.dtype == np.uint16 and np.array_equal(written, expect[k]["depth_u16"]), name
        assert np.array_equal(formats.read_depth_png(model_dir / name), written)       # what fuse_depth.py --depth_files reads back
        total += MR.depth_agreement(written, _png(tmp_path / "depth" / name), 10)
    share, mean_mm, within = total[0] / total[:3].sum(), total[3] / total[0], total[4] / total[0]
    line = re.search(r"All 6 frames: valid in both maps ([0-9.]+) % .* mean \|model - measured\| ([0-9.]+) mm, within 10.0 mm ([0-9.]+) %", log)
    assert line, log[-2000:]
    assert line.groups() == (f"{100.0 * share:.2f}", f"{mean_mm:.3f}", f"{100.0 * within:.2f}")
    assert total[0] > 1000
    # render_mesh.py on that file writes the same maps, and normals and colours equal to the restatement's
    out = tmp_path / "rendered"
    with caplog.at_level(logging.INFO):
        assert cli.render_mesh_main([os.path.join(str(tmp_path), "mesh.ply"), os.path.join(str(tmp_path), "poses.txt"),
                                     os.path.join(str(tmp_path), "frame_*.png"), str(out), "--depth_files", os.path.join(str(tmp_path), "depth", "*.png"),
                                     "--max_depth", "4", "--write_normals", "True", "--write_colour", "True", "--compare_depth_files",
                                     os.path.join(str(tmp_path), "depth", "*.png"), "--output_json", str(out / "agreement.json")]) == 0
    _, colours, _ = FC.read_mesh_ply(os.path.join(str(tmp_path), "mesh.ply"))
    full, _ = MR.render(v, f, MR.rows([(h, w)] * n, cam_to_world=c2w, focals=focals), colours=colours, min_depth=0.05, max_depth=4.0,
                        outputs=("depth_u16", "normal", "colour"))
    for k, name in enumerate(names):
        assert np.array_equal(_png(out / "depth" / name), _png(model_dir / name)), name
        assert np.array_equal(_png(out / "normals" / name), full[k]["normal"]) and np.array_equal(_png(out / "colour" / name), full[k]["colour"])
    import json
    report = json.load(open(out / "agreement.json"))
    assert report["total"]["both_valid"] == total[0] and report["total"]["sum_abs_units"] == total[3] and len(report["frames"]) == n
