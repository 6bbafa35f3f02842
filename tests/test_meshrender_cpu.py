"""CPU: the restatement of include/acez.h section R (tests/meshrender_restated.py) against geometry with a closed form, the library's
argument checks without a device, depth_agreement on hand-made maps and the new command-line flags. Here the definition is judged;
tests/test_meshrender_gpu.py then holds the kernels to the restatement bit for bit.

The round trip, measured here with the restatements (tests/tsdf_restated.py, tests/meshrender_restated.py): the sphere scene fused at
min_weight 1, its mesh rendered from the 14 fusing cameras and compared with the depth that was fused: mean |delta| 3.228 mm over the
27902 pixels valid in both maps, which are 98.088 % of the pixels valid in either (the other 544 are the model's alone: the mesh is
a little larger than the sphere, tests/test_fusion_cpu.py). Asserted with the margins
tests/test_fusion_cpu.py uses for its measured bounds: 1.25 x the mean, 0.98 x the share."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import fusion_cases as FC
from tests import meshrender_cases as MC
from tests import meshrender_restated as MR

ROUND_TRIP_MEAN_MM = 1.25 * 3.228
ROUND_TRIP_SHARE = 0.98 * 0.98088


def _one(vertices, faces, table=None, **kw):
    frames, status = MR.render(vertices, faces, table or MC.small_table(), **{"max_depth": 10.0, **kw})
    return frames[0], status


# ------------------------------------------------------------------------------------------------------------ coverage and depth
def test_fronto_parallel_plane_is_exact_and_covered_once():
    table = MR.rows([(16, 24)], cam_to_world=MC.IDENTITY[None], focals=20.0)
    for z, x1 in ((2.0, 0.5), (1.5, 0.43), (3.0, 0.61)):
        v, f = MC.quad(z, -0.5, x1, -0.3, 0.3)
        out, _ = _one(v, f, table, outputs=("depth", "face"))
        cover = out["face"] >= 0
        # z = 2: iz = 1/2 and every edge function is an integer below 2^24 (the quad is 2560 x 1536 sub-pixels), so every product and
        # sum of step 7 is exact and the depth is the plane's, bit for bit. Other depths round 1 / z, three products, two sums and
        # two quotients: within 8 units of 2^-24
        if z == 2.0:
            assert (out["depth"][cover] == np.float32(2.0)).all()
        assert (np.abs(out["depth"][cover].astype(np.float64) / z - 1.0) <= 8 * 2.0 ** -24).all() and (out["depth"][~cover] == 0).all()
        ys, xs = np.nonzero(cover)
        # the union is exactly a rectangle (no hole), and the triangles alone add up to it (no pixel of the diagonal taken twice)
        assert cover.sum() == (ys.max() - ys.min() + 1) * (xs.max() - xs.min() + 1) > 20
        alone = [(_one(v, f[k:k + 1], table, outputs=("face",))[0]["face"] >= 0).sum() for k in range(2)]
        assert alone[0] + alone[1] == cover.sum() and min(alone) > 0
        # the sample of pixel (ix, iy) is the point (ix, iy): the covered columns are those with x0 <= (ix - ppx) z / f < x1 or so
        u0, u1 = 20.0 * -0.5 / z + 12.0, 20.0 * x1 / z + 12.0
        assert xs.min() == math.ceil(u0 - 1e-6) and xs.max() in (math.floor(u1 + 1e-6), math.ceil(u1) - 1)


def test_box_room_matches_the_analytic_depth_without_a_crack():
    v, f, _ = MC.room_mesh()
    c2w, table = MC.room_table(6, 30, 40, 40.0)
    small, medium, large = MC.routes(v, f, table)
    assert medium > 0 and large > 0                                 # most triangles cross the near plane; some fill the image
    frames, status = MR.render(v, f, table, min_depth=0.05, max_depth=10.0, depth_unit=0.001)
    assert status == 0
    for k, fr in enumerate(frames):
        ref = FC.room_depth(c2w[k], 30, 40, 40.0).astype(np.int64)
        slope = max(np.abs(np.diff(ref, axis=0)).max(), np.abs(np.diff(ref, axis=1)).max())     # units per pixel, from the analytic depth
        snap = math.ceil(slope / 256.0)                                                         # vertices move by up to 1/256 px
        d = fr["depth_u16"].astype(np.int64)
        assert (d > 0).all(), f"frame {k}: {(d == 0).sum()} empty pixels"
        worst = np.abs(d - ref).max()
        print(f"frame {k}: largest |delta| {worst} units, bound 1 + {snap}")
        assert worst <= 1 + snap


def test_ties_go_to_the_lower_id_and_a_nearer_triangle_owns_its_coverage():
    v, f = MC.soup(MC.BASE, MC.BASE)
    out, _ = _one(v, f, outputs=("face",))
    assert (out["face"] >= 0).sum() > 100 and set(np.unique(out["face"])) == {-1, 0}
    swapped, _ = _one(v, f[::-1].copy(), outputs=("face",))         # (ids follow the rows)
    assert np.array_equal(swapped["face"], out["face"])
    v, f = MC.soup(MC.BASE, MC.NEAR)
    both, _ = _one(v, f, outputs=("face", "depth"))
    near_alone, _ = _one(*MC.soup(MC.NEAR), outputs=("face",))
    base_alone, _ = _one(*MC.soup(MC.BASE), outputs=("face",))
    assert np.array_equal(both["face"] == 1, near_alone["face"] == 0) and (near_alone["face"] == 0).sum() > 10
    assert np.array_equal(both["face"] >= 0, base_alone["face"] >= 0)
    for face, z in ((1, 1.5), (0, 2.0)):                            # (step 7 rounds some seven times: within 8 units of 2^-24)
        assert (np.abs(both["depth"][both["face"] == face].astype(np.float64) / z - 1.0) <= 8 * 2.0 ** -24).all()


@pytest.mark.parametrize("name", sorted(MC.DROPPED))
def test_dropped_triangles_leave_the_image_unchanged(name):
    outputs = ("depth", "face", "depth_u16", "normal")
    alone, status0 = _one(*MC.soup(MC.BASE, MC.NEAR), outputs=outputs)
    v, f = MC.soup(MC.BASE, MC.NEAR, MC.DROPPED[name])
    out, status = _one(v, f, outputs=outputs)
    for plane in outputs:
        assert np.array_equal(out[plane], alone[plane]), plane
    assert status0 == 0 and status == (1 if name == "guard" else 0)


def test_depth_beyond_max_depth_and_u16_range():
    v, f = MC.soup(MC.BASE)
    out, _ = _one(v, f, max_depth=1.9, outputs=("depth",))
    assert not out["depth"].any()
    out, _ = _one(v, f, depth_unit=0.00002, outputs=("depth", "depth_u16"))      # 2 m = 100000 units: beyond uint16
    assert out["depth"].any() and not out["depth_u16"].any()


# ------------------------------------------------------------------------------------------------------------ colour and normals
RGB_TRIANGLE = np.array([[-0.7, -0.5, 1.2], [0.8, -0.4, 2.5], [0.1, 0.7, 1.6]], np.float32)
RGB = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)


def test_colour_is_perspective_correct():
    v, f = MC.soup(RGB_TRIANGLE)
    table = MR.rows([(48, 64)], cam_to_world=MC.IDENTITY[None], focals=50.0)
    out, _ = _one(v, f, table, colours=RGB, outputs=("colour", "face"))
    ys, xs = np.nonzero(out["face"] == 0)
    assert len(ys) > 300
    # analytic: the pixel's ray meets the triangle's plane; barycentrics of that point, in float64
    P = RGB_TRIANGLE.astype(np.float64)
    n = np.cross(P[1] - P[0], P[2] - P[0])
    rays = np.stack([(xs - 32.0) / 50.0, (ys - 24.0) / 50.0, np.ones(len(xs))], 1)
    X = rays * ((P[0] @ n) / (rays @ n))[:, None]
    bary = np.stack([np.cross(P[(k + 1) % 3] - X, P[(k + 2) % 3] - X) @ n for k in range(3)], 1) / (n @ n)
    assert np.allclose(bary.sum(1), 1.0)
    assert np.abs(out["colour"][ys, xs].astype(np.float64) - 255.0 * bary).max() <= 1.0
    assert not out["colour"][out["face"] < 0].any()


def test_clipping_does_not_change_the_colours():
    tri = np.array([[-0.6, -0.4, 0.3], [0.7, -0.3, 2.0], [0.0, 0.6, 1.1]], np.float32)
    v, f = MC.soup(tri)
    table = MR.rows([(48, 64)], cam_to_world=MC.IDENTITY[None], focals=50.0)
    clipped, _ = _one(v, f, table, colours=RGB, min_depth=0.8, outputs=("colour", "face", "normal"))
    whole, _ = _one(v, f, table, colours=RGB, min_depth=0.01, outputs=("colour", "face", "normal"))
    both = (clipped["face"] == 0) & (whole["face"] == 0)
    assert 50 < both.sum() < (whole["face"] == 0).sum()
    assert np.array_equal(clipped["colour"][both], whole["colour"][both]) and np.array_equal(clipped["normal"][both], whole["normal"][both])


def test_room_normals_are_the_walls_axes():
    v, f, axes = MC.room_mesh()
    c2w, table = MC.room_table(6, 30, 40, 40.0)
    frames, _ = MR.render(v, f, table, outputs=("normal", "face"))
    for k, fr in enumerate(frames):
        n_cam = (fr["normal"].astype(np.float64) - 128.0) / 127.0
        n_world = n_cam.reshape(-1, 3) @ c2w[k][:3, :3].T
        expect = -axes[fr["face"].reshape(-1)]                       # towards the camera: into the room
        assert np.abs(n_world - expect).max() <= 1.0 / 127.0 + 1e-6  # half a step of the encoding per component, times sqrt(3) <= 1 step


# ------------------------------------------------------------------------------------------------------------ the round trip
def test_round_trip_of_the_fused_sphere():
    from tests.test_fusion_cpu import sphere_mesh
    depths, c2w, focal = FC.sphere_scene()
    v, _, f = sphere_mesh()
    table = MR.rows([d.shape for d in depths], cam_to_world=c2w, focals=focal)
    frames, status = MR.render(v, f, table, min_depth=0.05, max_depth=4.0, depth_unit=0.001)
    total = np.zeros(5, np.int64)
    for fr, d in zip(frames, depths):
        total += MR.depth_agreement(fr["depth_u16"], d, 10)
    both, model_only, measured_only, sum_abs, _ = total
    mean_mm, share = sum_abs / both, both / (both + model_only + measured_only)
    print(f"round trip: mean |delta| {mean_mm:.4f} mm over {both} pixels valid in both, {100.0 * share:.3f} % of those valid in either "
          f"({model_only} model only, {measured_only} measured only)")
    assert status == 0
    assert mean_mm <= ROUND_TRIP_MEAN_MM and share >= ROUND_TRIP_SHARE


# ------------------------------------------------------------------------------------------------------------ depth_agreement
def test_depth_agreement_on_hand_made_maps():
    from acezero_amd.meshrender import agreement_line, depth_agreement
    model = np.array([[1000, 0, 2000, 65535], [0, 500, 40000, 7]], np.uint16)
    measured = np.array([[1010, 300, 0, 1], [0, 489, 40012, 7]], np.uint16)
    counts = depth_agreement(model, measured, 10)
    assert counts == (5, 1, 1, 10 + 65534 + 11 + 12 + 0, 2) == MR.depth_agreement(model, measured, 10)
    assert depth_agreement(torch.from_numpy(model), torch.from_numpy(measured.view(np.int16)), 12)[4] == 4
    share, mean_mm, within = agreement_line(counts, 0.001)
    assert share == 5 / 7 and within == 2 / 5 and math.isclose(mean_mm, counts[3] / 5)
    assert all(math.isnan(x) for x in agreement_line((0, 0, 0, 0, 0), 0.001))
    with pytest.raises(ValueError):
        depth_agreement(model, measured[:1], 10)


# ------------------------------------------------------------------------------------------------------------ the library's checks
def _call(lib, N, **change):
    """acez_meshrender on host memory standing in for the device's: the checks come before anything touches it."""
    a = dict(n_vertices=3, n_faces=1, h=4, w=6, focal=10.0, ppx=3.0, ppy=2.0, offset=0, min_depth=0.05, max_depth=4.0, depth_unit=0.001, n_keys=24,
             n_pixels=24, n_frames=1, keys=True, depth=True, status=True, colour=False, colours=False, m0=1.0)
    a.update(change)
    rows = (N.TsdfFrame * 1)()
    rows[0].m[:] = [a["m0"], 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    rows[0].focal, rows[0].ppx, rows[0].ppy, rows[0].h, rows[0].w, rows[0].offset = a["focal"], a["ppx"], a["ppy"], a["h"], a["w"], a["offset"]
    buf = np.zeros(4096, np.uint8)
    p = lambda on: C.c_void_p(buf.ctypes.data if on else 0)
    return lib.acez_meshrender(p(True), p(a["colours"]), a["n_vertices"], p(True), a["n_faces"], rows, a["n_frames"], p(True), a["min_depth"],
                               a["max_depth"], a["depth_unit"], p(a["keys"]), a["n_keys"], p(a["depth"]), None, None, None, p(a["colour"]),
                               a["n_pixels"], p(a["status"]), None)


def test_library_refuses_invalid_arguments_before_touching_a_device():
    from acezero_amd import _native as N
    lib = N.lib()
    assert (N.MESHRENDER_SMALL, N.MESHRENDER_LARGE) == (MC.SMALL, MC.LARGE)
    faces = np.array([[0, 1, 2], [2, 1, 0]], np.int32)
    assert lib.acez_meshrender_check_faces(faces.ctypes.data, 2, 3) == 0
    for bad in (3, -1):
        faces[1, 2] = bad
        assert lib.acez_meshrender_check_faces(faces.ctypes.data, 2, 3) == -1 and b"face index" in lib.acez_last_error()
    assert lib.acez_meshrender_check_faces(None, 0, 0) == 0 and lib.acez_meshrender_check_faces(None, 1, 3) == -1
    if not torch.cuda.is_available():                                # the valid call passes every check (with a device it would run,
        assert _call(lib, N) == -3 and b"no HIP device" in lib.acez_last_error()      # on host memory: never made there)
    invalid = [dict(h=0), dict(w=40000), dict(focal=0.0), dict(focal=float("nan")), dict(m0=float("inf")), dict(offset=-1), dict(offset=1),
               dict(ppx=2.0e6), dict(min_depth=0.0), dict(min_depth=-1.0), dict(max_depth=0.0), dict(max_depth=float("inf")),
               dict(depth_unit=0.0), dict(depth_unit=float("nan")), dict(n_keys=23), dict(n_pixels=23), dict(n_frames=257), dict(n_frames=-1),
               dict(keys=False), dict(depth=False), dict(status=False), dict(colour=True), dict(n_faces=-1), dict(n_faces=1, n_vertices=0)]
    for change in invalid:
        assert _call(lib, N, **change) == -1, change
    assert _call(lib, N, n_frames=0) == 0                           # nothing to do, with or without a device


def test_render_mesh_needs_device_tensors():
    from acezero_amd.meshrender import render_mesh
    v, f = MC.soup(MC.BASE)
    with pytest.raises(RuntimeError, match="no CPU path"):
        render_mesh(torch.from_numpy(v), torch.from_numpy(f), cam_to_world=MC.IDENTITY[None], focals=30.0, sizes=(24, 32))


# ------------------------------------------------------------------------------------------------------------ command line
def test_new_arguments_parse_and_default_to_off():
    from acezero_amd import cli
    opt = cli.render_mesh_parser().parse_args(["mesh.ply", "poses.txt", "rgb/*.png", "out"])
    assert (opt.image_resolution, opt.depth_files, opt.compare_depth_files, opt.output_json) == (None, None, None, None)
    assert (opt.write_normals, opt.write_colour, opt.depth_unit, opt.min_depth, opt.confidence_threshold) == (False, False, 0.001, 0.05, 1000)
    opt = cli.render_mesh_parser().parse_args(["mesh.ply", "poses.txt", "rgb/*.png", "out", "--depth_files", "d/*.png", "--depth_unit", "0.0005",
                                               "--min_depth", "0.1", "--max_depth", "8", "--confidence_threshold", "500", "--write_normals", "True",
                                               "--write_colour", "True", "--compare_depth_files", "d/*.png", "--compare_tolerance", "0.02",
                                               "--output_json", "a.json", ])
    assert (opt.depth_files, opt.depth_unit, opt.min_depth, opt.max_depth, opt.write_normals, opt.write_colour, opt.compare_tolerance) == \
        ("d/*.png", 0.0005, 0.1, 8.0, True, True, 0.02)
    assert cli.render_mesh_parser().parse_args(["m.ply", "p.txt", "*.png", "out", "--image_resolution", "240"]).image_resolution == 240
    base = ["poses.txt", "rgb/*.png", "mesh.ply", "--depth_files", "d/*.png"]
    opt = cli.fuse_depth_parser().parse_args(base)
    assert opt.model_depth_dir is None and opt.model_depth_compare is False
    opt = cli.fuse_depth_parser().parse_args(base + ["--model_depth_dir", "model", "--model_depth_compare", "True"])
    assert str(opt.model_depth_dir) == "model" and opt.model_depth_compare is True
    with pytest.raises(SystemExit):
        cli.fuse_depth_main(base + ["--model_depth_compare", "True"])
    with pytest.raises(SystemExit):
        cli.render_mesh_main(["m.ply", "p.txt", "*.png", "out", "--image_resolution", "240", "--depth_files", "d/*.png"])
