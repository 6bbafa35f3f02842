"""CPU: the DEFINITION of plane-sweep stereo (include/acez.h section L) checked on its numpy restatement (tests/mvs_restated.py), so
that the kernels' bit-for-bit parity with it (tests/test_mvs_gpu.py) means something; the host helpers, estimate_depth.py's refusals
and the entry points' argument checks, none of which needs a device.

Measured here with the restatement on the scene of tests/mvs_cases.py (wall at 2 m, box at 1.5 m, six cameras of 96 x 128 px 0.15 m
apart, 32 planes over 1 .. 3 m, four sources, keep 2, window radius 2): median relative error of the sweep's
pixels 0.356 %; after the check 55882 of 73728 pixels have a depth (completeness 0.7579) and 931 of them are more than 2 % off
(inaccurate share 0.01666); fused with tests/tsdf_restated.py at 2 cm voxels, min_weight 2, the mesh's vertices lie within 42.76 mm
of the scene's planes. The kernels must agree bit for bit, so the margins below only guard against edits to the scene."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import mvs_cases as MC
from tests import mvs_restated as R

COMPLETENESS = 0.7579
INACCURATE_SHARE = 0.01666
MESH_BOUND = 1.25 * 0.04276          # metres; tests/test_mvs_gpu.py imports it
N = 6


@functools.lru_cache(maxsize=None)
def scene_estimate():
    """(images, exact depths, c2w, rows, sources, uint16 maps, float32 sweep maps) of the scene, estimated by the restatement."""
    images, truth, c2w, rows = MC.scene(N)
    sources = MC.nearest_sources(N, MC.SOURCES)
    out, depths = R.estimate(images, rows, sources, [(MC.Z_NEAR, MC.Z_FAR)] * N, MC.PLANES)
    return images, truth, c2w, rows, sources, out, depths


def plane_distance(points):
    """Distance of points [n,3] to the nearest of the scene's planes: the wall, the box's front and its four sides."""
    p = np.asarray(points, np.float64)
    return np.minimum.reduce([np.abs(p[:, 2] - MC.WALL_Z), np.abs(p[:, 2] - MC.BOX_Z), np.abs(np.abs(p[:, 0]) - MC.BOX_X),
                              np.abs(np.abs(p[:, 1]) - MC.BOX_Y)])


def test_sweep_finds_the_right_plane():
    """A sweep that picks the right plane and refines nothing is off by at most half a plane step: d * step / 2 relative, taken at
    the scene's nearest depth, where it is smallest."""
    _, truth, _, _, _, _, depths = scene_estimate()
    _, step = R.plane_steps(MC.Z_NEAR, MC.Z_FAR, MC.PLANES)
    rel = np.concatenate([np.abs(d[d > 0] - t[d > 0]) / t[d > 0] for d, t in zip(depths, truth)])
    bound = MC.BOX_Z * float(step) / 2.0
    print(f"median relative error {np.median(rel):.5f}, half a plane step at {MC.BOX_Z} m {bound:.5f}, {len(rel)} pixels")
    assert len(rel) > 0.8 * N * MC.H * MC.W
    assert np.median(rel) < bound


def test_completeness_and_accuracy_after_the_check():
    _, truth, _, _, _, out, _ = scene_estimate()
    q = [o.astype(np.float64) * 0.001 for o in out]
    kept, total = sum(int((x > 0).sum()) for x in q), sum(x.size for x in q)
    bad = sum(int(((x > 0) & (np.abs(x - t) / t > 0.02)).sum()) for x, t in zip(q, truth))
    completeness, inaccurate = kept / total, bad / kept
    print(f"completeness {completeness:.4f} ({kept} of {total}), inaccurate share {inaccurate:.5f} ({bad})")
    assert completeness >= 0.5 and 1.0 - inaccurate >= 0.9, "the definition or the scene is wrong"
    assert completeness >= 0.8 * COMPLETENESS
    assert inaccurate <= 1.25 * INACCURATE_SHARE


def test_keeping_the_best_half_handles_occlusion():
    """The two middle cameras have sources on both sides of the box, so a wall pixel beside it that is hidden from one side is seen
    from the other: scoring a plane by the best two of four sources leaves fewer wrong pixels at the silhouette than scoring it by all."""
    images, truth, _, rows, sources, _, _ = scene_estimate()
    g = [R.prefilter(im) for im in images]
    wrong = {2: 0, 4: 0}
    for ref in (2, 3):
        band = MC.silhouette(truth[ref])
        assert band.sum() > 1000
        for keep in wrong:
            d, _, _ = R.sweep(g, rows, ref, sources[ref], MC.Z_NEAR, MC.Z_FAR, MC.PLANES, keep=keep)
            wrong[keep] += int(((d > 0) & band & (np.abs(d - truth[ref]) / truth[ref] > 0.02)).sum())
    print(f"pixels beyond 2 % at the silhouette: keep 2 -> {wrong[2]}, keep 4 -> {wrong[4]}")
    assert wrong[2] < wrong[4]


def test_the_check_removes_what_a_wrong_pose_produced():
    images, _, c2w, rows, _, _, _ = scene_estimate()
    sources = MC.nearest_sources(N, 2)
    ranges = [(MC.Z_NEAR, MC.Z_FAR)] * N
    good, _ = R.estimate(images, rows, sources, ranges, MC.PLANES)
    a = np.radians(2.0)
    turn = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    turned = [R.Row(np.linalg.inv(T @ turn if k == 3 else T), MC.FOCAL, MC.W / 2.0, MC.H / 2.0, MC.H, MC.W) for k, T in enumerate(c2w)]
    bad, _ = R.estimate(images, turned, sources, ranges, MC.PLANES)
    assert 3 in sources[2]
    kept = good[2] > 0
    removed = kept & (bad[2] == 0)
    print(f"frame 2: {int(kept.sum())} pixels kept, {int(removed.sum())} of them removed once source 3 is turned by 2 degrees")
    assert kept.sum() > 0.4 * MC.H * MC.W
    assert removed.sum() >= 0.5 * kept.sum()


def test_fused_mesh_lies_on_the_scene():
    """The restated chain estimate -> fuse -> extract, as estimate_depth.py and fuse_depth.py run it: where MESH_BOUND comes from."""
    from acezero_amd.fusion import bounds_from_frames
    from tests import tsdf_restated as TR
    _, _, c2w, _, _, out, _ = scene_estimate()
    origin, dims = bounds_from_frames(out, c2w, MC.FOCAL, 0.02, 0.08)
    vol = TR.Volume(origin, dims, 0.02, 0.08)
    TR.integrate(vol, out, np.linalg.inv(c2w), [MC.FOCAL] * N, [MC.W / 2.0] * N, [MC.H / 2.0] * N)
    v, _, f = TR.extract(vol.tsdf, vol.weight, None, vol.origin, vol.v, 2.0)
    dist = plane_distance(v)
    print(f"{len(v)} vertices, {len(f)} faces, largest distance to a plane of the scene {dist.max() * 1000:.2f} mm, median {np.median(dist) * 1000:.2f} mm")
    assert len(v) > 5000 and len(f) > 10000
    assert dist.max() <= MESH_BOUND


def test_prefilter_and_edge_definitions():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (13, 7), dtype=np.uint8)
    g = R.prefilter(img)
    for y, x in ((0, 0), (12, 6), (5, 3), (4, 6)):
        win = img[max(y - 4, 0):y + 5, max(x - 4, 0):x + 5].astype(np.int64)
        m = (win.sum() + win.size // 2) // win.size
        assert g[y, x] == min(max(int(img[y, x]) - m + 128, 0), 255)
    assert (R.prefilter(np.full((9, 11), 77, np.uint8)) == 128).all()            # an exposure offset disappears
    # constant images: every cost ties at 0, the first minimum is plane 0 and 0 against 0 is not unique: nothing is kept
    rows = [R.Row(np.eye(4), 50.0, 16.0, 12.0, 24, 32), R.Row(np.eye(4)[:3] + [[0, 0, 0, -0.1], [0] * 4, [0] * 4], 50.0, 16.0, 12.0, 24, 32)]
    flat = [np.full((24, 32), 128, np.uint8)] * 2
    depth, cost, plane = R.sweep(flat, rows, 0, [1], 1.0, 3.0, 9, keep=1)
    assert (depth == 0).all() and (cost[8:16, 12:20] == 0).all() and (plane[8:16, 12:20] == 0).all()
    # two planes: no neighbourhood, no end-plane rule, no refinement; the depth is the near or the far plane
    images, _, _, scene_rows = MC.scene(3)
    g = [R.prefilter(im) for im in images]
    depth, _, plane = R.sweep(g, scene_rows, 1, [0, 2], 1.5, 2.0, 2, keep=1)
    assert set(np.unique(plane)) == {0, 1} and (depth > 0).sum() > 0.5 * depth.size
    assert np.allclose(depth[(depth > 0) & (plane == 0)], 2.0, rtol=1e-6) and np.allclose(depth[(depth > 0) & (plane == 1)], 1.5, rtol=1e-6)


def test_select_sources():
    from acezero_amd.mvs import select_sources
    c2w = np.tile(np.eye(4), (7, 1, 1))
    c2w[:, 0, 3] = [0.0, 0.01, 0.1, -0.1, 0.3, 0.6, 0.2]          # baselines to frame 0 in units of the scene depth 1
    a = np.radians(40.0)
    c2w[6, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]          # looks 40 degrees away
    sizes, focals = [(24, 32)] * 7, [30.0] * 7
    src = select_sources(c2w, focals, sizes, 1.0, 4)
    assert src[0] == [2, 3, 4]                                    # 0.01 too close, 0.6 too far, frame 6 turned away; the tie by index
    assert src[6] == []                                           # nobody looks its way
    assert select_sources(c2w, focals, sizes, 1.0, 1)[0] == [2]
    assert select_sources(c2w[:1], focals[:1], sizes[:1], 1.0, 4) == [[]]
    assert select_sources(c2w, focals, sizes, 100.0, 4)[0] == []  # every baseline is below 2 % of that depth
    c2w[3] = np.nan                                               # a frame without a pose serves nobody and gets nothing
    src = select_sources(c2w, focals, sizes, 1.0, 4)
    assert src[0] == [2, 4] and src[3] == []
    # the scene's cameras: the same neighbours as tests/mvs_cases.py hands the restatement
    got = select_sources(MC.cameras(N), [MC.FOCAL] * N, [(MC.H, MC.W)] * N, np.sqrt(MC.Z_NEAR * MC.Z_FAR), MC.SOURCES)
    assert [sorted(s) for s in got] == [sorted(s) for s in MC.nearest_sources(N, MC.SOURCES)]


def test_depth_range_from_cloud():
    from acezero_amd.mvs import depth_range_from_cloud
    rng = np.random.default_rng(1)
    pts = np.stack([rng.uniform(-0.5, 0.5, 400), rng.uniform(-0.4, 0.4, 400), rng.uniform(2.0, 4.0, 400)], 1)
    behind = pts * [1, 1, -1]
    outside = pts + [50.0, 0, 0]
    w2c = np.eye(4)
    near, far = depth_range_from_cloud(np.concatenate([pts, behind, outside]), w2c, 40.0, 32.0, 24.0, 48, 64)
    z1, z99 = np.percentile(pts[:, 2], [1, 99])
    assert near == pytest.approx(z1 / 1.25) and far == pytest.approx(z99 * 1.25)
    assert depth_range_from_cloud(np.concatenate([pts[:15], behind, outside]), w2c, 40.0, 32.0, 24.0, 48, 64) is None
    assert depth_range_from_cloud(pts[:16], w2c, 40.0, 32.0, 24.0, 48, 64) is not None
    assert depth_range_from_cloud(np.zeros((0, 3)), w2c, 40.0, 32.0, 24.0, 48, 64) is None
    moved = np.eye(4)
    moved[2, 3] = 1.0                                             # world -> camera: the points are a metre further away
    assert depth_range_from_cloud(pts, moved, 40.0, 32.0, 24.0, 48, 64)[0] == pytest.approx((z1 + 1.0) / 1.25, rel=0.05)


def test_point_cloud_reader(tmp_path):
    from acezero_amd.formats import read_ply_vertices, write_ply
    from acezero_amd.pointcloud import write_point_cloud
    xyz = np.random.default_rng(2).normal(size=(37, 3)).astype(np.float32)
    write_point_cloud(tmp_path / "pc.ply", xyz, np.full((37, 3), 200.0))
    assert np.array_equal(read_ply_vertices(tmp_path / "pc.ply"), xyz)
    write_ply(tmp_path / "mesh.ply", xyz, np.zeros((37, 3), np.uint8), np.array([[0, 1, 2]], np.int32))
    assert np.array_equal(read_ply_vertices(tmp_path / "mesh.ply"), xyz)
    (tmp_path / "bad.ply").write_bytes(b"ply\nformat ascii 1.0\nend_header\n")
    with pytest.raises(SystemExit, match="not a binary"):
        read_ply_vertices(tmp_path / "bad.ply")


def native_rows(rows):
    from acezero_amd import _native as N_
    table = (N_.TsdfFrame * len(rows))()
    at = 0
    for k, r in enumerate(rows):
        table[k].m[:] = r.m.tolist()
        table[k].focal, table[k].ppx, table[k].ppy, table[k].h, table[k].w, table[k].offset = float(r.focal), float(r.ppx), float(r.ppy), r.h, r.w, at
        at += r.h * r.w
    return table, at


def test_relative_pose_is_the_librarys():
    from acezero_amd import _native as N_
    lib = N_.lib()
    _, _, _, rows = MC.scene(N)
    table, _ = native_rows(rows)
    out = (C.c_float * 12)()
    for r, s in ((0, 5), (2, 3), (4, 4)):
        assert lib.acez_mvs_relative(C.byref(table[r]), C.byref(table[s]), out) == 0
        assert np.array_equal(np.array(out[:], np.float32).view(np.uint32), R.relative(rows[r], rows[s]).view(np.uint32))
    assert lib.acez_mvs_relative(None, C.byref(table[0]), out) == -1 and b"null pointer" in lib.acez_last_error()
    table[0].m[5] = float("nan")
    assert lib.acez_mvs_relative(C.byref(table[0]), C.byref(table[1]), out) == -1 and b"non-finite" in lib.acez_last_error()


def test_host_images_without_a_gpu_are_refused():
    from acezero_amd.mvs import StereoFrames, estimate_depth_maps
    with pytest.raises(RuntimeError, match="no CPU path"):
        StereoFrames([np.zeros((8, 8), np.uint8)], world_to_cam=np.eye(4)[None], focals=10.0, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        estimate_depth_maps([np.zeros((8, 8), np.uint8)], world_to_cam=np.eye(4)[None], focals=10.0, sources=[[]], ranges=[None], device="cpu")


def test_argument_validation_without_device():
    from acezero_amd import _native as N_
    lib = N_.lib()
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data                                          # never dereferenced: every call below is refused before any launch
    rows = [R.Row(np.eye(4), 40.0, 4.0, 3.0, 6, 8) for _ in range(3)]
    table, n_pixels = native_rows(rows)
    assert n_pixels == 144
    src = (C.c_int32 * 8)(1, 2, 1, 2, 1, 2, 1, 2)

    def refused(rc, text):
        assert rc == -1 and text in lib.acez_last_error(), lib.acez_last_error()

    def prefilter(grey=p, out=p, n_pixels=144, frames=table, n_frames=3, d_frames=p):
        return lib.acez_mvs_prefilter(grey, out, n_pixels, frames, n_frames, d_frames, None)

    def sweep(g=p, n_pixels=144, frames=table, n_frames=3, ref=0, sources=src, n_sources=2, near=1.0, far=3.0, planes=16, radius=2, T=40,
              keep=1, q=5, depth=p):
        return lib.acez_mvs_sweep(g, n_pixels, frames, n_frames, ref, sources, n_sources, near, far, planes, radius, T, keep, q, depth, None, None,
                                  None)

    def check(depth=p, n_pixels=144, frames=table, n_frames=3, ref=0, sources=src, n_sources=2, tol=0.01, need=2, unit=0.001, out=p):
        return lib.acez_mvs_check(depth, n_pixels, frames, n_frames, ref, sources, n_sources, tol, need, unit, out, None)

    for call in (prefilter, sweep, check):
        refused(call(frames=None), b"null pointer")
        refused(call(n_pixels=143), b"past the end")             # 3 x 48 pixels
        refused(call(n_pixels=-1), b"negative buffer length")
        refused(call(n_frames=0), b"frame count")
    refused(prefilter(grey=None), b"null pointer")
    refused(prefilter(out=None), b"null pointer")
    refused(prefilter(d_frames=None), b"null pointer")
    refused(prefilter(n_frames=65536), b"frame count")
    refused(sweep(g=None), b"null pointer")
    refused(sweep(depth=None), b"null pointer")
    refused(sweep(sources=None), b"null pointer")
    refused(check(depth=None), b"null pointer")
    refused(check(out=None), b"null pointer")
    refused(check(sources=None), b"null pointer")
    for call in (sweep, check):
        refused(call(ref=3), b"reference index")
        refused(call(ref=-1), b"reference index")
        refused(call(n_sources=0), b"source count")
        refused(call(n_sources=9), b"source count")
        src[1] = 3
        refused(call(), b"source index")
        src[1] = -1
        refused(call(), b"source index")
        src[1] = 2
    refused(sweep(near=0.0), b"0 < near < far")
    refused(sweep(near=-1.0), b"0 < near < far")
    refused(sweep(near=3.0), b"0 < near < far")
    refused(sweep(far=float("inf")), b"0 < near < far")
    refused(sweep(near=float("nan")), b"0 < near < far")
    refused(sweep(planes=1), b"plane count")
    refused(sweep(planes=1025), b"plane count")
    refused(sweep(radius=-1), b"window radius")
    refused(sweep(radius=5), b"window radius")
    refused(sweep(T=0), b"truncation")
    refused(sweep(T=256), b"truncation")
    refused(sweep(keep=0), b"keep")
    refused(sweep(keep=3), b"keep")
    refused(sweep(q=-1), b"uniqueness")
    refused(sweep(q=101), b"uniqueness")
    refused(check(tol=-0.01), b"tolerance")
    refused(check(tol=float("nan")), b"tolerance")
    refused(check(need=-1), b"min_consistent")
    refused(check(unit=0.0), b"depth unit")
    refused(check(unit=float("inf")), b"depth unit")
    for field, value, text in (("offset", 97, b"past the end"), ("offset", -1, b"past the end"), ("w", 0, b"frame size"), ("h", 32769, b"frame size"),
                               ("focal", 0.0, b"focal"), ("focal", float("nan"), b"non-finite"), ("ppx", float("inf"), b"non-finite")):
        for row, calls in ((0, (prefilter, sweep, check)), (2, (prefilter, sweep, check))):      # the reference's row and a source's
            saved = getattr(table[row], field)
            setattr(table[row], field, value)
            for call in calls:
                refused(call(), text)
            setattr(table[row], field, saved)
    table[1].m[7] = float("inf")
    for call in (prefilter, sweep, check):
        refused(call(), b"non-finite")


def test_cli_refusals(tmp_path):
    from acezero_amd import cli
    pose_file, images = MC.write_scene(str(tmp_path), 3)
    out = str(tmp_path / "depth")
    base = [pose_file, images, out]
    rng = ["--depth_range", "1", "3"]
    for extra, text in (([], "exactly one of"),
                        (rng + ["--point_cloud", str(tmp_path / "pc.ply")], "exactly one of"),
                        (["--depth_range", "3", "1"], "0 < NEAR < FAR"),
                        (["--depth_range", "0", "1"], "0 < NEAR < FAR"),
                        (rng + ["--planes", "1"], "--planes"),
                        (rng + ["--planes", "1025"], "--planes"),
                        (rng + ["--sources", "0"], "--sources"),
                        (rng + ["--sources", "9"], "--sources"),
                        (rng + ["--keep", "5"], "--keep"),
                        (rng + ["--keep", "0"], "--keep"),
                        (rng + ["--window", "5"], "--window"),
                        (rng + ["--uniqueness", "101"], "--uniqueness"),
                        (rng + ["--tolerance", "-1"], "--tolerance"),
                        (rng + ["--min_consistent", "-1"], "--min_consistent"),
                        (rng + ["--depth_unit", "0"], "--depth_unit"),
                        (rng + ["--image_resolution", "8"], "--image_resolution"),
                        (rng + ["--confidence_threshold", "6000"], "no pose above the confidence threshold")):
        with pytest.raises(SystemExit, match=text):
            cli.estimate_depth_main(base + extra)
    with pytest.raises(SystemExit, match="no files match"):
        cli.estimate_depth_main([pose_file, str(tmp_path / "*.jpg"), out] + rng)
    (tmp_path / "pc.ply").write_bytes(b"ply\nformat ascii 1.0\nend_header\n")
    with pytest.raises(SystemExit, match="not a binary"):
        cli.estimate_depth_main(base + ["--point_cloud", str(tmp_path / "pc.ply")])
    other = tmp_path / "other"
    os.makedirs(other)
    os.rename(tmp_path / "frame_000.png", other / "elsewhere.png")
    with pytest.raises(SystemExit, match="no image of the glob has a pose"):
        cli.estimate_depth_main([pose_file, str(other / "*.png"), out] + rng)
    assert not os.path.exists(out)
