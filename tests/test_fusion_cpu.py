"""CPU: the DEFINITION of TSDF fusion and surface-net extraction (include/acez.h section K) checked on its numpy restatement
(tests/tsdf_restated.py), so that the kernels' bit-for-bit parity with it (tests/test_fusion_gpu.py) means something; the PLY writer,
fuse_depth.py's refusals and the entry points' argument checks, none of which needs a device.

Measured here with the restatement on the sphere scene (radius 0.3 m, v = 0.02 m, tau = 4 v, 48^3 voxels, 14 cameras of 80 x 60 px,
min_weight 1): signed volume 1.59 % above 4/3 pi r^3, largest vertex distance to the sphere 7.80 mm. Asserted
with 25 % headroom; one voxel is the sanity ceiling of the distance. With min_weight 2 the same cameras leave 256 open edges (corners
just inside the surface that only one camera reaches within the truncation), so the sphere is extracted at min_weight 1."""
import functools
import os

import numpy as np
import pytest

from tests import fusion_cases as FC
from tests import tsdf_restated as R

VOLUME_MARGIN = 1.25 * 0.0159        # relative to 4/3 pi r^3
DISTANCE_BOUND = 1.25 * 0.00780      # metres; tests/test_fusion_gpu.py imports it


@functools.lru_cache(maxsize=None)
def sphere_volume():
    depths, c2w, focal = FC.sphere_scene()
    vol = R.Volume(**{k: FC.SPHERE_VOLUME[k] for k in ("origin", "dims", "voxel_size", "truncation")})
    n = len(depths)
    R.integrate(vol, depths, np.linalg.inv(c2w), [focal] * n, [40.0] * n, [30.0] * n)
    return vol


@functools.lru_cache(maxsize=None)
def sphere_mesh():
    vol = sphere_volume()
    return R.extract(vol.tsdf, vol.weight, vol.colour, vol.origin, vol.v, 1.0)


def test_sphere_is_a_closed_oriented_surface_of_the_right_size():
    v, _, f = sphere_mesh()
    assert len(v) > 1000 and len(f) > 2000
    assert f.min() >= 0 and f.max() < len(v)
    undirected, directed = FC.mesh_edge_counts(f)
    assert (undirected == 2).all(), f"{int((undirected != 2).sum())} edges do not belong to exactly two faces"
    assert (directed == 1).all(), "two faces run through an edge in the same direction: the orientation is not consistent"
    volume, exact = FC.signed_volume(v, f), 4.0 / 3.0 * np.pi * FC.SPHERE_R ** 3
    distance = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - FC.SPHERE_R).max()
    print(f"signed volume {volume:.6f} m^3 ({(volume - exact) / exact:+.4%} of the sphere's), largest distance {distance * 1000:.3f} mm")
    assert volume > 0, "normals point inwards"
    assert abs(volume - exact) <= VOLUME_MARGIN * exact
    assert distance <= DISTANCE_BOUND < 0.02


def test_chunking_does_not_change_a_bit():
    depths, c2w, focal = FC.sphere_scene()
    depths, w2c = depths[:5], np.linalg.inv(c2w[:5])
    rgbs = [np.random.default_rng(k).integers(0, 256, d.shape + (3,), dtype=np.uint8) for k, d in enumerate(depths)]
    args = dict(origin=(-0.31, -0.29, -0.33), dims=(31, 29, 33), voxel_size=0.02, truncation=0.08, max_weight=3.0)
    once = R.integrate(R.Volume(**args), depths, w2c, [focal] * 5, [40.0] * 5, [30.0] * 5, rgbs)
    parts = R.Volume(**args)
    for lo, hi in ((0, 2), (2, 4), (4, 5)):
        R.integrate(parts, depths[lo:hi], w2c[lo:hi], [focal] * (hi - lo), [40.0] * (hi - lo), [30.0] * (hi - lo), rgbs[lo:hi])
    assert once.weight.max() == 3.0 and (once.weight > 0).sum() > 1000
    for a, b in ((once.tsdf, parts.tsdf), (once.weight, parts.weight), (once.colour, parts.colour)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_camera_inside_a_room():
    """One camera inside the box room, its far wall beyond max_depth, a hole in its depth image."""
    h, w, focal, max_depth = 120, 160, 80.0, 0.9
    c2w = FC.look_at((0.03, -0.02, -0.3), (0.03, -0.02, 1.0))
    depth = FC.room_depth(c2w, h, w, focal)
    depth[40:60, 100:120] = 0
    vol = R.Volume((-0.7, -0.6, -0.8), (71, 61, 81), 0.02, 0.08)
    R.integrate(vol, [depth], np.linalg.inv(c2w)[None], [focal], [w / 2.0], [h / 2.0], max_depth=max_depth)
    # every voxel's fate in float64, with a margin around each decision so that fp32 rounding cannot flip it
    x, y, z = (a.astype(np.float64) for a in vol.centres())
    p = np.stack(np.broadcast_arrays(x[None, None, :], y[None, :, None], z[:, None, None]), -1)
    cam = (p - c2w[:3, 3]) @ c2w[:3, :3]
    zc = cam[..., 2]
    with np.errstate(all="ignore"):
        u, v_ = focal * cam[..., 0] / zc + w / 2.0, focal * cam[..., 1] / zc + h / 2.0
    eps = 1e-3
    behind = zc < -eps
    outside = (zc > eps) & ((u < -0.5 - eps) | (u > w - 0.5 + eps) | (v_ < -0.5 - eps) | (v_ > h - 0.5 + eps))
    clear = (zc > eps) & (u > -0.5 + eps) & (u < w - 0.5 - eps) & (v_ > -0.5 + eps) & (v_ < h - 0.5 - eps)
    clear &= (np.abs(u + 0.5 - np.rint(u + 0.5)) > eps) & (np.abs(v_ + 0.5 - np.rint(v_ + 0.5)) > eps)    # not on a pixel boundary
    ix = np.clip(np.floor(u + 0.5), 0, w - 1).astype(int)
    iy = np.clip(np.floor(v_ + 0.5), 0, h - 1).astype(int)
    raw = depth[iy, ix].astype(np.float64)
    hole = clear & (raw == 0)
    too_far = clear & (raw * 0.001 > max_depth + 1e-6)
    seen = clear & (raw > 0) & (raw * 0.001 < max_depth - 1e-6) & (raw * 0.001 - zc > -0.08 + eps)
    for name, mask in (("behind the camera", behind), ("outside the image", outside), ("on the hole", hole), ("beyond max_depth", too_far)):
        assert mask.sum() > 500, name
        assert (vol.weight[mask] == 0).all(), name
    assert seen.sum() > 500 and (vol.weight[seen] == 1).all()
    v, _, f = R.extract(vol.tsdf, vol.weight, None, vol.origin, vol.v, 1.0)
    assert len(v) > 1000 and len(f) > 1000
    wd = FC.wall_distance(v)
    print(f"largest vertex distance to a wall plane {wd.max() * 1000:.3f} mm")
    assert wd.max() <= DISTANCE_BOUND
    # the far wall (z-depth 1.01 m > max_depth) is not in the mesh; the side walls, the floor and the ceiling are
    assert (np.abs(v[:, 2] - FC.ROOM_HALF[2]) > 0.05).all()
    assert (np.abs(np.abs(v[:, 0]) - FC.ROOM_HALF[0]) < DISTANCE_BOUND).sum() > 200


def test_extraction_edge_cases():
    o, v = (0.0, 0.0, 0.0), 0.5
    tsdf, weight = np.ones((3, 3, 3), np.float32), np.zeros((3, 3, 3), np.float32)
    vert, col, faces = R.extract(tsdf, weight, None, o, v, 1.0)
    assert vert.shape == (0, 3) and col.shape == (0, 3) and faces.shape == (0, 3)
    weight[:2, :2, :2] = 1.0                                    # one cell known, its corner 0 inside
    tsdf[0, 0, 0] = -1.0
    vert, _, faces = R.extract(tsdf, weight, None, o, v, 1.0)
    assert faces.shape == (0, 3) and vert.shape == (1, 3)
    assert np.array_equal(vert[0], np.full(3, np.float32(0.5) / np.float32(3) * np.float32(0.5), np.float32))                   # three crossings at s = 0.5, one per axis
    vert, _, faces = R.extract(np.ones((1, 4, 2), np.float32), np.ones((1, 4, 2), np.float32), None, o, v, 1.0)
    assert vert.shape == (0, 3) and faces.shape == (0, 3)       # nz = 1: no cell


def test_ply_round_trip(tmp_path):
    from acezero_amd.formats import write_ply
    v, c, f = sphere_mesh()
    c = (np.arange(len(v) * 3) % 251).astype(np.uint8).reshape(-1, 3)
    path = tmp_path / "mesh.ply"
    write_ply(path, v, c, f)
    blob = path.read_bytes()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    assert f"element vertex {len(v)}" in lines and f"element face {len(f)}" in lines
    assert lines[-1] == "property list uchar int vertex_indices"
    assert len(body) == len(v) * 16 + len(f) * 13
    vrec = np.frombuffer(body[:len(v) * 16], dtype=[("xyz", "<f4", (3,)), ("rgba", "u1", (4,))])
    frec = np.frombuffer(body[len(v) * 16:], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    assert np.array_equal(vrec["xyz"], v) and np.array_equal(vrec["rgba"][:, :3], c) and (vrec["rgba"][:, 3] == 255).all()
    assert (frec["n"] == 3).all() and np.array_equal(frec["v"], f)


def test_cli_refusals(tmp_path):
    from acezero_amd import cli
    args = FC.write_room_scene(tmp_path, 3, 24, 32, 20.0)
    os.remove(tmp_path / "depth" / "frame_002.png")
    with pytest.raises(SystemExit, match="2 depth files for 3 images"):
        cli.fuse_depth_main(args)
    args = FC.write_room_scene(tmp_path, 3, 24, 32, 20.0)
    with pytest.raises(SystemExit, match="no pose above the confidence threshold"):
        cli.fuse_depth_main(args + ["--confidence_threshold", "6000"])
    with pytest.raises(SystemExit, match="more than --max_voxels 1000"):
        cli.fuse_depth_main(args + ["--max_voxels", "1000"])
    assert not (tmp_path / "mesh.ply").exists()


def test_bounds_hold_the_depth():
    from acezero_amd.fusion import bounds_from_frames
    c2w = FC.room_cameras(4)
    depths = [FC.room_depth(T, 48, 64, 40.0) for T in c2w]
    origin, dims = bounds_from_frames(depths, c2w, 40.0, 0.02, 0.08, max_depth=4.0, stride=1)
    hi = origin + (np.array(dims) - 1) * 0.02
    assert (origin <= -FC.ROOM_HALF - 0.08 + 1e-6).all() and (hi >= FC.ROOM_HALF + 0.08 - 1e-6).all()
    assert (origin >= -FC.ROOM_HALF - 0.08 - 0.021).all() and (hi <= FC.ROOM_HALF + 0.08 + 0.021).all()
    assert np.allclose(origin / 0.02, np.rint(origin / 0.02), atol=1e-4)


def test_host_tensors_are_refused():
    from acezero_amd.fusion import TSDFVolume
    with pytest.raises(RuntimeError, match="no CPU path"):
        TSDFVolume((0, 0, 0), (4, 4, 4), 0.02, 0.08, "cpu")


def test_argument_validation_without_device():
    from acezero_amd import _native as N
    lib = N.lib()
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data                                          # never dereferenced: every call below is refused before any launch
    rows = (N.TsdfFrame * 1)()
    rows[0].m[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    rows[0].focal, rows[0].ppx, rows[0].ppy, rows[0].h, rows[0].w, rows[0].offset = 40.0, 4.0, 3.0, 6, 8, 0

    def integrate(tsdf=p, depth=p, frames=rows, d_frames=p, dims=(4, 4, 4), v=0.02, tau=0.08, n_pixels=48, n_frames=1, colour=None, rgb=None):
        return lib.acez_tsdf_integrate(tsdf, p, colour, *dims, 0.0, 0.0, 0.0, v, tau, depth, rgb, n_pixels, frames, n_frames, d_frames, 0.001,
                                       4.0, 64.0, 1, None)

    def refused(rc, text):
        assert rc == -1 and text in lib.acez_last_error(), lib.acez_last_error()

    refused(integrate(tsdf=None), b"null pointer")
    refused(integrate(depth=None), b"null pointer")
    refused(integrate(frames=None), b"null pointer")
    refused(integrate(d_frames=None), b"null pointer")
    refused(integrate(rgb=p), b"colour images without a colour volume")
    refused(integrate(dims=(4, 0, 4)), b"dimensions")
    refused(integrate(dims=(2048, 2048, 2048)), b"too large")
    refused(integrate(tau=0.0), b"positive")
    refused(integrate(tau=-0.08), b"positive")
    refused(integrate(v=0.0), b"positive")
    refused(integrate(tau=float("nan")), b"non-finite")
    refused(integrate(n_frames=257), b"frame count")
    refused(integrate(n_pixels=47), b"past the end")             # 6 x 8 = 48 pixels from offset 0
    rows[0].offset = 1
    refused(integrate(), b"past the end")
    rows[0].offset = -1
    refused(integrate(), b"past the end")
    rows[0].offset, rows[0].w = 0, 0
    refused(integrate(), b"frame size")
    rows[0].w, rows[0].focal = 8, 0.0
    refused(integrate(), b"focal")
    rows[0].focal, rows[0].m[3] = 40.0, float("inf")
    refused(integrate(), b"non-finite")
    refused(lib.acez_tsdf_cells(None, p, None, 4, 4, 4, 0.0, 0.0, 0.0, 0.02, 1.0, p, None, None, None, 0, None), b"null pointer")
    refused(lib.acez_tsdf_cells(p, p, None, 4, 4, 4, 0.0, 0.0, 0.0, 0.02, 1.0, None, None, None, None, 0, None), b"null pointer")
    refused(lib.acez_tsdf_cells(p, p, None, 4, 4, 0, 0.0, 0.0, 0.0, 0.02, 1.0, p, None, None, None, 0, None), b"dimensions")
    refused(lib.acez_tsdf_cells(p, p, None, 4, 4, 4, 0.0, 0.0, 0.0, 0.0, 1.0, p, None, None, None, 0, None), b"positive")
    refused(lib.acez_tsdf_cells(p, p, None, 4, 4, 4, 0.0, 0.0, 0.0, 0.02, 1.0, p, p, None, None, 5, None), b"without a vertex buffer")
    refused(lib.acez_tsdf_faces(p, p, 4, 4, 4, 1.0, None, p, None, None, None, 0, None), b"null pointer")
    refused(lib.acez_tsdf_faces(p, p, 0, 4, 4, 1.0, p, p, None, None, None, 0, None), b"dimensions")
    refused(lib.acez_tsdf_faces(p, p, 4, 4, 4, 1.0, p, p, None, p, None, 2, None), b"without vertex ranks")
    refused(lib.acez_tsdf_faces(p, p, 4, 4, 4, 1.0, p, p, p, p, p, -2, None), b"negative")
