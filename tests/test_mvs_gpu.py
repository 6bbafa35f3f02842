"""GPU: the stereo kernels of acezero_amd/csrc/mvs_api.hip against the numpy restatement of their definition (tests/mvs_restated.py,
itself checked in tests/test_mvs_cpu.py), bit for bit: depth, winning cost, winning plane and the uint16 output; estimate_depth.py and
fuse_depth.py end to end."""
import functools
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mvs_cases as MC
from tests import mvs_restated as R
from tests.test_mvs_cpu import MESH_BOUND, N, plane_distance, scene_estimate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR, FAR = 1.0, 3.0


@functools.lru_cache(maxsize=None)
def frames():
    """Ten frames of smoothed noise: 0 the reference (61 x 83: no side a multiple of 16), 1-3 beside it, 4 of another size and focal,
    5 turned so far that it sees part of what the reference sees, 6 beyond the swept depths looking the same way (the reference's
    points are behind it), 7-9 further frames of a third size for the sweep with eight sources."""
    sizes = [(61, 83)] * 4 + [(48, 70), (61, 83), (61, 83)] + [(35, 53)] * 3
    focals = [70.0, 70.0, 70.0, 70.0, 55.0, 70.0, 70.0, 40.0, 40.0, 40.0]
    eyes = [(0, 0, 0), (0.12, 0.01, 0), (-0.1, -0.02, 0.01), (0.05, 0.1, -0.02), (0.2, 0, 0.05), (0.3, 0, 0), (0.02, 0, 3.5), (-0.2, 0.05, 0),
            (0.15, -0.1, 0), (-0.05, -0.15, 0.03)]
    targets = [(0, 0, 2), (0.05, 0, 2), (0, 0.02, 2), (0, 0, 2), (0.05, 0, 2), (1.3, 0, 2), (0.02, 0, 6), (0, 0, 2), (0, 0, 2), (0, 0.05, 2)]
    return MC.random_frames(11, sizes, focals, eyes, targets)


def device_frames(images, rows):
    from acezero_amd.mvs import StereoFrames
    w2c = np.stack([np.concatenate([r.m.reshape(3, 4).astype(np.float64), [[0, 0, 0, 1]]]) for r in rows])
    fs = StereoFrames(images, world_to_cam=w2c, focals=[float(r.focal) for r in rows], ppx=[float(r.ppx) for r in rows],
                      ppy=[float(r.ppy) for r in rows])
    for k, r in enumerate(rows):                                 # the table holds the restatement's float32 numbers
        assert np.array_equal(np.array(fs.rows[k].m[:], np.float32), r.m) and fs.rows[k].focal == r.focal and fs.rows[k].ppx == r.ppx
    return fs


def assert_same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    raw = {4: np.uint32, 2: np.uint16, 1: np.uint8}[got.dtype.itemsize]
    diff = got.view(raw) != want.view(raw)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} pixels differ, first at {np.argwhere(diff)[0]}: {got[diff][0]} != {want[diff][0]}"


def test_prefilter_matches_the_restatement():
    images, rows = frames()
    rng = np.random.default_rng(5)
    images = list(images)
    images[1] = np.where(rng.random(images[1].shape) < 0.5, 0, 255).astype(np.uint8)             # the extremes, pixel by pixel
    images[2] = np.where((np.add.outer(np.arange(61) // 7, np.arange(83) // 5) % 2) == 0, 0, 255).astype(np.uint8)   # ... and in blocks
    images[3] = np.full_like(images[3], 255)
    fs = device_frames(images, rows).prefilter()
    want = [R.prefilter(im) for im in images]
    assert want[2].min() == 0 and want[2].max() == 255 and (want[3] == 128).all()
    for k in range(len(images)):
        assert_same_bits(fs.frame(fs.filtered, k), want[k], f"frame {k}")


SWEEPS = {                                                       # name: (sources, planes, radius, keep)
    "one-source": ([1], 33, 2, 1),
    "three-keep-two": ([1, 2, 3], 33, 2, 2),
    "eight-sources": ([1, 2, 3, 4, 5, 7, 8, 9], 17, 2, 4),
    "two-planes": ([1, 2, 3], 2, 2, 2),
    "radius-0": ([1, 2, 3], 33, 0, 2),
    "radius-4": ([1, 2, 3], 17, 4, 2),
    "other-size-and-focal": ([4, 7, 1], 33, 2, 2),
    "partly-out-of-view": ([5, 1], 33, 2, 1),
    "behind-the-source": ([6, 1], 33, 2, 1),
    "behind-the-source-keep-all": ([6, 1], 17, 2, 2),
}


@functools.lru_cache(maxsize=None)
def filtered_frames():
    images, rows = frames()
    return device_frames(images, rows).prefilter(), [R.prefilter(im) for im in images]


@pytest.mark.parametrize("name", list(SWEEPS))
def test_sweep_matches_the_restatement(name):
    sources, planes, radius, keep = SWEEPS[name]
    _, rows = frames()
    fs, g = filtered_frames()
    depth, cost, plane = R.sweep(g, rows, 0, sources, NEAR, FAR, planes, radius=radius, keep=keep)
    if name == "behind-the-source-keep-all":
        assert (depth == 0).all()                                # frame 6 never has the pixel in view: fewer than `keep` sources do
    elif name == "two-planes":
        assert set(np.unique(plane)) == {0, 1}
    else:
        assert (depth > 0).mean() > 0.02 and len(np.unique(plane)) > planes // 2, "the case does not exercise the sweep"
    fs.sweep(0, sources, NEAR, FAR, planes, window=radius, keep=keep)
    torch.cuda.synchronize()
    assert_same_bits(fs.frame(fs.plane, 0), plane, "winning plane")
    assert_same_bits(fs.frame(fs.cost, 0), cost, "winning cost")
    assert_same_bits(fs.frame(fs.depth, 0), depth, "depth")


def test_reference_of_another_size():
    """The small frame 7 as the reference of larger sources; its tile grid is 3 x 4 with a ragged edge."""
    _, rows = frames()
    fs, g = filtered_frames()
    depth, cost, plane = R.sweep(g, rows, 7, [0, 8, 4], NEAR, FAR, 33, keep=2)
    assert (depth > 0).mean() > 0.05
    fs.sweep(7, [0, 8, 4], NEAR, FAR, 33, keep=2)
    torch.cuda.synchronize()
    assert_same_bits(fs.frame(fs.plane, 7), plane, "winning plane")
    assert_same_bits(fs.frame(fs.cost, 7), cost, "winning cost")
    assert_same_bits(fs.frame(fs.depth, 7), depth, "depth")


def test_constant_images_give_nothing():
    """Wide-angle sources that see every window of the reference on every plane: all costs of a pixel tie (at 0, or at the part of its
    window outside the reference frame, the same on every plane), the first plane wins everywhere and nothing is kept: plane 0 is an
    end plane, and 0 against 0 is not unique. (Where a source's edge of view moves through a window from plane to plane, the
    out-of-view cost T does break the tie; this geometry has no such pixel.)"""
    from tests.fusion_cases import look_at
    eyes = [(0, 0, 0), (0.1, 0.01, 0), (-0.08, -0.02, 0.01), (0.03, 0.09, -0.02)]
    rows = [R.Row(np.linalg.inv(look_at(e, (e[0], e[1], 2.0))), 70.0 if k == 0 else 45.0, 41.8, 30.3, 61, 83) for k, e in enumerate(eyes)]
    flat = [np.full((61, 83), 90 + 40 * k, np.uint8) for k in range(4)]
    fs = device_frames(flat, rows).prefilter()
    g = [R.prefilter(im) for im in flat]
    assert all((x == 128).all() for x in g)
    depth, cost, plane = R.sweep(g, rows, 0, [1, 2, 3], NEAR, FAR, 33, keep=2)
    assert (depth == 0).all() and (plane == 0).all() and (cost[2:-2, 2:-2] == 0).all() and (cost[0] > 0).all()
    fs.sweep(0, [1, 2, 3], NEAR, FAR, 33, keep=2)
    torch.cuda.synchronize()
    assert_same_bits(fs.frame(fs.plane, 0), plane, "winning plane")
    assert_same_bits(fs.frame(fs.cost, 0), cost, "winning cost")
    assert_same_bits(fs.frame(fs.depth, 0), depth, "depth")
    assert not fs.frame(fs.depth, 0).any()


def test_scene_matches_the_restatement():
    """The analytic scene, every frame: the sweep's depth and the checked uint16 maps are the restatement's."""
    from acezero_amd.mvs import estimate_depth_maps
    images, _, _, rows, sources, out, depths = scene_estimate()
    fs = device_frames(images, rows).prefilter()
    for f in range(N):
        fs.sweep(f, sources[f], MC.Z_NEAR, MC.Z_FAR, MC.PLANES)
    for f in range(N):
        fs.check(f, sources[f])
    torch.cuda.synchronize()
    for f in range(N):
        assert_same_bits(fs.frame(fs.depth, f), depths[f], f"depth of frame {f}")
        assert_same_bits(fs.frame(fs.out, f), out[f], f"uint16 map of frame {f}")
    w2c = np.stack([np.concatenate([r.m.reshape(3, 4).astype(np.float64), [[0, 0, 0, 1]]]) for r in rows])
    maps = estimate_depth_maps(torch.from_numpy(np.stack(images)).cuda(), world_to_cam=w2c, focals=MC.FOCAL, sources=sources,
                               ranges=[(MC.Z_NEAR, MC.Z_FAR)] * N, planes=MC.PLANES)
    for f in range(N):
        assert_same_bits(maps[f], out[f], f"estimate_depth_maps, frame {f}")


def check_case(depth_maps, rows, sources, **kw):
    fs = device_frames([np.zeros((r.h, r.w), np.uint8) for r in rows], rows)
    fs.depth.copy_(torch.from_numpy(np.concatenate([d.reshape(-1) for d in depth_maps])))
    fs.check(0, sources, **kw)
    torch.cuda.synchronize()
    want = R.check(depth_maps, rows, 0, sources, **kw)
    assert_same_bits(fs.frame(fs.out, 0), want, "uint16 map")
    return want


def test_check_on_and_beyond_the_tolerance():
    """Two cameras at one place: a pixel of the reference at 2 m meets the same pixel of the source at zc = 2. Column x of the source
    holds the float (x - 16) places away from 2 + tolerance * 2, so that agreement ends exactly at one column."""
    rows = [R.Row(np.eye(4), 40.0, 16.0, 12.0, 24, 32), R.Row(np.eye(4), 40.0, 16.0, 12.0, 24, 32)]
    ref = np.full((24, 32), 2.0, np.float32)
    for tol in (0.01, 0.25):
        edge = np.float32(2.0) + np.float32(tol) * np.float32(2.0)
        column = np.array([edge], np.float32).view(np.int32)[0] + (np.arange(32, dtype=np.int32) - 16)
        src = np.tile(column.view(np.float32), (24, 1))
        want = check_case([ref, src], rows, [1], tolerance=tol, min_consistent=1)
        kept = want[12] > 0
        assert kept[:14].all() and not kept[19:].any() and (want[12][kept] == 2000).all()
        last = int(kept.nonzero()[0].max())
        assert 14 <= last <= 18 and kept[:last + 1].all(), "agreement must end once, within two places of the computed edge"
    both = check_case([ref, -ref], rows, [1], min_consistent=0)                                   # nothing to agree with, nothing needed
    assert (both == 2000).all()


def test_check_millimetres_at_the_end_of_uint16():
    rows = [R.Row(np.eye(4), 40.0, 16.0, 12.0, 24, 32), R.Row(np.eye(4), 40.0, 16.0, 12.0, 24, 32)]
    ref = np.tile(np.linspace(65.53, 65.54, 32).astype(np.float32), (24, 1))
    ref[0, :4] = [65.535, 65.536, 65.5354, 65.5356]
    want = check_case([ref, ref.copy()], rows, [1])
    assert (want == 65535).any() and (want[1:, 20:] == 0).all() and (want[1:, :15] >= 65530).all()
    assert want[0, 0] == 65535 and want[0, 1] == 0 and want[0, 2] == 65535 and want[0, 3] == 0
    other_unit = check_case([ref, ref.copy()], rows, [1], depth_unit=0.002)
    assert (other_unit > 32760).all()


def test_argument_validation_with_device_buffers():
    from acezero_amd import _native as N_
    from acezero_amd.head import _ptr
    import ctypes as C
    lib = N_.lib()
    images, rows = frames()
    fs = device_frames(images[:3], rows[:3]).prefilter()
    src = (C.c_int32 * 2)(1, 2)

    def call(ref=0, n_pixels=fs.n_pixels, planes=9, keep=1, depth=fs.depth):
        return lib.acez_mvs_sweep(_ptr(fs.filtered), n_pixels, fs.rows, 3, ref, src, 2, 1.0, 3.0, planes, 2, 40, keep, 5, _ptr(depth), None, None, None)

    assert call() == 0                                           # without the optional outputs
    torch.cuda.synchronize()
    assert call(n_pixels=fs.n_pixels - 1) == -1 and b"past the end" in lib.acez_last_error()
    assert call(ref=3) == -1 and call(planes=1) == -1 and call(keep=3) == -1 and call(depth=None) == -1
    with pytest.raises(N_.AcezError, match="ACEZ_ERR_INVALID"):
        fs.sweep(0, [1, 2], 3.0, 1.0)
    with pytest.raises(N_.AcezError, match="ACEZ_ERR_INVALID"):
        fs.check(0, [1, 5])
    torch.cuda.synchronize()                                     # nothing was launched by the refused calls; the device is fine


def test_estimate_then_fuse_end_to_end(tmp_path):
    from acezero_amd import cli, mvs
    from acezero_amd.fusion import _w2c34
    from tests.fusion_cases import read_mesh_ply
    pose_file, pattern = MC.write_scene(str(tmp_path), N)
    out_dir = tmp_path / "depth"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "estimate_depth.py"), pose_file, pattern, str(out_dir), "--image_resolution", str(MC.H),
                        "--depth_range", str(MC.Z_NEAR), str(MC.Z_FAR), "--planes", str(MC.PLANES), "--sources", str(MC.SOURCES)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert f"Estimated {N} of {N} depth maps" in r.stderr
    # the restatement on what the tool read: the decoded frames, the pose file's poses and focal, select_sources' neighbours
    files = sorted(glob.glob(pattern))
    grey, heights = mvs.load_grey_frames(files, MC.H)
    names, c2w, focals = cli.read_ace_pose_file(pose_file, 1000)
    assert [os.path.basename(n) for n in names] == [os.path.basename(f) for f in files] and heights == [MC.H] * N
    w2c = _w2c34(None, c2w, N)
    rows = [R.Row(w2c[k], focals[k], MC.W / 2.0, MC.H / 2.0, MC.H, MC.W) for k in range(N)]
    sources = mvs.select_sources(c2w, focals, [(MC.H, MC.W)] * N, np.sqrt(MC.Z_NEAR * MC.Z_FAR), MC.SOURCES)
    want, _ = R.estimate(grey, rows, sources, [(MC.Z_NEAR, MC.Z_FAR)] * N, MC.PLANES)
    from PIL import Image
    written = sorted(glob.glob(str(out_dir / "*.png")))
    assert [os.path.basename(p) for p in written] == [os.path.basename(f) for f in files]
    for k, path in enumerate(written):
        got = np.asarray(Image.open(path))
        assert got.dtype == np.uint16
        assert_same_bits(got, want[k], f"depth map {k}")
    mesh = str(tmp_path / "mesh.ply")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fuse_depth.py"), pose_file, pattern, mesh, "--depth_files", str(out_dir / "*.png")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    v, _, f = read_mesh_ply(mesh)
    dist = plane_distance(v)
    print(f"{len(v)} vertices, {len(f)} faces, largest distance to a plane of the scene {dist.max() * 1000:.2f} mm")
    assert len(v) > 5000 and len(f) > 10000
    assert dist.max() <= MESH_BOUND
