"""GPU: the kernels of include/acez.h section M (acez_mvs_volume, acez_mvs_aggregate, acez_mvs_select in
acezero_amd/csrc/mvs_api.hip) against their definition, bit for bit: the volume against tests/mvs_restated.cost_volume, volume ->
select against acez_mvs_sweep itself (the pin), the aggregation against tests/sgm_restated.py, and estimate_depth.py --aggregation
sgm end to end on the scene with a textureless band (tests/sgm_cases.py), chained into fuse_depth.py. Everything is integer
arithmetic or section L's float expression, so no comparison has a tolerance."""
import ctypes as C
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
from tests import sgm_cases as SC
from tests import sgm_restated as SR
from tests.test_mvs_gpu import assert_same_bits, device_frames
from tests.test_sgm_cpu import BAND_VERTICES, RANGES, SGM_MESH_BOUND, band_estimates

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR, FAR = 1.0, 3.0


@functools.lru_cache(maxsize=None)
def frames():
    """Eleven frames of smoothed noise: 0 the reference (37 x 53: no side a multiple of 16, more than one tile each way), 1 - 3
    beside it, 4 of 16 x 16 (exactly one tile), 5 - 9 of a third size and focal for eight sources, 10 of 9 x 8 for 1024 planes."""
    sizes = [(37, 53)] * 4 + [(16, 16)] + [(30, 44)] * 5 + [(9, 8)]
    focals = [50.0] * 4 + [20.0] + [40.0] * 5 + [12.0]
    eyes = [(0, 0, 0), (0.12, 0.01, 0), (-0.1, -0.02, 0.01), (0.05, 0.1, -0.02), (0.03, -0.02, 0), (0.2, 0, 0.05), (-0.2, 0.05, 0), (0.15, -0.1, 0),
            (-0.05, -0.15, 0.03), (0.3, 0, 0), (0.01, 0.01, 0)]
    targets = [(0, 0, 2), (0.05, 0, 2), (0, 0.02, 2), (0, 0, 2), (0, 0, 2), (0.05, 0, 2), (0, 0, 2), (0, 0, 2), (0, 0.05, 2), (0.9, 0, 2), (0, 0, 2)]
    return MC.random_frames(17, sizes, focals, eyes, targets)


@functools.lru_cache(maxsize=None)
def filtered_frames():
    images, rows = frames()
    return device_frames(images, rows).prefilter(), [R.prefilter(im) for im in images]


EIGHT = [1, 2, 3, 5, 6, 7, 8, 9]
VOLUMES = {                                                      # name: (reference, sources, planes, radius, keep, truncation)
    "one-source": (0, [1], 33, 2, 1, 40),
    "eight-keep-one-two-planes": (0, EIGHT, 2, 2, 1, 40),
    "eight-keep-half-radius-0": (0, EIGHT, 3, 0, 4, 40),
    "eight-keep-all-radius-4": (0, EIGHT, 65, 4, 8, 40),         # costs up to 8 * 81 * 40 = 25920
    "three-keep-two-130-planes": (0, [1, 2, 3], 130, 2, 2, 40),
    "one-tile-other-sizes": (4, [0, 5, 1], 33, 2, 2, 40),        # the 16 x 16 frame against sources of two other sizes: one call, three sizes
    "partly-out-of-view": (0, [9, 1], 33, 2, 1, 40),
    "1024-planes": (10, [0], 1024, 2, 1, 40),
    "costs-to-the-last-bit": (4, [0, 1], 3, 4, 2, 202),          # 2 * 81 * 202 = 32724 <= 32767; part of the window is outside: T each
}


def scratch_for(elements):
    from acezero_amd.mvs import SgmScratch
    sc = SgmScratch(elements, "cuda")
    sc.volume.fill_(0x5A5A), sc.s.fill_(-7)                      # stale contents must not matter
    return sc


@functools.lru_cache(maxsize=None)
def volume_case(name):
    """(the device's volume as uint16 [h,w,D], the restatement's, select's (depth, cost, plane) on C, the sweep kernel's)."""
    ref, sources, planes, radius, keep, T = VOLUMES[name]
    _, rows = frames()
    fs, g = filtered_frames()
    h, w = rows[ref].h, rows[ref].w
    Cv, n_in = R.cost_volume(g, rows, ref, sources, NEAR, FAR, planes, radius, T, keep)
    sc = scratch_for(h * w * planes + 5)
    fs.volume(ref, sources, NEAR, FAR, sc, planes, radius, T, keep)
    fs.select(ref, NEAR, FAR, sc, planes, aggregated=False)
    torch.cuda.synchronize()
    got = sc.volume.cpu().numpy().view(np.uint16)
    assert (got[h * w * planes:] == 0x5A5A).all(), "the volume kernel wrote past h * w * D elements"
    selected = [fs.frame(b, ref).copy() for b in (fs.depth, fs.cost, fs.plane)]
    fs.depth.zero_(), fs.cost.zero_(), fs.plane.zero_()
    fs.sweep(ref, sources, NEAR, FAR, planes, window=radius, truncation=T, keep=keep)
    torch.cuda.synchronize()
    swept = [fs.frame(b, ref).copy() for b in (fs.depth, fs.cost, fs.plane)]
    return got[:h * w * planes].reshape(h, w, planes), SR.pack(Cv, n_in, keep), selected, swept


@pytest.mark.parametrize("name", list(VOLUMES))
def test_volume_matches_the_restatement(name):
    got, want, _, _ = volume_case(name)
    if name == "costs-to-the-last-bit":
        assert (want & 0x7FFF).max() > 25920
    assert (want >> 15).any() and len(np.unique(want & 0x7FFF)) > 2, "the case does not exercise the volume"
    assert_same_bits(got & 0x7FFF, want & 0x7FFF, "C")
    assert_same_bits(got >> 15, want >> 15, "V")


@pytest.mark.parametrize("name", list(VOLUMES))
def test_volume_then_select_is_the_sweep(name):
    """The pin: VOLUME followed by SELECT on C equals acez_mvs_sweep's three outputs bit for bit."""
    _, _, selected, swept = volume_case(name)
    for a, b, what in zip(selected, swept, ("depth", "winning cost", "winning plane")):
        assert_same_bits(a, b, what)


AGGREGATES = {                                                   # name: (h, w, planes, P1, P2, largest cost)
    "one-pixel": (1, 1, 2, 3, 20, 500),
    "one-row": (1, 70, 64, 5, 40, 500),
    "one-column-equal-penalties": (70, 1, 65, 5, 5, 500),
    "two-planes": (37, 53, 2, 3, 20, 60),
    "64-planes": (37, 53, 64, 7, 100, 2000),
    "130-planes": (37, 53, 130, 80, 640, 2000),
    "300-planes": (9, 8, 300, 80, 640, 2000),                     # eight planes per lane; with 2, 64, 65, 130 and 1024 every instantiation runs
    "1024-planes": (9, 8, 1024, 80, 640, 2000),
    "bound-on-s": (37, 53, 65, 32767, 32767, 32767),             # costs at the storage's maximum, penalties at theirs
}


def aggregate(sc, h, w, planes, paths, direction, p1, p2):
    from acezero_amd import _native as N_
    from acezero_amd.head import _ptr, _stream
    n = h * w * planes
    sc.s[:n].zero_()
    N_.check(N_.lib().acez_mvs_aggregate(_ptr(sc.volume), _ptr(sc.s), sc.elements, h, w, planes, paths, direction, p1, p2, _stream()))
    torch.cuda.synchronize()
    got = sc.s.cpu().numpy()
    assert (got[n:] == -7).all(), "the aggregation wrote past h * w * D elements"
    return got[:n].reshape(h, w, planes).astype(np.int64)


@pytest.mark.parametrize("name", list(AGGREGATES))
def test_aggregate_matches_the_restatement(name):
    """Each direction alone, then four and eight paths; the last one twice, into a re-zeroed S."""
    h, w, planes, p1, p2, top = AGGREGATES[name]
    rng = np.random.default_rng(len(name) + planes)
    Cv = rng.integers(0, top + 1, (planes, h, w)).astype(np.int32)
    if name == "bound-on-s":
        Cv[rng.random(Cv.shape) < 0.9] = 32767
    sc = scratch_for(h * w * planes + 5)
    packed = SR.pack(Cv, rng.integers(0, 2, Cv.shape), 1)        # V is set at random: the aggregation ignores bit 15
    sc.volume[:h * w * planes].copy_(torch.from_numpy(packed.reshape(-1).view(np.int16)))
    single = [SR.path(Cv, r, p1, p2) for r in range(1, 9)]
    for r in range(1, 9):
        got = aggregate(sc, h, w, planes, 8, r, p1, p2)
        assert np.array_equal(got, single[r - 1].transpose(1, 2, 0)), f"direction {r}: {int((got != single[r - 1].transpose(1, 2, 0)).sum())} differ"
        if r <= 4:
            assert np.array_equal(aggregate(sc, h, w, planes, 4, r, p1, p2), got)
    for paths in (4, 8):
        got = aggregate(sc, h, w, planes, paths, 0, p1, p2)
        assert np.array_equal(got, SR.aggregate(Cv, paths, p1, p2).transpose(1, 2, 0)), f"{paths} paths"
    assert np.array_equal(aggregate(sc, h, w, planes, 8, 0, p1, p2), got), "two runs into a zeroed S differ"
    if name == "bound-on-s":
        assert got.max() == 8 * (32767 + 32767), "the case does not reach the stated bound on S"
    assert_same_bits(sc.volume.cpu().numpy()[:h * w * planes].view(np.uint16), packed.reshape(-1), "the volume after the aggregation")


def test_select_on_aggregated_costs_matches_the_restatement():
    """volume -> aggregate -> select of a middle frame of the band scene, four and eight paths: depth, S(k*) and k* as float32 and
    int32, before the check quantises anything."""
    (images, _, _, rows, _), sources, _, _ = band_estimates()
    fs = device_frames(images, rows).prefilter()
    g = [R.prefilter(im) for im in images]
    ref = 2
    sc = scratch_for(MC.H * MC.W * SC.PLANES)
    for paths, p1, p2 in ((4, 80, 640), (8, 30, 30)):
        want = SR.sweep(g, rows, ref, sources[ref], MC.Z_NEAR, MC.Z_FAR, SC.PLANES, SC.WINDOW, 40, SC.KEEP, 5, paths, p1, p2)
        assert (want[0] > 0).mean() > 0.5 and len(np.unique(want[2])) > 10
        fs.volume(ref, sources[ref], MC.Z_NEAR, MC.Z_FAR, sc, SC.PLANES, SC.WINDOW, 40, SC.KEEP)
        fs.aggregate(ref, sc, SC.PLANES, paths, p1, p2).select(ref, MC.Z_NEAR, MC.Z_FAR, sc, SC.PLANES)
        torch.cuda.synchronize()
        assert_same_bits(fs.frame(fs.plane, ref), want[2], "winning plane")
        assert_same_bits(fs.frame(fs.cost, ref), want[1], "winning cost")
        assert_same_bits(fs.frame(fs.depth, ref), want[0], "depth")


def test_band_scene_maps_match_the_restated_chain():
    from acezero_amd.mvs import estimate_depth_maps
    (images, _, _, rows, _), sources, plain, sgm = band_estimates()
    w2c = np.stack([np.concatenate([r.m.reshape(3, 4).astype(np.float64), [[0, 0, 0, 1]]]) for r in rows])
    info = {}
    maps = estimate_depth_maps(torch.from_numpy(np.stack(images)).cuda(), world_to_cam=w2c, focals=MC.FOCAL, sources=sources, ranges=RANGES,
                               planes=SC.PLANES, aggregation="sgm", info=info)
    for f in range(SC.N):
        assert_same_bits(maps[f], sgm[f], f"aggregation sgm, frame {f}")
    assert info["sgm_scratch_bytes"] == 4 * 6 * MC.H * MC.W * SC.PLANES
    maps = estimate_depth_maps(torch.from_numpy(np.stack(images)).cuda(), world_to_cam=w2c, focals=MC.FOCAL, sources=sources, ranges=RANGES,
                               planes=SC.PLANES, aggregation=None)
    for f in range(SC.N):
        assert_same_bits(maps[f], plain[f], f"no aggregation, frame {f}")
    eight = estimate_depth_maps(images, world_to_cam=w2c, focals=MC.FOCAL, sources=sources, ranges=RANGES, planes=SC.PLANES, aggregation="sgm",
                                sgm_paths=8, sgm_p1=40, sgm_p2=320)
    want, _ = SR.estimate(images, rows, sources, RANGES, SC.PLANES, paths=8, p1=40, p2=320)
    for f in range(SC.N):
        assert_same_bits(eight[f], want[f], f"eight paths, frame {f}")


def test_estimate_with_aggregation_then_fuse_end_to_end(tmp_path):
    """estimate_depth.py --aggregation sgm writes the restated chain's maps, --aggregation none what no flag writes, and fuse_depth.py
    makes a mesh of each. (The script runs once as a process; the other runs call the mains the two scripts are stubs of.) Measured on
    the CPU with tests/tsdf_restated.py (tests/test_sgm_cpu.py::test_fused_mesh_fills_the_band): 194 vertices inside the band region
    from the plain maps, 2026 from the aggregated ones, 10.44 times as many, and the aggregated mesh's farthest vertex 59.03 mm from
    a plane of the scene. Asserted: at least 3 + (10.44 - 3) / 2 = 6.72 times as many (the required third, with the measured margin
    halved), and the farthest vertex within 1.25 x 59.03 mm."""
    from PIL import Image
    from acezero_amd import cli, mvs
    from acezero_amd.fusion import _w2c34
    from tests.fusion_cases import read_mesh_ply
    from tests.test_mvs_cpu import plane_distance
    pose_file, pattern = SC.write_scene(str(tmp_path))
    options = ["--image_resolution", MC.H, "--depth_range", MC.Z_NEAR, MC.Z_FAR, "--planes", SC.PLANES, "--sources", SC.SOURCES]
    args = lambda folder, *extra: [str(a) for a in [pose_file, pattern, tmp_path / folder] + options + list(extra)]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "estimate_depth.py")] + args("sgm", "--aggregation", "sgm"), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Aggregation: sgm, 4 paths, P1 / P2 = 80 / 640" in r.stderr and "scratch" in r.stderr
    assert f"Estimated {SC.N} of {SC.N} depth maps" in r.stderr
    assert cli.estimate_depth_main(args("none", "--aggregation", "none")) == 0
    assert cli.estimate_depth_main(args("plain")) == 0
    # the restatement on what the tool read: the decoded frames, the pose file's poses and focal, select_sources' neighbours
    files = sorted(glob.glob(pattern))
    grey, _ = mvs.load_grey_frames(files, MC.H)
    _, c2w, focals = cli.read_ace_pose_file(pose_file, 1000)
    w2c = _w2c34(None, c2w, SC.N)
    rows = [R.Row(w2c[k], focals[k], MC.W / 2.0, MC.H / 2.0, MC.H, MC.W) for k in range(SC.N)]
    sources = mvs.select_sources(c2w, focals, [(MC.H, MC.W)] * SC.N, np.sqrt(MC.Z_NEAR * MC.Z_FAR), SC.SOURCES)
    assert all(len(s) == SC.SOURCES for s in sources)
    g = [R.prefilter(im) for im in grey]
    plain, sgm = [], []
    for f in range(SC.N):                                        # one cost volume per frame serves both chains
        Cv, n_in = R.cost_volume(g, rows, f, sources[f], MC.Z_NEAR, MC.Z_FAR, SC.PLANES, SC.WINDOW, 40, SC.KEEP)
        plain.append(SR.select(Cv, n_in >= SC.KEEP, MC.Z_NEAR, MC.Z_FAR)[0])
        sgm.append(SR.select(SR.aggregate(Cv, 4, 80, 640), n_in >= SC.KEEP, MC.Z_NEAR, MC.Z_FAR)[0])
    want = {"sgm": [R.check(sgm, rows, f, sources[f]) for f in range(SC.N)], "plain": [R.check(plain, rows, f, sources[f]) for f in range(SC.N)]}
    want["none"] = want["plain"]
    names = [os.path.splitext(os.path.basename(f))[0] + ".png" for f in files]
    for folder in ("sgm", "none", "plain"):
        assert sorted(os.listdir(tmp_path / folder)) == names
        for k, name in enumerate(names):
            got = np.asarray(Image.open(tmp_path / folder / name))
            assert got.dtype == np.uint16
            assert_same_bits(got, want[folder][k], f"{folder}: depth map {k}")
    inside = {}
    for folder in ("plain", "sgm"):
        mesh = str(tmp_path / f"{folder}.ply")
        assert cli.fuse_depth_main([pose_file, pattern, mesh, "--depth_files", str(tmp_path / folder / "*.png")]) == 0
        v, _, f = read_mesh_ply(mesh)
        inside[folder] = int(SC.in_band_region(v).sum())
        print(f"{folder}: {len(v)} vertices, {len(f)} faces, {inside[folder]} inside the band region, farthest {plane_distance(v).max() * 1000:.2f} mm")
        if folder == "sgm":
            assert plane_distance(v).max() <= SGM_MESH_BOUND
    assert BAND_VERTICES == dict(plain=194, sgm=2026)            # the docstring's figures
    assert inside["sgm"] >= 6.72 * inside["plain"] and inside["sgm"] > 0


def test_refusals_launch_nothing():
    """Outputs pre-filled with a pattern stay untouched by every refused call."""
    from acezero_amd import _native as N_
    from acezero_amd.head import _ptr
    lib = N_.lib()
    images, rows = frames()
    fs = device_frames(images[:3], rows[:3]).prefilter()
    h, w, planes = rows[0].h, rows[0].w, 9
    n = h * w * planes
    sc = scratch_for(n)
    fs.depth.fill_(-3.0), fs.cost.fill_(-3), fs.plane.fill_(-3)
    src = (C.c_int32 * 2)(1, 2)

    def volume(planes=planes, radius=2, T=40, keep=1, vol=sc.volume, n_volume=n, ref=0):
        return lib.acez_mvs_volume(_ptr(fs.filtered), fs.n_pixels, fs.rows, 3, ref, src, 2, 1.0, 3.0, planes, radius, T, keep, _ptr(vol) if vol is not None else None,
                                   n_volume, None)

    def aggregate(vol=sc.volume, s=sc.s, n_volume=n, paths=4, direction=0, p1=10, p2=80):
        return lib.acez_mvs_aggregate(_ptr(vol) if vol is not None else None, _ptr(s) if s is not None else None, n_volume, h, w, planes, paths,
                                      direction, p1, p2, None)

    def select(vol=sc.volume, n_volume=n, planes=planes, q=5, depth=fs.depth, near=1.0):
        return lib.acez_mvs_select(_ptr(vol) if vol is not None else None, _ptr(sc.s), n_volume, fs.n_pixels, fs.rows, 3, 0, near, 3.0, planes, q,
                                   _ptr(depth) if depth is not None else None, _ptr(fs.cost), _ptr(fs.plane), None)

    refusals = [volume(vol=None), volume(n_volume=n - 1), volume(planes=1), volume(keep=3), volume(ref=3), volume(radius=4, T=203, keep=2),
                aggregate(vol=None), aggregate(s=None), aggregate(n_volume=n - 1), aggregate(paths=6), aggregate(paths=0), aggregate(direction=5),
                aggregate(p1=0), aggregate(p1=81), aggregate(p2=32768),
                select(vol=None), select(depth=None), select(n_volume=n - 1), select(planes=1025), select(q=101), select(near=3.0)]
    assert refusals == [-1] * len(refusals)
    with pytest.raises(ValueError, match="sgm_paths"):
        fs.sweep_frames([(0, [1, 2], 1.0, 3.0, 1)], planes, aggregation="sgm", sgm_paths=5)
    torch.cuda.synchronize()
    assert (sc.volume.cpu().numpy().view(np.uint16) == 0x5A5A).all()
    assert (sc.s == -7).all()
    assert (fs.depth == -3.0).all() and (fs.cost == -3).all() and (fs.plane == -3).all()
    assert volume() == 0 and aggregate() == 0 and select() == 0  # the same calls with valid arguments run
    torch.cuda.synchronize()
    assert (fs.frame(fs.depth, 0) >= 0).all() and (sc.volume.cpu().numpy().view(np.uint16) != 0x5A5A).any()
