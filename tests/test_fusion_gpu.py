"""GPU: the TSDF kernels of acezero_amd/csrc/fusion_api.hip against the numpy restatement of their definition
(tests/tsdf_restated.py, itself checked in tests/test_fusion_cpu.py), bit for bit; the entry points' argument checks with device
buffers; fuse_depth.py end to end."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import fusion_cases as FC
from tests import tsdf_restated as R
from tests.test_fusion_cpu import DISTANCE_BOUND, sphere_volume

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# no dimension is a multiple of the 32 x 4 x 2 brick
MIXED = dict(origin=(-0.36, -0.28, -0.2), dims=(37, 29, 21), voxel_size=0.02, truncation=0.08, max_weight=3.0)
MAX_DEPTH = 4.0


@functools.lru_cache(maxsize=None)
def mixed_frames():
    """5 frames of mixed sizes around the MIXED volume (centre (0, 0, 0)): two outside it that see all of it, one INSIDE it (voxels
    behind the camera), one far away with a long lens that sees one corner only, one without any depth. 30 % holes, some values beyond
    MAX_DEPTH; the depth is a rough shell around the volume's centre, so that the truncation band, free space and the far side occur."""
    rng = np.random.default_rng(7)
    eyes = [(0.05, -0.03, -1.0), (1.1, 0.1, 0.05), (0.1, 0.05, -0.02), (2.6, 2.0, 1.5), (0.0, 0.0, -1.2)]
    targets = [(0, 0, 0), (0, 0, 0), (1.0, 0.6, 0.5), (0.3, 0.22, 0.15), (0, 0, 0)]
    sizes = [(60, 80), (80, 60), (60, 80), (80, 60), (60, 80)]
    focals = [70.0, 65.0, 40.0, 900.0, 70.0]
    c2w = np.stack([FC.look_at(e, t) for e, t in zip(eyes, targets)])
    depths, rgbs = [], []
    bases = [1.25, 1.5, 0.5, 3.2, 1.2]                            # metres: about each camera's distance to what it looks at
    for k, ((h, w), base) in enumerate(zip(sizes, bases)):
        d = (base + rng.uniform(-0.2, 0.2, (h, w))) * 1000.0
        d[rng.random((h, w)) < 0.05] = 1000.0 * MAX_DEPTH + rng.uniform(1, 2000)
        d[rng.random((h, w)) < 0.30] = 0
        if k == 4:
            d[:] = 0
        depths.append(d.astype(np.uint16))
        rgbs.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    ppx = [w / 2.0 + 0.3 for _, w in sizes]
    ppy = [h / 2.0 - 0.2 for h, _ in sizes]
    return depths, rgbs, np.linalg.inv(c2w), focals, ppx, ppy


@functools.lru_cache(maxsize=None)
def mixed_reference(colour):
    depths, rgbs, w2c, focals, ppx, ppy = mixed_frames()
    vol = R.integrate(R.Volume(**MIXED), depths, w2c, focals, ppx, ppy, rgbs if colour else None, max_depth=MAX_DEPTH)
    # what the case is for
    x, y, z = vol.centres()
    zc2 = (w2c[2, 2, 0] * x[None, None, :] + w2c[2, 2, 1] * y[None, :, None]) + w2c[2, 2, 2] * z[:, None, None] + w2c[2, 2, 3]
    assert (zc2 <= 0).sum() > 1000 and (zc2 > 0).sum() > 1000, "the third camera is not inside the volume"
    uncapped = R.integrate(R.Volume(**dict(MIXED, max_weight=64.0)), depths, w2c, focals, ppx, ppy, None, max_depth=MAX_DEPTH)
    assert vol.weight.max() == 3.0 and (uncapped.weight == 4.0).sum() > 50, "the weight cap does not bind"
    assert (vol.weight == 0).sum() > 100 and (vol.weight == 1.0).sum() > 100
    return vol


def device_volume(spec):
    from acezero_amd.fusion import TSDFVolume
    return TSDFVolume(spec["origin"], spec["dims"], spec["voxel_size"], spec["truncation"], "cuda", max_weight=spec.get("max_weight", 64.0))


def integrate_mixed(colour, chunks=((0, 5),), **kw):
    depths, rgbs, w2c, focals, ppx, ppy = mixed_frames()
    vol = device_volume(MIXED)
    for lo, hi in chunks:
        vol.integrate(depths[lo:hi], world_to_cam=w2c[lo:hi], focals=focals[lo:hi], ppx=ppx[lo:hi], ppy=ppy[lo:hi],
                      rgb=rgbs[lo:hi] if colour else None, max_depth=MAX_DEPTH, **kw)
    torch.cuda.synchronize()
    return vol


def assert_same_volume(vol, ref):
    for name in ("tsdf", "weight", "colour"):
        got, want = getattr(vol, name).cpu().numpy(), getattr(ref, name)
        diff = got.view(np.uint32) != want.view(np.uint32)
        assert not diff.any(), f"{name}: {int(diff.sum())} of {diff.size} voxels differ, first at {np.argwhere(diff)[0]}"


@pytest.mark.parametrize("colour", [True, False])
def test_integrate_matches_the_restatement(colour):
    ref = mixed_reference(colour)
    assert_same_volume(integrate_mixed(colour), ref)
    assert_same_volume(integrate_mixed(colour, chunks=((0, 2), (2, 4), (4, 5))), ref)          # the caller's chunks
    assert_same_volume(integrate_mixed(colour, frames_per_call=2), ref)                         # integrate()'s own chunks


def test_frustum_skip_is_conservative():
    """The long-lens camera misses most bricks and the inside camera has bricks behind it: with the skip (the default, compared with
    the restatement, which has none, above) and without it the volumes are the same bits."""
    depths, _, w2c, focals, ppx, ppy = mixed_frames()
    x, y, z = R.Volume(**MIXED).centres()
    m = w2c[3].astype(np.float64)
    p = np.stack(np.broadcast_arrays(x[None, None, :], y[None, :, None], z[:, None, None]), -1).astype(np.float64)
    cam = p @ m[:3, :3].T + m[:3, 3]
    u, v = focals[3] * cam[..., 0] / cam[..., 2] + ppx[3], focals[3] * cam[..., 1] / cam[..., 2] + ppy[3]
    h, w = depths[3].shape
    seen = (u >= -0.5) & (u < w - 0.5) & (v >= -0.5) & (v < h - 0.5)
    assert 0.01 < seen.mean() < 0.4, "the long lens should see a small part of the volume"
    ref = mixed_reference(True)
    assert_same_volume(integrate_mixed(True, frustum_skip=True), ref)
    assert_same_volume(integrate_mixed(True, frustum_skip=False), ref)


def upload(vol, tsdf, weight, colour=None):
    vol.tsdf.copy_(torch.from_numpy(np.ascontiguousarray(tsdf)))
    vol.weight.copy_(torch.from_numpy(np.ascontiguousarray(weight)))
    if colour is not None:
        vol.colour.copy_(torch.from_numpy(np.ascontiguousarray(colour)))
    return vol


def assert_same_mesh(got, want):
    gv, gc, gf = (t.cpu().numpy() for t in got)
    wv, wc, wf = want
    assert gf.shape == wf.shape and np.array_equal(gf, wf)
    assert gv.shape == wv.shape and np.array_equal(gv.view(np.uint32), wv.view(np.uint32))
    assert np.array_equal(gc, wc)


@pytest.mark.parametrize("slab", [False, True])
def test_extraction_matches_the_restatement(slab):
    ref = sphere_volume()
    tsdf, weight = ref.tsdf.copy(), ref.weight.copy()
    colour = np.random.default_rng(3).uniform(0, 255, (3,) + tsdf.shape).astype(np.float32)
    if slab:
        weight[:, 19:22, :] = 0                                  # an unknown slab through the sphere: the mesh has a boundary there
    want = R.extract(tsdf, weight, colour, ref.origin, ref.v, 1.0)
    assert len(want[0]) > 1000 and len(want[2]) > 2000
    if slab:
        assert (FC.mesh_edge_counts(want[2])[0] == 1).any()
    vol = upload(device_volume(FC.SPHERE_VOLUME), tsdf, weight, colour)
    first, second = vol.extract_mesh(1.0), vol.extract_mesh(1.0)
    assert_same_mesh(first, want)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_sphere_fused_on_the_device_is_the_restatements_sphere():
    depths, c2w, focal = FC.sphere_scene()
    vol = device_volume(FC.SPHERE_VOLUME).integrate(depths, cam_to_world=c2w, focals=focal)
    ref = sphere_volume()
    assert_same_volume(vol, ref)
    assert_same_mesh(vol.extract_mesh(1.0), R.extract(ref.tsdf, ref.weight, ref.colour, ref.origin, ref.v, 1.0))


def test_extraction_edge_cases():
    spec = dict(origin=(0.0, 0.0, 0.0), dims=(5, 4, 3), voxel_size=0.5, truncation=1.0)
    vol = device_volume(spec)
    vol.integrate([], world_to_cam=np.zeros((0, 3, 4)), focals=[])                              # no frame: no launch
    v, c, f = vol.extract_mesh(1.0)
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    tsdf, weight = np.ones((3, 4, 5), np.float32), np.zeros((3, 4, 5), np.float32)
    weight[1:, 1:3, 2:4] = 1.0
    tsdf[2, 2, 3] = -0.25
    want = R.extract(tsdf, weight, None, spec["origin"], 0.5, 1.0)
    assert want[0].shape == (1, 3) and want[2].shape == (0, 3)
    got = upload(vol, tsdf, weight).extract_mesh(1.0)
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and got[2].shape == (0, 3)
    rng = np.random.default_rng(5)                                                             # nx = 2: one layer of cells
    tsdf, weight = rng.uniform(-1, 1, (6, 5, 2)).astype(np.float32), (rng.random((6, 5, 2)) < 0.9).astype(np.float32)
    colour = rng.uniform(0, 255, (3, 6, 5, 2)).astype(np.float32)
    thin = upload(device_volume(dict(spec, dims=(2, 5, 6))), tsdf, weight, colour)
    want = R.extract(tsdf, weight, colour, spec["origin"], 0.5, 1.0)
    assert len(want[0]) > 5
    assert_same_mesh(thin.extract_mesh(1.0), want)


def test_argument_validation_with_device_buffers():
    from acezero_amd import _native as N
    from acezero_amd.head import _ptr
    lib = N.lib()
    vol = device_volume(dict(origin=(0.0, 0.0, 0.0), dims=(4, 4, 4), voxel_size=0.02, truncation=0.08))
    depth = torch.zeros(48, dtype=torch.int16, device="cuda")
    d_rows = torch.zeros(80, dtype=torch.uint8, device="cuda")
    rows = (N.TsdfFrame * 1)()
    rows[0].m[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.5]
    rows[0].focal, rows[0].ppx, rows[0].ppy, rows[0].h, rows[0].w, rows[0].offset = 40.0, 4.0, 3.0, 6, 8, 0

    def call(tsdf=vol.tsdf, d=depth, dims=(4, 4, 4), tau=0.08, n_pixels=48, frames=rows, d_frames=d_rows):
        return lib.acez_tsdf_integrate(_ptr(tsdf), _ptr(vol.weight), _ptr(vol.colour), *dims, 0.0, 0.0, 0.0, 0.02, tau, _ptr(d), None, n_pixels,
                                       frames, 1, _ptr(d_frames), 0.001, 4.0, 64.0, 1, None)

    assert call() == 0
    torch.cuda.synchronize()
    rows[0].offset = 1
    assert call() == -1 and b"past the end" in lib.acez_last_error()
    rows[0].offset = 0
    assert call(n_pixels=47) == -1 and b"past the end" in lib.acez_last_error()
    assert call(dims=(4, 0, 4)) == -1 and b"dimensions" in lib.acez_last_error()
    assert call(tau=0.0) == -1 and call(tau=-1.0) == -1 and b"positive" in lib.acez_last_error()
    assert call(tsdf=None) == -1 and call(d=None) == -1 and call(frames=None) == -1 and call(d_frames=None) == -1
    assert b"null pointer" in lib.acez_last_error()
    with pytest.raises(N.AcezError, match="ACEZ_ERR_INVALID"):
        N.check(call(tau=0.0))
    torch.cuda.synchronize()                                     # nothing was launched by the refused calls; the device is fine
    assert float(vol.weight.sum().item()) == 0.0                 # (all-zero depth)


def test_fuse_depth_end_to_end(tmp_path):
    args = FC.write_room_scene(tmp_path, 12, 120, 160, 100.0)
    outs = []
    for run in range(2):
        args[2] = str(tmp_path / f"mesh_{run}.ply")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "fuse_depth.py")] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(open(args[2], "rb").read())
    assert "Fused 12 of 12 frames" in r.stderr and "vertices" in r.stderr and "Known voxels" in r.stderr
    v, c, f = FC.read_mesh_ply(args[2])
    assert len(v) > 3000 and len(f) > 5000 and f.min() >= 0 and f.max() < len(v)
    wd = FC.wall_distance(v)
    print(f"{len(v)} vertices, {len(f)} faces, largest distance to a wall plane {wd.max() * 1000:.3f} mm")
    assert wd.max() <= DISTANCE_BOUND
    palette = {(220, 60, 60), (60, 220, 60), (60, 60, 220), (220, 220, 60), (60, 220, 220), (220, 60, 220)}
    flat = wd < 0.002                                            # away from the room's edges a vertex has its wall's colour
    assert len({tuple(x) for x in c[flat]} & palette) >= 4
    assert outs[0] == outs[1], "two runs wrote different files"
