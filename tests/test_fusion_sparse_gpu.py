"""GPU: the block-sparse TSDF kernels of acezero_amd/csrc/fusion_api.hip (include/acez.h section K2) against the numpy restatements
(tests/tsdf_sparse_restated.py for the mark rule and the layout, tests/tsdf_restated.py for the voxels and the mesh): flags byte for
byte, voxels bit for bit, the mesh as the dense mesh under the comparison rule; a virtual grid the dense path refuses; the entry
points' argument checks with device buffers; fuse_depth.py --sparse True end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import fusion_cases as FC
from tests import tsdf_restated as R
from tests import tsdf_sparse_restated as S
from tests.test_fusion_cpu import DISTANCE_BOUND, sphere_volume
from tests.test_fusion_gpu import MAX_DEPTH, MIXED, mixed_frames, mixed_reference
from tests.test_fusion_sparse_cpu import ROOM_FRAMES, mixed_flags, room_case, sphere_flags

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sparse_volume(spec, **kw):
    from acezero_amd.fusion import SparseTSDFVolume
    return SparseTSDFVolume(spec["origin"], spec["dims"], spec["voxel_size"], spec["truncation"], "cuda", max_weight=spec.get("max_weight", 64.0), **kw)


def mixed_args(lo=0, hi=5, colour=False):
    depths, rgbs, w2c, focals, ppx, ppy = mixed_frames()
    args = dict(world_to_cam=w2c[lo:hi], focals=focals[lo:hi], ppx=ppx[lo:hi], ppy=ppy[lo:hi], max_depth=MAX_DEPTH)
    if colour:
        args["rgb"] = rgbs[lo:hi]
    return depths[lo:hi], args


def sphere_args(lo=0, hi=14):
    depths, c2w, focal = FC.sphere_scene()
    return depths[lo:hi], dict(cam_to_world=c2w[lo:hi], focals=focal)


def marked_mixed(chunks=((0, 5),)):
    vol = sparse_volume(MIXED)
    for lo, hi in chunks:
        depths, args = mixed_args(lo, hi)
        vol.mark(depths, **args)
    return vol


def marked_sphere(chunks=((0, 14),), spec=FC.SPHERE_VOLUME):
    vol = sparse_volume(spec)
    for lo, hi in chunks:
        depths, args = sphere_args(lo, hi)
        vol.mark(depths, **args)
    return vol


def flags_of(vol):
    bx, by, bz = vol.grid
    return vol.block_flags.cpu().numpy().reshape(bz, by, bx)


def test_mark_matches_the_restatement():
    for once, parts, want in ((marked_sphere(), marked_sphere(((0, 5), (5, 6), (6, 14))), sphere_flags()),
                              (marked_mixed(), marked_mixed(((0, 2), (2, 4), (4, 5))), mixed_flags())):
        got = flags_of(once)
        assert got.shape == want.shape
        assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} block flags differ, first at {np.argwhere(got != want)[0]}"
        assert np.array_equal(flags_of(parts), want), "marking in three calls gives other flags than marking in one"
        assert 0 < int(want.sum()) < want.size


def assert_same_blocks(vol, ref, flags):
    """Every voxel of every allocated block holds the dense restatement's bits; beyond the grid the storage is as allocate() left it."""
    assert vol.allocated_blocks == int(flags.sum())
    blocks = np.flatnonzero(flags.reshape(-1))
    assert np.array_equal(vol.slot_blocks.cpu().numpy(), blocks)
    table = np.full(flags.size, -1, np.int32)
    table[blocks] = np.arange(len(blocks))
    assert np.array_equal(vol.block_table.cpu().numpy().reshape(-1), table)
    for name, got, want in (("tsdf", vol.tsdf, S.to_blocks(ref.tsdf, flags, np.float32(1.0))),
                            ("weight", vol.weight, S.to_blocks(ref.weight, flags, np.float32(0.0))),
                            ("colour", vol.colour, np.stack([S.to_blocks(ref.colour[ch], flags, np.float32(0.0)) for ch in range(3)]))):
        got = got.cpu().numpy()
        diff = got.view(np.uint32) != want.view(np.uint32)
        assert not diff.any(), f"{name}: {int(diff.sum())} of {diff.size} voxels differ, first at {np.argwhere(diff)[0]}"
    beyond = ~S.inside_grid(flags, (ref.nx, ref.ny, ref.nz))
    assert (vol.weight.cpu().numpy()[beyond] == 0).all()


def integrate_mixed(colour, chunks=((0, 5),), **kw):
    vol = marked_mixed()
    vol.allocate()
    for lo, hi in chunks:
        depths, args = mixed_args(lo, hi, colour)
        vol.integrate(depths, **args, **kw)
    torch.cuda.synchronize()
    return vol


@pytest.mark.parametrize("colour", [True, False])
def test_integrate_matches_the_restatement(colour):
    ref, flags = mixed_reference(colour), mixed_flags()
    assert (~S.inside_grid(flags, MIXED["dims"])).sum() > 1000     # partial blocks on every axis
    vol = integrate_mixed(colour)
    assert_same_blocks(vol, ref, flags)
    assert_same_blocks(integrate_mixed(colour, chunks=((0, 2), (2, 4), (4, 5))), ref, flags)     # the caller's chunks
    assert_same_blocks(integrate_mixed(colour, frames_per_call=2), ref, flags)                    # integrate()'s own chunks
    assert_same_blocks(integrate_mixed(colour, frustum_skip=False), ref, flags)
    # to_dense(): the dense restatement inside the marked blocks, the cleared state elsewhere
    mask = S.voxel_mask(flags, MIXED["dims"])
    tsdf, weight, colours = (t.cpu().numpy() for t in vol.to_dense())
    assert np.array_equal(tsdf.view(np.uint32), np.where(mask, ref.tsdf, np.float32(1.0)).view(np.uint32))
    assert np.array_equal(weight.view(np.uint32), np.where(mask, ref.weight, np.float32(0.0)).view(np.uint32))
    assert np.array_equal(colours.view(np.uint32), np.where(mask[None], ref.colour, np.float32(0.0)).view(np.uint32))
    assert vol.known_voxels(1.0) == int(((ref.weight >= 1.0) & mask).sum())


def fused_sphere(chunks=((0, 14),)):
    vol = marked_sphere()
    vol.allocate()
    for lo, hi in chunks:
        depths, args = sphere_args(lo, hi)
        vol.integrate(depths, **args)
    return vol


def test_sphere_fused_on_the_device_is_the_restatements_sphere():
    ref = sphere_volume()
    once, parts = fused_sphere(), fused_sphere(((0, 5), (5, 6), (6, 14)))
    assert_same_blocks(once, ref, sphere_flags())
    mesh, again = once.extract_mesh(1.0), parts.extract_mesh(1.0)
    S.assert_same_mesh([t.cpu().numpy() for t in mesh], R.extract(ref.tsdf, ref.weight, ref.colour, ref.origin, ref.v, 1.0))
    for a, b in zip(mesh, again):
        assert torch.equal(a, b), "the row order depends on how the integration was cut into calls"
    vid = mesh[2].cpu().numpy()
    assert vid.min() >= 0 and vid.max() < len(mesh[0])


def upload(vol, flags, tsdf, weight, colour):
    vol.tsdf.copy_(torch.from_numpy(S.to_blocks(tsdf, flags, np.float32(1.0))))
    vol.weight.copy_(torch.from_numpy(S.to_blocks(weight, flags, np.float32(0.0))))
    vol.colour.copy_(torch.from_numpy(np.stack([S.to_blocks(colour[ch], flags, np.float32(0.0)) for ch in range(3)])))
    return vol


@pytest.mark.parametrize("slab", [False, True])
def test_extraction_matches_the_restatement(slab):
    ref, flags = sphere_volume(), sphere_flags()
    tsdf, weight = ref.tsdf.copy(), ref.weight.copy()
    colour = np.random.default_rng(3).uniform(0, 255, (3,) + tsdf.shape).astype(np.float32)
    if slab:
        weight[:, 19:22, :] = 0                                  # an unknown slab through the sphere: the mesh has a boundary there
    want = R.extract(tsdf, weight, colour, ref.origin, ref.v, 1.0)
    assert len(want[0]) > 1000 and len(want[2]) > 2000
    if slab:
        assert (FC.mesh_edge_counts(want[2])[0] == 1).any()
    vol = marked_sphere()
    vol.allocate()
    upload(vol, flags, tsdf, weight, colour)
    first, second = vol.extract_mesh(1.0), vol.extract_mesh(1.0)
    S.assert_same_mesh([t.cpu().numpy() for t in first], want)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    # the order: vertices ascend by block, then by voxel inside the block
    v = first[0].cpu().numpy().astype(np.float64)
    idx = np.floor((v - np.asarray(ref.origin, np.float64)) / 0.02 + 1e-6).astype(np.int64)      # the cell of every vertex
    bx, by, _ = vol.grid
    key = (((idx[:, 2] >> 3) * by + (idx[:, 1] >> 3)) * bx + (idx[:, 0] >> 3)) * 512 + ((idx[:, 2] & 7) * 8 + (idx[:, 1] & 7)) * 8 + (idx[:, 0] & 7)
    assert (np.diff(key) > 0).all(), "vertex ids do not ascend by block index, then by voxel index"


BIG = 2048
BIG_BLOCK = (100, 140, 60)               # the block whose centre is the sphere's centre


def test_a_volume_the_dense_path_cannot_hold():
    """The sphere in a virtual grid of 2048^3 voxels, 256^3 blocks, far from voxel (0, 0, 0), its centre at the centre of a block (voxel
    index 8 b + 3.5): that block is 0.14 m from the centre at its corners, inside the sphere beyond the truncation, and is not marked."""
    from acezero_amd import _native as N
    from acezero_amd.head import _ptr
    lib = N.lib()
    small = torch.zeros(8, dtype=torch.float32, device="cuda")
    assert BIG ** 3 >= 2 ** 31 // 3
    rc = lib.acez_tsdf_cells(_ptr(small), _ptr(small), None, BIG, BIG, BIG, 0.0, 0.0, 0.0, 0.02, 1.0, _ptr(small), None, None, None, 0, None)
    assert rc == -1 and b"too large" in lib.acez_last_error()
    spec = dict(FC.SPHERE_VOLUME, dims=(BIG, BIG, BIG), origin=tuple(-(8 * b + 3.5) * 0.02 for b in BIG_BLOCK))
    vol = marked_sphere(spec=spec)
    n = vol.allocate()
    n_grid = (BIG // 8) ** 3
    print(f"{n} of {n_grid} blocks allocated ({100.0 * n / n_grid:.4f} %)")
    assert 0 < n < 0.01 * n_grid
    bi, bj, bk = BIG_BLOCK
    assert int(vol.block_table[bk, bj, bi].item()) == -1, "the block around the sphere's centre is marked"
    with pytest.raises(ValueError, match="too large"):
        vol.to_dense()
    depths, args = sphere_args()
    vol.integrate(depths, **args)
    v, _, f = (t.cpu().numpy() for t in vol.extract_mesh(1.0))
    assert len(v) > 1000 and len(f) > 2000 and f.min() >= 0 and f.max() < len(v)
    undirected, directed = FC.mesh_edge_counts(f)
    assert (undirected == 2).all(), f"{int((undirected != 2).sum())} edges do not belong to exactly two faces"
    assert (directed == 1).all(), "the orientation is not consistent"
    distance = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - FC.SPHERE_R).max()
    print(f"{len(v)} vertices, {len(f)} faces, largest distance to the sphere {distance * 1000:.3f} mm")
    assert distance <= DISTANCE_BOUND
    assert FC.signed_volume(v, f) > 0, "normals point inwards"


def test_volume_life_cycle():
    vol = sparse_volume(MIXED, max_blocks=5)
    depths, args = mixed_args()
    with pytest.raises(ValueError, match="before allocate"):
        vol.integrate(depths, **args)
    vol.mark(depths, **args)
    with pytest.raises(ValueError, match="max_blocks 5"):
        vol.allocate()
    vol = marked_mixed()
    assert vol.allocated_blocks is None
    assert vol.allocate() == int(mixed_flags().sum()) == vol.allocated_blocks
    with pytest.raises(ValueError, match="after allocate"):
        vol.mark(depths, **args)
    empty = sparse_volume(MIXED)
    empty.mark(depths[4:], **mixed_args(4, 5)[1])                # the frame without any depth
    assert empty.allocate() == 0 and empty.tsdf is None and empty.known_voxels(1.0) == 0
    empty.integrate(depths, **args)                              # no block: no launch
    v, c, f = empty.extract_mesh(1.0)
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    with pytest.raises(ValueError, match="min_weight must be positive"):
        vol.extract_mesh(0.0)


def test_argument_validation_with_device_buffers():
    from acezero_amd import _native as N
    from acezero_amd.head import _ptr
    lib = N.lib()
    spec = dict(origin=(0.0, 0.0, 0.0), dims=(20, 20, 20), voxel_size=0.02, truncation=0.08)
    rows = (N.TsdfFrame * 1)()
    rows[0].m[:] = [1, 0, 0, -0.2, 0, 1, 0, -0.2, 0, 0, 1, 0.5]
    rows[0].focal, rows[0].ppx, rows[0].ppy, rows[0].h, rows[0].w, rows[0].offset = 40.0, 4.0, 3.0, 6, 8, 0
    vol = sparse_volume(spec)
    seen = torch.full((48,), 600, dtype=torch.int16, device="cuda")
    empty = torch.zeros(48, dtype=torch.int16, device="cuda")
    d_rows = torch.zeros(80, dtype=torch.uint8, device="cuda")

    def mark(flags=vol.block_flags, d=seen, dims=(20, 20, 20), tau=0.08, n_pixels=48, frames=rows, d_frames=d_rows):
        return lib.acez_tsdf_mark(_ptr(flags), *dims, 0.0, 0.0, 0.0, 0.02, tau, _ptr(d), n_pixels, frames, 1, _ptr(d_frames), 0.001, 4.0, None)

    assert mark(tau=0.0) == -1 and b"positive" in lib.acez_last_error()
    assert mark(flags=None) == -1 and mark(d=None) == -1 and mark(frames=None) == -1 and mark(d_frames=None) == -1
    assert b"null pointer" in lib.acez_last_error()
    assert mark(n_pixels=47) == -1 and b"past the end" in lib.acez_last_error()
    assert mark(dims=(16384, 16384, 16384)) == -1 and b"block grid too large" in lib.acez_last_error()
    torch.cuda.synchronize()
    assert int(vol.block_flags.sum().item()) == 0                # nothing was launched by the refused calls
    assert mark() == 0
    n = vol.allocate()
    assert 0 < n <= 27

    def integrate(tsdf=vol.tsdf, slots=vol.slot_blocks, n_blocks=n, d=empty, dims=(20, 20, 20), tau=0.08, n_pixels=48, frames=rows, d_frames=d_rows):
        return lib.acez_tsdf_integrate_blocks(_ptr(tsdf), _ptr(vol.weight), _ptr(vol.colour), _ptr(slots), n_blocks, *dims, 0.0, 0.0, 0.0, 0.02,
                                              tau, _ptr(d), None, n_pixels, frames, 1, _ptr(d_frames), 0.001, 4.0, 64.0, 1, None)

    def cells(table=vol.block_table, n_blocks=n, dims=(20, 20, 20), min_weight=1.0, active=vol.weight):
        return lib.acez_tsdf_cells_blocks(_ptr(vol.tsdf), _ptr(vol.weight), None, _ptr(table), _ptr(vol.slot_blocks), n_blocks, *dims, 0.0, 0.0,
                                          0.0, 0.02, min_weight, _ptr(active), None, None, None, 0, None)

    def faces(table=vol.block_table, n_blocks=n, dims=(20, 20, 20), min_weight=1.0, flags=vol.weight):
        return lib.acez_tsdf_faces_blocks(_ptr(vol.tsdf), _ptr(vol.weight), _ptr(table), _ptr(vol.slot_blocks), n_blocks, *dims, min_weight,
                                          _ptr(vol.weight), _ptr(flags), None, None, None, 0, None)

    assert integrate() == 0                                      # (all-zero depth: nothing is written)
    torch.cuda.synchronize()
    rows[0].offset = 1
    assert integrate() == -1 and b"past the end" in lib.acez_last_error()
    rows[0].offset = 0
    assert integrate(d=seen, n_pixels=47) == -1 and b"past the end" in lib.acez_last_error()
    assert integrate(d=seen, dims=(20, 0, 20)) == -1 and b"dimensions" in lib.acez_last_error()
    assert integrate(d=seen, tau=0.0) == -1 and integrate(d=seen, tau=-1.0) == -1 and b"positive" in lib.acez_last_error()
    assert integrate(d=seen, n_blocks=-1) == -1 and b"negative block count" in lib.acez_last_error()
    assert integrate(d=seen, n_blocks=28) == -1 and b"more blocks than the block grid has" in lib.acez_last_error()
    assert integrate(d=seen, dims=(16384, 16384, 16384)) == -1 and b"block grid too large" in lib.acez_last_error()
    assert integrate(tsdf=None) == -1 and integrate(slots=None) == -1 and integrate(d=None) == -1 and integrate(frames=None) == -1
    assert integrate(d_frames=None) == -1 and b"null pointer" in lib.acez_last_error()
    # (the refused extraction calls would have written flags over the weights)
    assert cells(table=None) == -1 and cells(active=None) == -1 and b"null pointer" in lib.acez_last_error()
    assert cells(n_blocks=-1) == -1 and cells(n_blocks=28) == -1 and b"more blocks" in lib.acez_last_error()
    assert cells(min_weight=0.0) == -1 and b"min_weight must be positive" in lib.acez_last_error()
    assert cells(dims=(16384, 16384, 16384)) == -1 and b"block grid too large" in lib.acez_last_error()
    assert faces(table=None) == -1 and faces(flags=None) == -1 and b"null pointer" in lib.acez_last_error()
    assert faces(n_blocks=-1) == -1 and faces(min_weight=0.0) == -1 and faces(dims=(20, 20, 0)) == -1
    with pytest.raises(N.AcezError, match="ACEZ_ERR_INVALID"):
        N.check(integrate(d=seen, tau=0.0))
    torch.cuda.synchronize()                                     # nothing was launched by the refused calls; the device is fine
    assert float(vol.weight.sum().item()) == 0.0 and float(vol.colour.abs().sum().item()) == 0.0
    assert bool((vol.tsdf == 1.0).all().item())


# ------------------------------------------------------------------------------------------------------------- fuse_depth.py --sparse True
MAX_VOXELS = 300000                      # between the room's allocated voxels and its dense volume at 0.02 m: asserted below


def run_fuse_depth(args, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fuse_depth.py")] + list(args) + list(extra), cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    return r


@pytest.fixture(scope="module")
def room_runs(tmp_path_factory):
    """The room scene, one dense run and two sparse runs of the same command under --max_voxels MAX_VOXELS."""
    folder = tmp_path_factory.mktemp("sparse_room")
    n, h, w, focal = ROOM_FRAMES
    args = FC.write_room_scene(folder, n, h, w, focal)
    out = {"args": args}
    for name, extra in (("dense", ()), ("sparse_0", ("--sparse", "True", "--max_voxels", str(MAX_VOXELS))),
                        ("sparse_1", ("--sparse", "True", "--max_voxels", str(MAX_VOXELS)))):
        run_args = list(args)
        run_args[2] = str(folder / f"{name}.ply")
        r = run_fuse_depth(run_args, *extra)
        assert r.returncode == 0, r.stderr[-3000:]
        out[name] = (run_args[2], r.stderr)
    return out


def test_fuse_depth_sparse_gives_the_dense_mesh(room_runs):
    dense, sparse = FC.read_mesh_ply(room_runs["dense"][0]), FC.read_mesh_ply(room_runs["sparse_0"][0])
    assert len(dense[0]) > 3000 and len(dense[2]) > 5000
    S.assert_same_mesh(sparse, dense)
    assert open(room_runs["sparse_0"][0], "rb").read() == open(room_runs["sparse_1"][0], "rb").read(), "two sparse runs wrote different files"
    log = room_runs["sparse_0"][1]
    _, flags = room_case()
    assert f"Allocated blocks: {int(flags.sum())} of {flags.size}" in log and "bytes of volume storage" in log
    assert "Fused 12 of 12 frames" in log and "Known voxels" in log
    assert "Allocated blocks" not in room_runs["dense"][1]


def test_fuse_depth_sparse_runs_where_dense_exceeds_max_voxels(room_runs):
    vol, flags = room_case()
    assert int(flags.sum()) * 512 < MAX_VOXELS < vol.nx * vol.ny * vol.nz        # chosen from bounds_from_frames and the restated block count
    args = list(room_runs["args"])
    args[2] = os.path.join(os.path.dirname(args[2]), "refused.ply")
    r = run_fuse_depth(args, "--max_voxels", str(MAX_VOXELS))
    assert r.returncode != 0 and f"more than --max_voxels {MAX_VOXELS}" in r.stderr and not os.path.exists(args[2])
    v, _, f = FC.read_mesh_ply(room_runs["sparse_0"][0])         # the same command with --sparse True succeeded
    assert len(v) > 3000 and len(f) > 5000 and f.min() >= 0 and f.max() < len(v)
    wd = FC.wall_distance(v)
    print(f"{len(v)} vertices, {len(f)} faces, largest distance to a wall plane {wd.max() * 1000:.3f} mm")
    assert wd.max() <= DISTANCE_BOUND
    r = run_fuse_depth(args, "--sparse", "True", "--max_voxels", str(int(flags.sum()) * 512 - 512))
    assert r.returncode != 0 and "more than --max_voxels" in r.stderr and "max_blocks" in r.stderr and not os.path.exists(args[2])
