"""CPU: the DEFINITION of the block-sparse TSDF volume (include/acez.h section K2) checked on its numpy restatement
(tests/tsdf_sparse_restated.py): the mark rule is a superset of what the dense extraction reads and is really sparse, and the sparse
chain's mesh is the dense restatement's mesh; fuse_depth.py --sparse True's refusals and the entry points' argument checks, none of
which needs a device."""
import functools

import numpy as np
import pytest

from tests import fusion_cases as FC
from tests import tsdf_restated as R
from tests import tsdf_sparse_restated as S
from tests.test_fusion_cpu import sphere_mesh, sphere_volume
from tests.test_fusion_gpu import MAX_DEPTH, MIXED, mixed_frames, mixed_reference

SPHERE = {k: FC.SPHERE_VOLUME[k] for k in ("origin", "dims", "voxel_size", "truncation")}
MIXED_GRID = {k: MIXED[k] for k in ("origin", "dims", "voxel_size", "truncation")}


@functools.lru_cache(maxsize=None)
def sphere_flags():
    depths, c2w, focal = FC.sphere_scene()
    n = len(depths)
    return S.mark(**SPHERE, depths=depths, w2c=np.linalg.inv(c2w), focals=[focal] * n, ppx=[40.0] * n, ppy=[30.0] * n)


@functools.lru_cache(maxsize=None)
def mixed_flags():
    depths, _, w2c, focals, ppx, ppy = mixed_frames()
    return S.mark(**MIXED_GRID, depths=depths, w2c=w2c, focals=focals, ppx=ppx, ppy=ppy, max_depth=MAX_DEPTH)


ROOM_FRAMES = (12, 120, 160, 100.0)      # FC.write_room_scene's frames as tests/test_fusion_gpu.py's end-to-end run writes them


@functools.lru_cache(maxsize=None)
def room_case(voxel_size=0.02):
    """(dense restated volume, flags) of the box room seen by write_room_scene's cameras, in fuse_depth.py's own bounds."""
    from acezero_amd.fusion import bounds_from_frames
    n, h, w, focal = ROOM_FRAMES
    c2w = FC.room_cameras(n)
    depths = [FC.room_depth(T, h, w, focal) for T in c2w]
    tau = 4.0 * voxel_size
    origin, dims = bounds_from_frames(depths, c2w, focal, voxel_size, tau)
    args = dict(depths=depths, w2c=np.linalg.inv(c2w), focals=[focal] * n, ppx=[w / 2.0] * n, ppy=[h / 2.0] * n)
    vol = R.integrate(R.Volume(origin, dims, voxel_size, tau), **args)
    return vol, S.mark(origin, dims, voxel_size, tau, **args)


def assert_superset(vol, flags):
    """Every voxel with tsdf < 0 and weight > 0, and each of its 26 neighbours inside the grid, is in a marked block."""
    dims = (vol.nx, vol.ny, vol.nz)
    marked = S.voxel_mask(flags, dims)
    k, j, i = np.nonzero((vol.tsdf < 0) & (vol.weight > 0))
    assert len(i) > 100
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ii, jj, kk = i + dx, j + dy, k + dz
                ok = (ii >= 0) & (jj >= 0) & (kk >= 0) & (ii < vol.nx) & (jj < vol.ny) & (kk < vol.nz)
                missed = ~marked[kk[ok], jj[ok], ii[ok]]
                assert not missed.any(), f"{int(missed.sum())} voxels at offset ({dx}, {dy}, {dz}) of an inside voxel are in unmarked blocks"


def test_mark_is_a_superset_on_the_sphere():
    assert_superset(sphere_volume(), sphere_flags())


def test_mark_is_a_superset_on_the_mixed_frames():
    """37 x 29 x 21: no axis is a multiple of 8; the camera inside the volume, the long lens and the empty frame occur."""
    flags = mixed_flags()
    assert flags.shape == (3, 4, 5)
    assert_superset(mixed_reference(True), flags)
    assert 0.0 < flags.mean() < 1.0, "the marked share of MIXED must lie strictly between 0 and 1"


def test_mark_is_a_superset_in_the_room():
    vol, flags = room_case()
    assert_superset(vol, flags)
    assert 0.0 < flags.mean() < 1.0


def test_marking_the_sphere_is_sparse():
    flags = sphere_flags()
    assert flags.shape == (6, 6, 6)
    print(f"sphere: {int(flags.sum())} of {flags.size} blocks marked")
    assert flags.any(), "no block is marked"
    assert not flags.all(), "every block is marked"
    assert 0.0 < flags.mean() < 1.0
    assert not flags[0, 0, 0] and not flags[5, 5, 5], "a corner block of the volume is 0.3 m from the surface"


# FC.SPHERE_VOLUME grown by half a block on every side: 56^3 voxels, 7^3 blocks, the same voxel planes. The sphere's centre, voxel
# index 27.5, is then the centre of block 3 (voxels 24 .. 31), so that "the sphere's centre block" exists.
SPHERE_CENTRED = dict(origin=(-0.55, -0.55, -0.55), dims=(56, 56, 56), voxel_size=0.02, truncation=0.08)


@functools.lru_cache(maxsize=None)
def centred_sphere_case():
    depths, c2w, focal = FC.sphere_scene()
    n = len(depths)
    args = dict(depths=depths, w2c=np.linalg.inv(c2w), focals=[focal] * n, ppx=[40.0] * n, ppy=[30.0] * n)
    return R.integrate(R.Volume(**SPHERE_CENTRED), **args), S.mark(**SPHERE_CENTRED, **args)


def test_the_spheres_centre_block_is_not_marked():
    """In FC.SPHERE_VOLUME itself no block is the sphere's centre block: the centre (0, 0, 0) lies at voxel index 23.5 on every axis,
    the common corner of eight blocks, each of which reaches 0.26 m out along its diagonal, into the truncation band of the 0.3 m
    sphere. The dense restatement has 20 voxels with tsdf < 0 in each of the eight, so the superset property requires all eight to be
    marked, and they are (asserted here, so that the marking is not tighter than it may be). The assertion about the centre block is
    therefore made on the same scene, frames, voxel planes and truncation in a grid half a block larger on every side, in which the
    centre is the middle of a block: that block lies within 0.13 m of the centre, holds no voxel with tsdf < 0 and is not marked,
    and the superset property holds in that grid too."""
    vol, flags = sphere_volume(), sphere_flags()
    inside = (vol.tsdf < 0) & (vol.weight > 0)
    for bk in (2, 3):
        for bj in (2, 3):
            for bi in (2, 3):
                assert inside[8 * bk:8 * bk + 8, 8 * bj:8 * bj + 8, 8 * bi:8 * bi + 8].sum() == 20 and flags[bk, bj, bi]
    vol, flags = centred_sphere_case()
    assert flags.shape == (7, 7, 7)
    assert_superset(vol, flags)
    assert 0.0 < flags.mean() < 1.0
    assert not ((vol.tsdf < 0) & (vol.weight > 0))[24:32, 24:32, 24:32].any()
    assert not flags[3, 3, 3], "the sphere's centre block is marked"
    assert flags[3, 3, 1] and flags[3, 3, 5] and flags[1, 3, 3] and flags[3, 5, 3], "the blocks the surface passes through are not marked"


def test_the_sparse_chain_gives_the_dense_mesh_on_the_sphere():
    want = sphere_mesh()
    assert len(want[0]) > 1000 and len(want[2]) > 2000
    S.assert_same_mesh(S.sparse_chain(sphere_volume(), sphere_flags(), 1.0), want)


def test_the_sparse_chain_gives_the_dense_mesh_in_the_room():
    vol, flags = room_case()
    want = R.extract(vol.tsdf, vol.weight, vol.colour, vol.origin, vol.v, 2.0)
    assert len(want[0]) > 3000 and len(want[2]) > 5000
    S.assert_same_mesh(S.sparse_chain(vol, flags, 2.0), want)


def test_the_mesh_comparison_sees_a_difference():
    v, c, f = sphere_mesh()
    order = np.random.default_rng(1).permutation(len(v))
    rename = np.empty(len(v), np.int64)
    rename[order] = np.arange(len(v))
    shuffled = (v[order], c[order], rename[f][::-1].astype(np.int32))
    S.assert_same_mesh(shuffled, (v, c, f))
    flipped = shuffled[2].copy()
    flipped[0] = flipped[0, ::-1]                                # one face turned over
    with pytest.raises(AssertionError, match="face rows differ"):
        S.assert_same_mesh((shuffled[0], shuffled[1], flipped), (v, c, f))
    moved = shuffled[0].copy()
    moved[5, 1] = np.nextafter(moved[5, 1], np.float32(np.inf))  # one ulp
    with pytest.raises(AssertionError, match="one mesh only"):
        S.assert_same_mesh((moved, shuffled[1], shuffled[2]), (v, c, f))


def test_block_layout_round_trip():
    flags = mixed_flags()
    nx, ny, nz = MIXED["dims"]
    dense = np.arange(nx * ny * nz, dtype=np.float32).reshape(nz, ny, nx)
    rows = S.to_blocks(dense, flags, -1.0)
    inside = S.inside_grid(flags, MIXED["dims"])
    assert rows.shape == (int(flags.sum()), 8, 8, 8) and (rows[~inside] == -1.0).all() and (~inside).sum() > 100
    blocks = np.flatnonzero(flags.reshape(-1))
    bz, by, bx = flags.shape
    slot = 7
    b = blocks[slot]
    bi, bj, bk = b % bx, (b // bx) % by, b // (bx * by)
    assert rows[slot, 1, 2, 3] == dense[8 * bk + 1, 8 * bj + 2, 8 * bi + 3]


def test_cli_refusals(tmp_path):
    from acezero_amd import cli
    args = FC.write_room_scene(tmp_path, 3, 24, 32, 20.0) + ["--sparse", "True"]
    with pytest.raises(SystemExit, match="more than 2\\^28: raise --voxel_size or lower --max_depth"):
        cli.fuse_depth_main(args + ["--voxel_size", "0.0002"])   # a 1.4 m room in 0.2 mm voxels: some 7000^3 voxels, 6e8 blocks
    import torch
    if not torch.cuda.is_available():
        # --max_voxels counts allocated voxels, which the device decides: the dense refusal does not apply, the run gets to the device
        with pytest.raises(SystemExit, match="needs a GPU"):
            cli.fuse_depth_main(args + ["--max_voxels", "1000"])
    assert not (tmp_path / "mesh.ply").exists()


def test_argument_validation_without_device():
    from acezero_amd import _native as N
    lib = N.lib()
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data                                          # never dereferenced: every call below is refused before any launch
    rows = (N.TsdfFrame * 1)()
    rows[0].m[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    rows[0].focal, rows[0].ppx, rows[0].ppy, rows[0].h, rows[0].w, rows[0].offset = 40.0, 4.0, 3.0, 6, 8, 0

    def mark(flags=p, depth=p, frames=rows, d_frames=p, dims=(20, 20, 20), v=0.02, tau=0.08, n_pixels=48, n_frames=1):
        return lib.acez_tsdf_mark(flags, *dims, 0.0, 0.0, 0.0, v, tau, depth, n_pixels, frames, n_frames, d_frames, 0.001, 4.0, None)

    def integrate(tsdf=p, slots=p, n_blocks=2, depth=p, frames=rows, d_frames=p, dims=(20, 20, 20), v=0.02, tau=0.08, n_pixels=48, n_frames=1,
                  colour=None, rgb=None):
        return lib.acez_tsdf_integrate_blocks(tsdf, p, colour, slots, n_blocks, *dims, 0.0, 0.0, 0.0, v, tau, depth, rgb, n_pixels, frames,
                                              n_frames, d_frames, 0.001, 4.0, 64.0, 1, None)

    def cells(tsdf=p, table=p, slots=p, n_blocks=2, dims=(20, 20, 20), v=0.02, min_weight=1.0, active=p, rank=None, out=None, n_vertices=0):
        return lib.acez_tsdf_cells_blocks(tsdf, p, None, table, slots, n_blocks, *dims, 0.0, 0.0, 0.0, v, min_weight, active, rank, out, None,
                                          n_vertices, None)

    def faces(tsdf=p, table=p, slots=p, n_blocks=2, dims=(20, 20, 20), min_weight=1.0, active=p, flags=p, vrank=None, erank=None, out=None,
              n_faces=0):
        return lib.acez_tsdf_faces_blocks(tsdf, p, table, slots, n_blocks, *dims, min_weight, active, flags, vrank, erank, out, n_faces, None)

    def refused(rc, text):
        assert rc == -1 and text in lib.acez_last_error(), lib.acez_last_error()

    import torch
    if not torch.cuda.is_available():
        for call in (mark, integrate, cells, faces):
            assert call() == -3 and b"no HIP device" in lib.acez_last_error()          # valid arguments: ACEZ_ERR_NODEVICE
    huge = (16384, 16384, 16384)                                 # 2048^3 = 2^33 blocks
    for call in (mark, integrate, cells, faces):
        refused(call(dims=huge), b"block grid too large")
        refused(call(dims=(20, 0, 20)), b"dimensions")
    refused(mark(flags=None), b"null pointer")
    refused(mark(depth=None), b"null pointer")
    refused(mark(frames=None), b"null pointer")
    refused(mark(d_frames=None), b"null pointer")
    refused(mark(v=0.0), b"positive")
    refused(mark(tau=0.0), b"positive")
    refused(mark(tau=float("nan")), b"non-finite")
    refused(mark(n_frames=257), b"frame count")
    refused(mark(n_pixels=47), b"past the end")
    refused(integrate(tsdf=None), b"null pointer")
    refused(integrate(slots=None), b"null pointer")
    refused(integrate(rgb=p), b"colour images without a colour volume")
    refused(integrate(n_blocks=-1), b"negative block count")
    refused(integrate(n_blocks=28), b"more blocks than the block grid has")      # 3^3 = 27 blocks
    refused(integrate(tau=-0.08), b"positive")
    refused(integrate(v=0.0), b"positive")
    refused(integrate(n_pixels=47), b"past the end")
    refused(cells(tsdf=None), b"null pointer")
    refused(cells(table=None), b"null pointer")
    refused(cells(active=None), b"null pointer")
    refused(cells(n_blocks=-1), b"negative block count")
    refused(cells(v=0.0), b"positive")
    refused(cells(min_weight=0.0), b"min_weight must be positive")
    refused(cells(rank=p, n_vertices=5), b"without a vertex buffer")
    refused(cells(dims=(8192, 8192, 8192), n_blocks=2 ** 21), b"too many blocks")
    refused(faces(table=None), b"null pointer")
    refused(faces(flags=None), b"null pointer")
    refused(faces(min_weight=-1.0), b"min_weight must be positive")
    refused(faces(erank=p, n_faces=2), b"without vertex ranks")
    refused(faces(vrank=p, erank=p, out=p, n_faces=-2), b"negative")
    rows[0].offset = 1
    refused(mark(), b"past the end")
    refused(integrate(), b"past the end")
    rows[0].offset = 0
    rows[0].m[:] = [1, 0, 0, 0, 2, 0, 0, 0, 0, 0, 1, 0]          # rows 0 and 1 parallel
    refused(mark(), b"singular pose")


def test_host_tensors_are_refused():
    from acezero_amd.fusion import SparseTSDFVolume
    with pytest.raises(RuntimeError, match="no CPU path"):
        SparseTSDFVolume((0, 0, 0), (4, 4, 4), 0.02, 0.08, "cpu")
