"""TSDF fusion of depth maps along estimated poses and the fused surface as a triangle mesh (include/acez.h section K, DESIGN.md
section 4j; fuse_depth.py is the command line).

    vol = TSDFVolume(origin, (nx, ny, nz), voxel_size=0.02, truncation=0.08, device="cuda")
    vol.integrate(depth_u16, cam_to_world=poses, focals=f, ppx=cx, ppy=cy, rgb=rgb)
    vertices, colours, faces = vol.extract_mesh(min_weight=2)
    formats.write_ply("scene.ply", vertices.cpu(), colours.cpu(), faces.cpu())

The volume lives in HBM; integration and extraction are HIP kernels (acezero_amd/csrc/fusion_api.hip). There is no CPU fallback.
SparseTSDFVolume is the same function on a block-sparse volume (section K2), for grids whose dense volume does not fit.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from .head import _ptr, _stream


def _no_cpu(what):
    return RuntimeError(f"{what} needs device tensors: TSDF fusion is a HIP kernel, there is no CPU path")


def _w2c34(world_to_cam, cam_to_world, n):
    """float32 [n,3,4] world -> camera rows; a camera -> world input is inverted in float64 and rounded once."""
    if (world_to_cam is None) == (cam_to_world is None):
        raise ValueError("give exactly one of world_to_cam and cam_to_world")
    src = world_to_cam if cam_to_world is None else cam_to_world
    m = np.asarray(src.detach().cpu().numpy() if torch.is_tensor(src) else src, np.float64).reshape(n, -1, 4)
    if cam_to_world is not None:
        full = np.tile(np.eye(4), (n, 1, 1))
        full[:, :m.shape[1]] = m
        m = np.linalg.inv(full)
    return np.ascontiguousarray(m[:, :3].astype(np.float32))


def _per_frame(value, n):
    return np.broadcast_to(np.asarray(value, np.float64), (n,))


class TSDFVolume:
    """nx x ny x nz voxels of `voxel_size` metres, voxel (0,0,0)'s centre at `origin` (world, OpenCV convention). tsdf, weight
    [nz,ny,nx] and colour [3,nz,ny,nx] are float32 device tensors; a voxel no frame has reached has weight 0."""

    def __init__(self, origin, dims, voxel_size, truncation, device, max_weight=64.0):
        device = torch.device(device)
        if device.type != "cuda":
            raise _no_cpu("TSDFVolume")
        self.origin = tuple(float(np.float32(o)) for o in origin)
        self.dims = tuple(int(d) for d in dims)
        self.voxel_size, self.truncation, self.max_weight = float(voxel_size), float(truncation), float(max_weight)
        self.device = device
        nx, ny, nz = self.dims
        if min(self.dims) < 1:
            raise ValueError(f"volume dimensions {self.dims} must be at least 1")
        self.tsdf = torch.ones((nz, ny, nx), dtype=torch.float32, device=device)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=device)
        self.colour = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=device)
        self.frames_fused = 0

    def _pack(self, images, dtype, trailing):
        """One device tensor [n,h,w(,3)] or a list of per-frame arrays -> (flat device tensor, [(h, w)], element offsets)."""
        if torch.is_tensor(images):
            if not images.is_cuda:
                raise _no_cpu("TSDFVolume.integrate")
            if images.dtype in (torch.uint16, torch.int16) and dtype == np.uint16:
                images = images.view(torch.int16)
            elif not (images.dtype == torch.uint8 and dtype == np.uint8):
                raise TypeError(f"expected a {np.dtype(dtype).name} tensor, got {images.dtype}")
            n, h, w = images.shape[:3]
            if tuple(images.shape[3:]) != trailing:
                raise ValueError(f"expected [n,h,w{',3' if trailing else ''}], got {tuple(images.shape)}")
            return images.to(self.device).contiguous().reshape(-1), [(h, w)] * n, [i * h * w for i in range(n)]
        arrays = [np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a) for a in images]
        sizes, offsets, at = [], [], 0
        for a in arrays:
            if a.dtype != dtype or a.ndim != 2 + len(trailing) or tuple(a.shape[2:]) != trailing:
                raise TypeError(f"expected {np.dtype(dtype).name} [h,w{',3' if trailing else ''}] arrays, got {a.dtype} {a.shape}")
            sizes.append(a.shape[:2])
            offsets.append(at)
            at += a.shape[0] * a.shape[1]
        flat = np.concatenate([a.reshape(-1) for a in arrays]) if arrays else np.zeros(0, dtype)
        if dtype == np.uint16:
            flat = flat.view(np.int16)                       # the same bits; torch has no arithmetic on uint16 and needs none here
        return torch.from_numpy(flat).to(self.device), sizes, offsets

    def integrate(self, depth_u16, world_to_cam=None, cam_to_world=None, focals=None, ppx=None, ppy=None, rgb=None, depth_unit=0.001,
                  max_depth=4.0, frames_per_call=64, frustum_skip=True):
        """Fuse n depth images (raw uint16 sensor units; 0 = no measurement) seen from the given poses, in order. depth_u16 / rgb:
        one device tensor [n,h,w] / uint8 [n,h,w,3], or lists of per-frame numpy arrays whose sizes may differ from frame to frame
        (they are packed and uploaded here). focals, ppx, ppy: pixels of the depth image, one number or one per frame; the principal
        point defaults to the image centre (w / 2, h / 2). The result does not depend on frames_per_call."""
        n = len(depth_u16)
        if n == 0:
            return self
        if not 1 <= int(frames_per_call) <= N.TSDF_MAX_FRAMES:
            raise ValueError(f"frames_per_call must be in 1 .. {N.TSDF_MAX_FRAMES}")
        if focals is None:
            raise ValueError("focals is required")
        lib = N.lib()
        w2c = _w2c34(world_to_cam, cam_to_world, n)
        focals = _per_frame(focals, n)
        nx, ny, nz = self.dims
        for lo in range(0, n, int(frames_per_call)):
            hi = min(n, lo + int(frames_per_call))
            part = slice(lo, hi)
            d_depth, sizes, offsets = self._pack(depth_u16[part], np.uint16, ())
            d_rgb = None
            if rgb is not None:
                d_rgb, rgb_sizes, _ = self._pack(rgb[part], np.uint8, (3,))
                if rgb_sizes != sizes:
                    raise ValueError("every colour image must have its depth image's size")
            rows = (N.TsdfFrame * (hi - lo))()
            for r, f in enumerate(range(lo, hi)):
                h, w = sizes[r]
                rows[r].m[:] = w2c[f].reshape(12).tolist()
                rows[r].focal = float(focals[f])
                rows[r].ppx = float(_per_frame(ppx, n)[f]) if ppx is not None else w / 2.0
                rows[r].ppy = float(_per_frame(ppy, n)[f]) if ppy is not None else h / 2.0
                rows[r].h, rows[r].w, rows[r].offset = int(h), int(w), int(offsets[r])
            d_rows = torch.empty((hi - lo) * C.sizeof(N.TsdfFrame), dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                N.check(lib.acez_tsdf_integrate(_ptr(self.tsdf), _ptr(self.weight), _ptr(self.colour), nx, ny, nz, *self.origin,
                                                self.voxel_size, self.truncation, _ptr(d_depth), _ptr(d_rgb), d_depth.numel(), rows, hi - lo,
                                                _ptr(d_rows), float(depth_unit), float(max_depth), self.max_weight, int(bool(frustum_skip)),
                                                _stream()))
            self.frames_fused += hi - lo
        return self

    def known_voxels(self, min_weight):
        return int((self.weight >= float(min_weight)).sum().item())

    def extract_mesh(self, min_weight=2.0):
        """Naive surface nets over the voxels with weight >= min_weight: (vertices float32 [V,3], colours uint8 [V,3], faces int32
        [F,3]) as device tensors. Vertex ids ascend with the cell index, faces are axis-major, then ascend with the edge index: the
        mesh is a deterministic function of the volume. Triangle normals point to free space."""
        lib = N.lib()
        nx, ny, nz = self.dims
        dev, n_vox = self.device, nx * ny * nz
        vol = (_ptr(self.tsdf), _ptr(self.weight))
        with torch.cuda.device(dev):
            active = torch.empty(n_vox, dtype=torch.uint8, device=dev)
            cell_args = (*vol, _ptr(self.colour), nx, ny, nz, *self.origin, self.voxel_size, float(min_weight), _ptr(active))
            N.check(lib.acez_tsdf_cells(*cell_args, None, None, None, 0, _stream()))
            vrank = torch.cumsum(active, 0, dtype=torch.int32)
            n_v = int(vrank[-1].item())
            vertices = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
            colours = torch.empty((n_v, 3), dtype=torch.uint8, device=dev)
            N.check(lib.acez_tsdf_cells(*cell_args, _ptr(vrank), _ptr(vertices), _ptr(colours), n_v, _stream()))
            flags = torch.empty(3 * n_vox, dtype=torch.uint8, device=dev)
            face_args = (*vol, nx, ny, nz, float(min_weight), _ptr(active), _ptr(flags), _ptr(vrank))
            N.check(lib.acez_tsdf_faces(*face_args, None, None, 0, _stream()))
            erank = torch.cumsum(flags, 0, dtype=torch.int32)
            n_f = 2 * int(erank[-1].item())
            faces = torch.empty((n_f, 3), dtype=torch.int32, device=dev)
            N.check(lib.acez_tsdf_faces(*face_args, _ptr(erank), _ptr(faces), n_f, _stream()))
        return vertices, colours, faces


BLOCK = 8                                # a block of the sparse volume is 8 x 8 x 8 voxels (include/acez.h section K2)
BLOCK_VOXELS = BLOCK ** 3
MAX_GRID_BLOCKS = 2 ** 31                # the entry points refuse a block grid of this many entries or more
DENSE_LIMIT = (2 ** 31 - 1) // 3         # acez_tsdf_cells refuses more voxels than this


def block_grid(dims):
    """(bx, by, bz): blocks per axis of a virtual grid of dims voxels."""
    return tuple((int(d) + BLOCK - 1) // BLOCK for d in dims)


class SparseTSDFVolume:
    """TSDFVolume's function on a block-sparse volume (include/acez.h section K2): the grid of nx x ny x nz voxels is
    virtual, and only the 8^3-voxel blocks that mark() found near a surface are stored. First mark() every frame, then allocate(), then
    integrate() the same frames; extract_mesh() then gives TSDFVolume's mesh with its rows ordered by block.

        vol = SparseTSDFVolume(origin, (nx, ny, nz), voxel_size=0.01, truncation=0.04, device="cuda")
        vol.mark(depth_u16, cam_to_world=poses, focals=f)
        vol.allocate()
        vol.integrate(depth_u16, cam_to_world=poses, focals=f, rgb=rgb)
        vertices, colours, faces = vol.extract_mesh(min_weight=2)

    After allocate(): tsdf, weight [n_blocks,8,8,8] and colour [3,n_blocks,8,8,8] float32, block_table int32 [bz,by,bx] (slot or -1),
    slot_blocks int32 [n_blocks] (block index, ascending)."""

    _pack = TSDFVolume._pack

    def __init__(self, origin, dims, voxel_size, truncation, device, max_weight=64.0, max_blocks=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise _no_cpu("SparseTSDFVolume")
        self.origin = tuple(float(np.float32(o)) for o in origin)
        self.dims = tuple(int(d) for d in dims)
        self.voxel_size, self.truncation, self.max_weight = float(voxel_size), float(truncation), float(max_weight)
        self.max_blocks = None if max_blocks is None else int(max_blocks)
        self.device = device
        if min(self.dims) < 1:
            raise ValueError(f"volume dimensions {self.dims} must be at least 1")
        self.grid = block_grid(self.dims)
        n_grid = self.grid[0] * self.grid[1] * self.grid[2]
        if n_grid >= MAX_GRID_BLOCKS:
            raise ValueError(f"a block grid of {self.grid[0]} x {self.grid[1]} x {self.grid[2]} blocks is too large (2^31 or more)")
        self.block_flags = torch.zeros(n_grid, dtype=torch.uint8, device=device)
        self.allocated_blocks = None                         # the number of blocks, once allocate() has run
        self.block_table = self.slot_blocks = self.tsdf = self.weight = self.colour = None
        self.frames_fused = 0

    def _calls(self, depth_u16, world_to_cam, cam_to_world, focals, ppx, ppy, rgb, frames_per_call):
        """The frames cut into calls: yields (d_depth, d_rgb, table rows, device scratch for them, number of frames)."""
        n = len(depth_u16)
        if not 1 <= int(frames_per_call) <= N.TSDF_MAX_FRAMES:
            raise ValueError(f"frames_per_call must be in 1 .. {N.TSDF_MAX_FRAMES}")
        if focals is None:
            raise ValueError("focals is required")
        w2c = _w2c34(world_to_cam, cam_to_world, n)
        focals = _per_frame(focals, n)
        for lo in range(0, n, int(frames_per_call)):
            hi = min(n, lo + int(frames_per_call))
            part = slice(lo, hi)
            d_depth, sizes, offsets = self._pack(depth_u16[part], np.uint16, ())
            d_rgb = None
            if rgb is not None:
                d_rgb, rgb_sizes, _ = self._pack(rgb[part], np.uint8, (3,))
                if rgb_sizes != sizes:
                    raise ValueError("every colour image must have its depth image's size")
            rows = (N.TsdfFrame * (hi - lo))()
            for r, f in enumerate(range(lo, hi)):
                h, w = sizes[r]
                rows[r].m[:] = w2c[f].reshape(12).tolist()
                rows[r].focal = float(focals[f])
                rows[r].ppx = float(_per_frame(ppx, n)[f]) if ppx is not None else w / 2.0
                rows[r].ppy = float(_per_frame(ppy, n)[f]) if ppy is not None else h / 2.0
                rows[r].h, rows[r].w, rows[r].offset = int(h), int(w), int(offsets[r])
            d_rows = torch.empty((hi - lo) * C.sizeof(N.TsdfFrame), dtype=torch.uint8, device=self.device)
            yield d_depth, d_rgb, rows, d_rows, hi - lo

    def mark(self, depth_u16, world_to_cam=None, cam_to_world=None, focals=None, ppx=None, ppy=None, depth_unit=0.001, max_depth=4.0,
             frames_per_call=64):
        """Flag the blocks that the frames' depth puts near a surface (frame arguments as in integrate()). Any number of calls, all of
        them before allocate(): a block that appeared later would have missed the earlier frames' free-space updates, and the volume
        would no longer be the dense one."""
        if self.allocated_blocks is not None:
            raise ValueError("mark() after allocate(): a late block would have missed the earlier frames")
        if len(depth_u16) == 0:
            return self
        lib = N.lib()
        for d_depth, _, rows, d_rows, n in self._calls(depth_u16, world_to_cam, cam_to_world, focals, ppx, ppy, None, frames_per_call):
            with torch.cuda.device(self.device):
                N.check(lib.acez_tsdf_mark(_ptr(self.block_flags), *self.dims, *self.origin, self.voxel_size, self.truncation, _ptr(d_depth),
                                           d_depth.numel(), rows, n, _ptr(d_rows), float(depth_unit), float(max_depth), _stream()))
        return self

    def allocate(self):
        """Give every marked block a slot, in ascending block index, and clear the slots' storage; returns the number of blocks. One
        host synchronisation (the count)."""
        if self.allocated_blocks is not None:
            raise ValueError("allocate() was already called")
        rank = torch.cumsum(self.block_flags, 0, dtype=torch.int32)
        n = int(rank[-1].item())
        if self.max_blocks is not None and n > self.max_blocks:
            raise ValueError(f"{n} blocks are marked, more than max_blocks {self.max_blocks}")
        marked = self.block_flags != 0
        bx, by, bz = self.grid
        self.block_table = torch.where(marked, rank - 1, torch.full_like(rank, -1)).reshape(bz, by, bx)
        self.slot_blocks = torch.nonzero(marked).reshape(-1).to(torch.int32)
        if n:
            self.tsdf = torch.ones((n, BLOCK, BLOCK, BLOCK), dtype=torch.float32, device=self.device)
            self.weight = torch.zeros((n, BLOCK, BLOCK, BLOCK), dtype=torch.float32, device=self.device)
            self.colour = torch.zeros((3, n, BLOCK, BLOCK, BLOCK), dtype=torch.float32, device=self.device)
        self.allocated_blocks = n
        return n

    def _volume_args(self):
        return (*self.dims, *self.origin, self.voxel_size)

    def integrate(self, depth_u16, world_to_cam=None, cam_to_world=None, focals=None, ppx=None, ppy=None, rgb=None, depth_unit=0.001,
                  max_depth=4.0, frames_per_call=64, frustum_skip=True):
        """TSDFVolume.integrate on the allocated blocks: the same arguments, the same bits in every allocated voxel, whatever
        frames_per_call."""
        if self.allocated_blocks is None:
            raise ValueError("integrate() before allocate()")
        if len(depth_u16) == 0:
            return self
        lib = N.lib()
        for d_depth, d_rgb, rows, d_rows, n in self._calls(depth_u16, world_to_cam, cam_to_world, focals, ppx, ppy, rgb, frames_per_call):
            if self.allocated_blocks:
                with torch.cuda.device(self.device):
                    N.check(lib.acez_tsdf_integrate_blocks(_ptr(self.tsdf), _ptr(self.weight), _ptr(self.colour), _ptr(self.slot_blocks),
                                                           self.allocated_blocks, *self._volume_args(), self.truncation, _ptr(d_depth),
                                                           _ptr(d_rgb), d_depth.numel(), rows, n, _ptr(d_rows), float(depth_unit),
                                                           float(max_depth), self.max_weight, int(bool(frustum_skip)), _stream()))
            self.frames_fused += n
        return self

    def known_voxels(self, min_weight):
        if not self.allocated_blocks:
            return 0
        return int((self.weight >= float(min_weight)).sum().item())      # a partial block's voxels beyond the grid keep weight 0

    def extract_mesh(self, min_weight=2.0):
        """TSDFVolume.extract_mesh's mesh with another row order: vertex ids ascend by block index, then by the voxel index inside the
        block; faces are axis-major, then in that order. min_weight must be positive."""
        if self.allocated_blocks is None:
            raise ValueError("extract_mesh() before allocate()")
        if not float(min_weight) > 0:
            raise ValueError("min_weight must be positive: a voxel without a block counts as never observed")
        dev, n_b = self.device, self.allocated_blocks
        if n_b == 0:
            return (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.uint8, device=dev),
                    torch.empty((0, 3), dtype=torch.int32, device=dev))
        lib = N.lib()
        n_sv = n_b * BLOCK_VOXELS
        vol = (_ptr(self.tsdf), _ptr(self.weight))
        blocks = (_ptr(self.block_table), _ptr(self.slot_blocks), n_b)
        with torch.cuda.device(dev):
            active = torch.empty(n_sv, dtype=torch.uint8, device=dev)
            cell_args = (*vol, _ptr(self.colour), *blocks, *self._volume_args(), float(min_weight), _ptr(active))
            N.check(lib.acez_tsdf_cells_blocks(*cell_args, None, None, None, 0, _stream()))
            vrank = torch.cumsum(active, 0, dtype=torch.int32)
            n_v = int(vrank[-1].item())
            vertices = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
            colours = torch.empty((n_v, 3), dtype=torch.uint8, device=dev)
            N.check(lib.acez_tsdf_cells_blocks(*cell_args, _ptr(vrank), _ptr(vertices), _ptr(colours), n_v, _stream()))
            flags = torch.empty(3 * n_sv, dtype=torch.uint8, device=dev)
            face_args = (*vol, *blocks, *self.dims, float(min_weight), _ptr(active), _ptr(flags), _ptr(vrank))
            N.check(lib.acez_tsdf_faces_blocks(*face_args, None, None, 0, _stream()))
            erank = torch.cumsum(flags, 0, dtype=torch.int32)
            n_f = 2 * int(erank[-1].item())
            faces = torch.empty((n_f, 3), dtype=torch.int32, device=dev)
            N.check(lib.acez_tsdf_faces_blocks(*face_args, _ptr(erank), _ptr(faces), n_f, _stream()))
        return vertices, colours, faces

    def to_dense(self):
        """(tsdf, weight [nz,ny,nx], colour [3,nz,ny,nx]) as TSDFVolume holds them, voxels without a block cleared (tsdf 1, weight 0):
        for tests and small volumes; refused above the dense extraction's limit."""
        if self.allocated_blocks is None:
            raise ValueError("to_dense() before allocate()")
        nx, ny, nz = self.dims
        bx, by, bz = self.grid
        if bx * by * bz * BLOCK_VOXELS > DENSE_LIMIT:
            raise ValueError(f"a dense volume of {nx} x {ny} x {nz} voxels is too large")
        slots = self.slot_blocks.long()

        def scatter(storage, fill):
            rows = torch.full((bz * by * bx, BLOCK, BLOCK, BLOCK), fill, dtype=torch.float32, device=self.device)
            if self.allocated_blocks:
                rows[slots] = storage
            full = rows.reshape(bz, by, bx, BLOCK, BLOCK, BLOCK).permute(0, 3, 1, 4, 2, 5).reshape(bz * BLOCK, by * BLOCK, bx * BLOCK)
            return full[:nz, :ny, :nx].contiguous()

        n = self.allocated_blocks
        tsdf = scatter(self.tsdf if n else None, 1.0)
        weight = scatter(self.weight if n else None, 0.0)
        colour = torch.stack([scatter(self.colour[ch] if n else None, 0.0) for ch in range(3)])
        return tsdf, weight, colour


def bounds_from_frames(depth, cam_to_world, focals, voxel_size, truncation, depth_unit=0.001, max_depth=4.0, percentile=0.0, stride=8,
                       max_voxels=2 ** 28):
    """(origin float32 [3], dims (nx, ny, nz)) of the volume that holds the frames' depth: every stride-th pixel of every frame (list
    of uint16 [h,w] arrays) is back-projected with the frame's pose, focal and centred principal point; per axis the box runs from
    the `percentile`-th to the (100 - percentile)-th percentile of the points, is padded by the truncation and snapped outwards to
    multiples of the voxel size. Host numpy. A box of more than max_voxels voxels is refused, not coarsened."""
    n = len(depth)
    c2w = np.asarray(cam_to_world, np.float64).reshape(n, 4, 4)
    focals = _per_frame(focals, n)
    pts = []
    for f in range(n):
        d = np.asarray(depth[f])
        h, w = d.shape
        ys, xs = np.mgrid[stride // 2:h:stride, stride // 2:w:stride]
        z = d[ys, xs].astype(np.float64) * depth_unit
        ok = (z > 0) & (z <= max_depth)
        x = (xs[ok] - w / 2.0) / focals[f] * z[ok]
        y = (ys[ok] - h / 2.0) / focals[f] * z[ok]
        pts.append(np.stack([x, y, z[ok]], 1) @ c2w[f, :3, :3].T + c2w[f, :3, 3])
    pts = np.concatenate(pts, 0) if pts else np.zeros((0, 3))
    if len(pts) == 0:
        raise SystemExit("no valid depth within --max_depth in any frame: nothing to fuse")
    lo = np.percentile(pts, percentile, axis=0) - truncation
    hi = np.percentile(pts, 100.0 - percentile, axis=0) + truncation
    lo_i, hi_i = np.floor(lo / voxel_size).astype(np.int64), np.ceil(hi / voxel_size).astype(np.int64)
    dims = tuple(int(d) for d in hi_i - lo_i + 1)
    if dims[0] * dims[1] * dims[2] > max_voxels:
        raise SystemExit(f"the volume would have {dims[0]} x {dims[1]} x {dims[2]} = {dims[0] * dims[1] * dims[2]} voxels, more than "
                         f"--max_voxels {max_voxels}: raise --voxel_size, lower --max_depth or raise --max_voxels")
    return (lo_i * voxel_size).astype(np.float32), dims

