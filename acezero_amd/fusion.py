"""TSDF fusion of depth maps along estimated poses and the fused surface as a triangle mesh (include/acez.h section K, DESIGN.md
section 4j; fuse_depth.py is the command line).

    vol = TSDFVolume(origin, (nx, ny, nz), voxel_size=0.02, truncation=0.08, device="cuda")
    vol.integrate(depth_u16, cam_to_world=poses, focals=f, ppx=cx, ppy=cy, rgb=rgb)
    vertices, colours, faces = vol.extract_mesh(min_weight=2)
    formats.write_ply("scene.ply", vertices.cpu(), colours.cpu(), faces.cpu())

The volume lives in HBM; integration and extraction are HIP kernels (acezero_amd/csrc/fusion_api.hip). There is no CPU fallback.
SparseTSDFVolume is the same function on a block-sparse volume (section K2), for grids whose dense volume does not fit.

    poses, info, _ = vol.track(depth_u16, cam_to_world=poses, focals=f)              # section K3: frame-to-model refinement
    vol, poses, rounds = refine_poses(make_volume, depth_u16, poses, f, rounds=2)    # fuse, track, fuse again
"""
import numpy as np
import torch

from . import _native as N
from .frames import _per_frame, _w2c34, calls  # noqa: F401  (_w2c34: the tests restate poses through fusion._w2c34)
from ._device import no_cpu, ptr as _ptr, read_loops, stream as _stream


class _Volume:
    """What the dense and the block-sparse volume share: the grid, integrate()'s loop over the calls and the two-pass extraction. A
    subclass holds the storage (tsdf, weight, colour; None while it has none) and supplies _integrate_call, _track_accumulate,
    _elements, _cells and _faces."""

    def __init__(self, origin, dims, voxel_size, truncation, device, max_weight):
        device = torch.device(device)
        if device.type != "cuda":
            raise no_cpu(type(self).__name__, "TSDF fusion is a HIP kernel")
        self.origin = tuple(float(np.float32(o)) for o in origin)
        self.dims = tuple(int(d) for d in dims)
        self.voxel_size, self.truncation, self.max_weight = float(voxel_size), float(truncation), float(max_weight)
        self.device = device
        if min(self.dims) < 1:
            raise ValueError(f"volume dimensions {self.dims} must be at least 1")
        self.frames_fused = 0

    def _check_ready(self, what, min_weight=None):
        """Raises where `what` cannot run (yet); the dense volume always can."""

    def _grid_args(self):
        return (*self.dims, *self.origin, self.voxel_size)

    def integrate(self, depth_u16, world_to_cam=None, cam_to_world=None, focals=None, ppx=None, ppy=None, rgb=None, depth_unit=0.001,
                  max_depth=4.0, frames_per_call=64, frustum_skip=True):
        """Fuse n depth images (raw uint16 sensor units; 0 = no measurement) seen from the given poses, in order. depth_u16 / rgb:
        one device tensor [n,h,w] / uint8 [n,h,w,3], or lists of per-frame numpy arrays whose sizes may differ from frame to frame
        (they are packed and uploaded here). focals, ppx, ppy: pixels of the depth image, one number or one per frame; the principal
        point defaults to the image centre (w / 2, h / 2). The result does not depend on frames_per_call, and the sparse volume
        holds the dense one's bits in every allocated voxel."""
        self._check_ready("integrate")
        if len(depth_u16) == 0:
            return self
        for d_depth, d_rgb, rows, d_rows, n in calls(depth_u16, world_to_cam, cam_to_world, focals, ppx, ppy, rgb, frames_per_call, self.device):
            with torch.cuda.device(self.device):
                self._integrate_call(d_depth, d_rgb, rows, n, d_rows, float(depth_unit), float(max_depth), int(bool(frustum_skip)))
            self.frames_fused += n
        return self

    def known_voxels(self, min_weight):
        if self.weight is None:
            return 0
        return int((self.weight >= float(min_weight)).sum().item())      # a partial block's voxels beyond the grid keep weight 0

    def extract_mesh(self, min_weight=2.0):
        """Naive surface nets over the voxels with weight >= min_weight: (vertices float32 [V,3], colours uint8 [V,3], faces int32
        [F,3]) as device tensors. Vertex ids ascend with the stored element (dense: the cell index; sparse: the block index, then the
        voxel index inside the block), faces are axis-major, then in that order: the mesh is a deterministic function of the volume,
        and the sparse volume's is the dense one's with another row order. Triangle normals point to free space."""
        self._check_ready("extract_mesh", min_weight)
        dev, n_el = self.device, self._elements()
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        if n_el == 0:
            return new((0, 3), torch.float32), new((0, 3), torch.uint8), new((0, 3), torch.int32)
        with torch.cuda.device(dev):
            tail = (_stream(),)
            active = new(n_el, torch.uint8)
            N.check(self._cells(float(min_weight), _ptr(active), None, None, None, 0, *tail))
            vrank = torch.cumsum(active, 0, dtype=torch.int32)
            n_v = int(vrank[-1].item())
            vertices, colours = new((n_v, 3), torch.float32), new((n_v, 3), torch.uint8)
            N.check(self._cells(float(min_weight), _ptr(active), _ptr(vrank), _ptr(vertices), _ptr(colours), n_v, *tail))
            flags = new(3 * n_el, torch.uint8)
            N.check(self._faces(float(min_weight), _ptr(active), _ptr(flags), _ptr(vrank), None, None, 0, *tail))
            erank = torch.cumsum(flags, 0, dtype=torch.int32)
            n_f = 2 * int(erank[-1].item())
            faces = new((n_f, 3), torch.int32)
            N.check(self._faces(float(min_weight), _ptr(active), _ptr(flags), _ptr(vrank), _ptr(erank), _ptr(faces), n_f, *tail))
        return vertices, colours, faces

    def track(self, depth_u16, cam_to_world, focals, ppx=None, ppy=None, depth_unit=0.001, max_depth=4.0, min_weight=1.0,
              max_iterations=10, rel_rms=1e-6, damping=1e-4, min_count=64, frames_per_call=64):
        """Refine the frames' poses against this volume (include/acez.h section K3): per frame, damped
        Gauss-Newton on the trilinear SDF at its back-projected depth pixels. Frame arguments as in integrate(); cam_to_world [n,4,4]
        is taken in float64. Per call of frames_per_call frames the max_iterations ACCUMULATE + UPDATE launches are enqueued back to
        back: every frame's loop lives on the device, launches after it has stopped pass over it, and the host reads all states and
        histories back once at the end. Returns (cam_to_world float64 [n,4,4]; one dict per frame: status ("converged",
        "max_iterations" or "degenerate": too few pixels on known voxels near the surface, or a system that determines no step),
        iterations, count_first / count_last (pixels used) and rms_first / rms_last (metres) of its first and last record; the history
        float64 [n,max_iterations,16]: per record the pose it was taken under (12), count, sum r^2, rms, the status after it). The
        result does not depend on frames_per_call."""
        self._check_ready("track", min_weight)
        n, max_iterations = len(depth_u16), int(max_iterations)
        c2w = np.asarray(cam_to_world.detach().cpu().numpy() if torch.is_tensor(cam_to_world) else cam_to_world, np.float64).reshape(n, -1, 4)
        if max_iterations < 1:
            raise ValueError("max_iterations must be at least 1")
        states, histories = [], []
        for d_depth, _, rows, d_rows, k in calls(depth_u16, None, c2w, focals, ppx, ppy, None, frames_per_call, self.device):
            lo = sum(len(s) for s in states)
            tiles = max((rows[f].h * rows[f].w + TRACK_TILE - 1) // TRACK_TILE for f in range(k))
            state_h = np.zeros((k, TRACK_STATE))
            state_h[:, :12] = c2w[lo:lo + k, :3].reshape(k, 12)
            state = torch.from_numpy(state_h).to(self.device)
            partials = torch.empty((k, tiles, TRACK_TERMS), dtype=torch.float64, device=self.device)
            history = torch.zeros((k, max_iterations, TRACK_RECORD), dtype=torch.float64, device=self.device)
            with torch.cuda.device(self.device):
                lib, stream = N.lib(), _stream()
                for it in range(max_iterations):                       # the table is uploaded once; no synchronisation after that
                    self._track_accumulate(_ptr(d_depth), d_depth.numel(), rows, k, _ptr(d_rows), int(it == 0), float(depth_unit),
                                           float(max_depth), float(min_weight), _ptr(state), _ptr(partials), stream)
                    N.check(lib.acez_tsdf_track_update(_ptr(partials), tiles, _ptr(d_rows), k, float(rel_rms), float(damping), int(min_count),
                                                       max_iterations, _ptr(state), _ptr(history), stream))
            states.append(state)
            histories.append(history)
        if n == 0:
            return np.zeros((0, 4, 4)), [], np.zeros((0, max_iterations, TRACK_RECORD))
        state_h, history_h, status, done = read_loops(states, histories)                                        # the one read-back
        poses = np.tile(np.eye(4), (n, 1, 1))
        poses[:, :3] = state_h[:, :12].reshape(n, 3, 4)
        info = []
        for f in range(n):
            first, last = history_h[f, 0], history_h[f, max(done[f] - 1, 0)]
            info.append(dict(status=TRACK_STATUS[status[f]], iterations=int(done[f]), count_first=int(first[12]), count_last=int(last[12]),
                             rms_first=float(first[14]), rms_last=float(last[14])))
        return poses, info, history_h


TRACK_TILE, TRACK_TERMS, TRACK_STATE, TRACK_RECORD = 256, 29, 45, 16      # include/acez.h section K3
TRACK_STATUS = {0: "max_iterations", 1: "converged", 2: "degenerate"}


class TSDFVolume(_Volume):
    """nx x ny x nz voxels of `voxel_size` metres, voxel (0,0,0)'s centre at `origin` (world, OpenCV convention). tsdf, weight
    [nz,ny,nx] and colour [3,nz,ny,nx] are float32 device tensors; a voxel no frame has reached has weight 0."""

    def __init__(self, origin, dims, voxel_size, truncation, device, max_weight=64.0):
        super().__init__(origin, dims, voxel_size, truncation, device, max_weight)
        nx, ny, nz = self.dims
        self.tsdf = torch.ones((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.colour = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=self.device)

    def _integrate_call(self, d_depth, d_rgb, rows, n, d_rows, depth_unit, max_depth, frustum_skip):
        N.check(N.lib().acez_tsdf_integrate(_ptr(self.tsdf), _ptr(self.weight), _ptr(self.colour), *self._grid_args(), self.truncation,
                                            _ptr(d_depth), _ptr(d_rgb), d_depth.numel(), rows, n, _ptr(d_rows), depth_unit, max_depth,
                                            self.max_weight, frustum_skip, _stream()))

    def _track_accumulate(self, *tail):
        N.check(N.lib().acez_tsdf_track_accumulate(_ptr(self.tsdf), _ptr(self.weight), *self._grid_args(), self.truncation, *tail))

    def _elements(self):
        return self.dims[0] * self.dims[1] * self.dims[2]

    def _cells(self, *tail):
        return N.lib().acez_tsdf_cells(_ptr(self.tsdf), _ptr(self.weight), _ptr(self.colour), *self._grid_args(), *tail)

    def _faces(self, *tail):
        return N.lib().acez_tsdf_faces(_ptr(self.tsdf), _ptr(self.weight), *self.dims, *tail)


class TooManyBlocks(ValueError):
    """SparseTSDFVolume.allocate(): more blocks are marked than max_blocks allows."""


BLOCK = 8                                # a block of the sparse volume is 8 x 8 x 8 voxels (include/acez.h section K2)
BLOCK_VOXELS = BLOCK ** 3
MAX_GRID_BLOCKS = 2 ** 31                # the entry points refuse a block grid of this many entries or more
DENSE_LIMIT = (2 ** 31 - 1) // 3         # acez_tsdf_cells refuses more voxels than this


def block_grid(dims):
    """(bx, by, bz): blocks per axis of a virtual grid of dims voxels."""
    return tuple((int(d) + BLOCK - 1) // BLOCK for d in dims)


class SparseTSDFVolume(_Volume):
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

    def __init__(self, origin, dims, voxel_size, truncation, device, max_weight=64.0, max_blocks=None):
        super().__init__(origin, dims, voxel_size, truncation, device, max_weight)
        self.max_blocks = None if max_blocks is None else int(max_blocks)
        self.grid = block_grid(self.dims)
        n_grid = self.grid[0] * self.grid[1] * self.grid[2]
        if n_grid >= MAX_GRID_BLOCKS:
            raise ValueError(f"a block grid of {self.grid[0]} x {self.grid[1]} x {self.grid[2]} blocks is too large (2^31 or more)")
        self.block_flags = torch.zeros(n_grid, dtype=torch.uint8, device=self.device)
        self.allocated_blocks = None                         # the number of blocks, once allocate() has run
        self.block_table = self.slot_blocks = self.tsdf = self.weight = self.colour = None

    def _check_ready(self, what, min_weight=None):
        if self.allocated_blocks is None:
            raise ValueError(f"{what}() before allocate()")
        if min_weight is not None and not float(min_weight) > 0:
            raise ValueError("min_weight must be positive: a voxel without a block counts as never observed")

    def mark(self, depth_u16, world_to_cam=None, cam_to_world=None, focals=None, ppx=None, ppy=None, depth_unit=0.001, max_depth=4.0,
             frames_per_call=64):
        """Flag the blocks that the frames' depth puts near a surface (frame arguments as in integrate()). Any number of calls, all of
        them before allocate(): a block that appeared later would have missed the earlier frames' free-space updates, and the volume
        would no longer be the dense one."""
        if self.allocated_blocks is not None:
            raise ValueError("mark() after allocate(): a late block would have missed the earlier frames")
        if len(depth_u16) == 0:
            return self
        for d_depth, _, rows, d_rows, n in calls(depth_u16, world_to_cam, cam_to_world, focals, ppx, ppy, None, frames_per_call, self.device):
            with torch.cuda.device(self.device):
                N.check(N.lib().acez_tsdf_mark(_ptr(self.block_flags), *self._grid_args(), self.truncation, _ptr(d_depth), d_depth.numel(),
                                               rows, n, _ptr(d_rows), float(depth_unit), float(max_depth), _stream()))
        return self

    def allocate(self):
        """Give every marked block a slot, in ascending block index, and clear the slots' storage; returns the number of blocks. One
        host synchronisation (the count)."""
        if self.allocated_blocks is not None:
            raise ValueError("allocate() was already called")
        rank = torch.cumsum(self.block_flags, 0, dtype=torch.int32)
        n = int(rank[-1].item())
        if self.max_blocks is not None and n > self.max_blocks:
            raise TooManyBlocks(f"{n} blocks are marked, more than max_blocks {self.max_blocks}")
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

    def _integrate_call(self, d_depth, d_rgb, rows, n, d_rows, depth_unit, max_depth, frustum_skip):
        if not self.allocated_blocks:                        # nothing to update; the frames still count
            return
        N.check(N.lib().acez_tsdf_integrate_blocks(_ptr(self.tsdf), _ptr(self.weight), _ptr(self.colour), _ptr(self.slot_blocks),
                                                   self.allocated_blocks, *self._grid_args(), self.truncation, _ptr(d_depth), _ptr(d_rgb),
                                                   d_depth.numel(), rows, n, _ptr(d_rows), depth_unit, max_depth, self.max_weight,
                                                   frustum_skip, _stream()))

    def _track_accumulate(self, *tail):
        N.check(N.lib().acez_tsdf_track_accumulate_blocks(_ptr(self.tsdf), _ptr(self.weight), _ptr(self.block_table), _ptr(self.slot_blocks),
                                                          self.allocated_blocks, *self._grid_args(), self.truncation, *tail))

    def _elements(self):
        return self.allocated_blocks * BLOCK_VOXELS

    def _cells(self, *tail):
        return N.lib().acez_tsdf_cells_blocks(_ptr(self.tsdf), _ptr(self.weight), _ptr(self.colour), _ptr(self.block_table),
                                              _ptr(self.slot_blocks), self.allocated_blocks, *self._grid_args(), *tail)

    def _faces(self, *tail):
        return N.lib().acez_tsdf_faces_blocks(_ptr(self.tsdf), _ptr(self.weight), _ptr(self.block_table), _ptr(self.slot_blocks),
                                              self.allocated_blocks, *self.dims, *tail)

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


def fuse(make_volume, depth, cam_to_world, focals, ppx=None, ppy=None, rgb=None, depth_unit=0.001, max_depth=4.0):
    """A fresh volume from make_volume() with the frames fused into it; a sparse volume is marked and allocated first."""
    vol = make_volume()
    if isinstance(vol, SparseTSDFVolume):
        vol.mark(depth, cam_to_world=cam_to_world, focals=focals, ppx=ppx, ppy=ppy, depth_unit=depth_unit, max_depth=max_depth)
        vol.allocate()
    return vol.integrate(depth, cam_to_world=cam_to_world, focals=focals, ppx=ppx, ppy=ppy, rgb=rgb, depth_unit=depth_unit, max_depth=max_depth)


def refine_poses(make_volume, depth, cam_to_world, focals, ppx=None, ppy=None, rgb=None, rounds=1, depth_unit=0.001, max_depth=4.0,
                 **track_args):
    """Alternate fusion and tracking `rounds` times: fuse the frames under the current poses into a fresh volume
    from make_volume() (without colour), track every frame against it (track_args: _Volume.track's keywords), take the tracked poses
    except for the frames that ended degenerate, which keep the pose they entered the round with; then fuse once more, with colour,
    under the final poses. Returns (that volume, cam_to_world float64 [n,4,4], per round a dict: info (track's list), poses, converged,
    degenerate, out_of_iterations (frame counts), rms_before, rms_after (metres, means over the frames that are not degenerate, nan
    if there is none) and pixels (mean pixels used))."""
    n = len(depth)
    poses = np.array(np.asarray(cam_to_world, np.float64).reshape(n, 4, 4))
    frames = dict(focals=focals, ppx=ppx, ppy=ppy, depth_unit=depth_unit, max_depth=max_depth)
    stats = []
    for _ in range(int(rounds)):
        vol = fuse(make_volume, depth, poses, rgb=None, **frames)
        tracked, info, _ = vol.track(depth, poses, **frames, **track_args)
        del vol
        good = np.array([i["status"] != "degenerate" for i in info], bool)
        poses[good] = tracked[good]
        mean = lambda key: float(np.mean([i[key] for i, g in zip(info, good) if g])) if good.any() else float("nan")
        stats.append(dict(info=info, poses=poses.copy(), converged=sum(i["status"] == "converged" for i in info), degenerate=int((~good).sum()),
                          out_of_iterations=sum(i["status"] == "max_iterations" for i in info), rms_before=mean("rms_first"),
                          rms_after=mean("rms_last"), pixels=mean("count_last")))
    return fuse(make_volume, depth, poses, rgb=rgb, **frames), poses, stats


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

