"""Dense depth for RGB reconstructions by plane-sweep stereo over neighbouring frames (include/acez.h section L, DESIGN.md section 4k;
estimate_depth.py is the command line).

    sources = select_sources(cam_to_world, focals, sizes, scene_depth, 4)
    maps = estimate_depth_maps(grey_images, cam_to_world=cam_to_world, focals=focals, sources=sources, ranges=ranges)

The result is one uint16 depth map per frame in the units acezero_amd.fusion takes. Prefilter, sweep and consistency check are HIP
kernels (acezero_amd/csrc/mvs_api.hip). There is no CPU fallback. This is classical multi-view stereo, not a learned one.

aggregation="sgm" (include/acez.h section M) replaces a frame's sweep by cost volume -> semi-global aggregation -> plane selection,
three more HIP kernels of the same unit: textureless surfaces inherit the depth of the texture around them."""
import concurrent.futures
import ctypes as C

import numpy as np
import torch

from . import _native as N
from .frames import device_rows, frame_rows, pack
from ._device import ptr as _ptr, stream as _stream

MAX_AXIS_ANGLE_DEG = 30.0           # select_sources: a source looks within this angle of the frame's own optical axis
BASELINE_RATIO = (0.02, 0.5)        # ... and stands this far away, in units of the scene depth
BEST_BASELINE_RATIO = 0.1           # ... preferably this far
MIN_CLOUD_POINTS = 16               # depth_range_from_cloud: fewer points inside the frame give no range
RANGE_MARGIN = 1.25
SWEEP_STREAMS = 4                   # StereoFrames.sweep_frames: reference frames swept side by side
SGM_PATHS = 4                       # aggregation="sgm": the default path count and the default penalties per sample of a cost
SGM_P1_PER_SAMPLE = 1.6             # ... (a cost sums n = keep * (2 * window + 1)^2 samples); DESIGN.md section 4k has the grid
SGM_P2_PER_SAMPLE = 12.8            # ... they were chosen from


def sgm_penalties(keep, window, p1=None, p2=None):
    """(P1, P2) of the aggregation: what was given, else the per-sample defaults times n = keep * (2 * window + 1)^2, at least 1 and
    at most 32767, so that changing the window does not silently change the smoothing. A default gives way to a given value: a
    default P1 is at most the given P2, a default P2 at least the given P1 (a frame with fewer sources has a smaller default)."""
    n = int(keep) * (2 * int(window) + 1) ** 2
    d1, d2 = min(max(int(round(SGM_P1_PER_SAMPLE * n)), 1), 32767), min(max(int(round(SGM_P2_PER_SAMPLE * n)), 1), 32767)
    if p1 is None and p2 is None:
        return min(d1, d2), d2
    if p1 is None:
        return min(d1, int(p2)), int(p2)
    if p2 is None:
        return int(p1), max(d2, int(p1))
    return int(p1), int(p2)


class SgmScratch:
    """The scratch of one stream: the cost volume (uint16 bits) and S (uint32 bits) of the largest frame it will see."""

    def __init__(self, elements, device):
        self.elements = int(elements)
        self.volume = torch.empty(self.elements, dtype=torch.int16, device=device)
        self.s = torch.empty(self.elements, dtype=torch.int32, device=device)

    @staticmethod
    def nbytes(elements):
        return 6 * int(elements)


def select_sources(c2w, focals, sizes, scene_depth, n_sources):
    """For every frame the up to n_sources other frames to match it against, best first (host numpy). c2w [n,4,4] camera -> world; a
    frame without a usable pose has a non-finite one and neither gets nor serves as a source. A candidate's optical axis is within
    30 degrees of the frame's own and its baseline / scene_depth (one number, or one per frame) within [0.02, 0.5]; candidates are
    ordered by |ratio - 0.1|, ties by frame index. focals and sizes ([(h, w)]) are part of the signature for rankings that weigh
    the overlap; this one does not read them. Returns a list of n lists of frame indices; an empty one means no depth map."""
    c2w = np.asarray(c2w, np.float64).reshape(-1, 4, 4)
    n = len(c2w)
    depth = np.broadcast_to(np.asarray(scene_depth, np.float64), (n,))
    posed = np.isfinite(c2w).all((1, 2))
    axis, centre = c2w[:, :3, 2], c2w[:, :3, 3]
    out = []
    for i in range(n):
        ranked = []
        if posed[i] and np.isfinite(depth[i]) and depth[i] > 0:
            for j in range(n):
                if j == i or not posed[j]:
                    continue
                cos = float(axis[i] @ axis[j]) / float(np.linalg.norm(axis[i]) * np.linalg.norm(axis[j]))
                ratio = float(np.linalg.norm(centre[j] - centre[i])) / float(depth[i])
                if cos >= np.cos(np.radians(MAX_AXIS_ANGLE_DEG)) and BASELINE_RATIO[0] <= ratio <= BASELINE_RATIO[1]:
                    ranked.append((abs(ratio - BEST_BASELINE_RATIO), j))
        out.append([j for _, j in sorted(ranked)[:int(n_sources)]])
    return out


def depth_range_from_cloud(points, w2c, focal, ppx, ppy, h, w):
    """(near, far) of a frame from a point cloud [m,3] in world coordinates: the 1st and 99th percentile of camera z over the points
    that project inside the frame (section K's pixel convention), widened by 1 / 1.25 and 1.25. None if fewer than 16 points do."""
    m = np.asarray(w2c, np.float64)[:3]
    cam = np.asarray(points, np.float64).reshape(-1, 3) @ m[:, :3].T + m[:, 3]
    z = cam[:, 2]
    with np.errstate(all="ignore"):
        u, v = focal * cam[:, 0] / z + ppx, focal * cam[:, 1] / z + ppy
        inside = (z > 0) & (u >= -0.5) & (u < w - 0.5) & (v >= -0.5) & (v < h - 0.5)
    if int(inside.sum()) < MIN_CLOUD_POINTS:
        return None
    near, far = np.percentile(z[inside], [1.0, 99.0])
    return float(near / RANGE_MARGIN), float(far * RANGE_MARGIN)


def load_grey_frames(files, image_resolution, workers=12):
    """Decode in a pool of threads (ingest.decode_frames), resize so that the short side is image_resolution and convert to grey,
    both as cli.load_frames does (Pillow bilinear, convert('L')): (list of uint8 [h,w], list of the files' original heights)."""
    from PIL import Image
    from .ingest import decode_frames, pool_size, resized_size
    decoded = decode_frames(files, workers)

    def small(a):
        _, nh, nw = resized_size(a.shape[1], a.shape[0], image_resolution)
        return np.ascontiguousarray(np.asarray(Image.fromarray(a).resize((nw, nh), Image.BILINEAR).convert("L"), np.uint8))
    with concurrent.futures.ThreadPoolExecutor(max_workers=pool_size(workers)) as pool:
        return list(pool.map(small, decoded)), [a.shape[0] for a in decoded]


class StereoFrames:
    """The frames of one estimate on the device: `grey`, `filtered` uint8, `depth` float32, `cost`, `plane` int32 and `out` int16
    (the uint16 bits), each one packed buffer of n_pixels elements, and the host table of rows (offset, size, pose, intrinsics)."""

    def __init__(self, images, world_to_cam=None, cam_to_world=None, focals=None, ppx=None, ppy=None, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("plane-sweep stereo needs a GPU: prefilter, sweep and check are HIP kernels, there is no CPU path")
        if focals is None:
            raise ValueError("focals is required")
        self.device = device
        self.grey, self.sizes, self.offsets = pack(images, np.uint8, (), device)
        self.n, self.n_pixels = len(self.sizes), int(self.grey.numel())
        self.rows = frame_rows(self.sizes, self.offsets, world_to_cam, cam_to_world, focals, ppx, ppy, length=max(self.n, 1))
        new = lambda dtype: torch.zeros(self.n_pixels, dtype=dtype, device=device)
        self.filtered, self.depth, self.cost, self.plane, self.out = new(torch.uint8), new(torch.float32), new(torch.int32), new(torch.int32), new(torch.int16)
        self._d_rows = device_rows(max(self.n, 1), device)

    def prefilter(self):
        with torch.cuda.device(self.device):
            N.check(N.lib().acez_mvs_prefilter(_ptr(self.grey), _ptr(self.filtered), self.n_pixels, self.rows, self.n, _ptr(self._d_rows), _stream()))
        return self

    def sweep(self, ref, sources, z_near, z_far, planes=128, window=2, truncation=40, keep=None, uniqueness=5):
        """The depth map of frame `ref` into `depth` (and C(k*), k* into `cost`, `plane`); keep defaults to ceil(sources / 2)."""
        src = (C.c_int32 * max(len(sources), 1))(*[int(s) for s in sources])
        keep = -(-len(sources) // 2) if keep is None else int(keep)
        with torch.cuda.device(self.device):
            N.check(N.lib().acez_mvs_sweep(_ptr(self.filtered), self.n_pixels, self.rows, self.n, int(ref), src, len(sources), float(z_near),
                                           float(z_far), int(planes), int(window), int(truncation), keep, int(uniqueness), _ptr(self.depth),
                                           _ptr(self.cost), _ptr(self.plane), _stream()))
        return self

    def volume(self, ref, sources, z_near, z_far, scratch, planes=128, window=2, truncation=40, keep=None):
        """Section M's VOLUME of frame `ref` into scratch.volume."""
        src = (C.c_int32 * max(len(sources), 1))(*[int(s) for s in sources])
        keep = -(-len(sources) // 2) if keep is None else int(keep)
        with torch.cuda.device(self.device):
            N.check(N.lib().acez_mvs_volume(_ptr(self.filtered), self.n_pixels, self.rows, self.n, int(ref), src, len(sources), float(z_near),
                                            float(z_far), int(planes), int(window), int(truncation), keep, _ptr(scratch.volume), scratch.elements,
                                            _stream()))
        return self

    def aggregate(self, ref, scratch, planes, paths, p1, p2, direction=0):
        """Section M's AGGREGATE of scratch.volume (frame `ref`'s) into scratch.s, which is zeroed first."""
        h, w = self.sizes[ref]
        with torch.cuda.device(self.device):
            scratch.s[:h * w * int(planes)].zero_()
            N.check(N.lib().acez_mvs_aggregate(_ptr(scratch.volume), _ptr(scratch.s), scratch.elements, int(h), int(w), int(planes), int(paths),
                                               int(direction), int(p1), int(p2), _stream()))
        return self

    def select(self, ref, z_near, z_far, scratch, planes=128, uniqueness=5, aggregated=True):
        """Section M's SELECT into `depth`, `cost`, `plane`: on scratch.s, or on the volume's own costs (aggregated=False)."""
        with torch.cuda.device(self.device):
            N.check(N.lib().acez_mvs_select(_ptr(scratch.volume), _ptr(scratch.s) if aggregated else None, scratch.elements, self.n_pixels,
                                            self.rows, self.n, int(ref), float(z_near), float(z_far), int(planes), int(uniqueness),
                                            _ptr(self.depth), _ptr(self.cost), _ptr(self.plane), _stream()))
        return self

    def sweep_frames(self, jobs, planes=128, window=2, truncation=40, uniqueness=5, streams=SWEEP_STREAMS, aggregation=None, sgm_paths=None,
                     sgm_p1=None, sgm_p2=None):
        """sweep() for every (ref, sources, z_near, z_far, keep) of jobs. A frame's sweep is 20 x 15 workgroups at 240 x 320 px, about
        one wave per SIMD, so the launches go round-robin to `streams` streams that start after the current stream's work (the
        prefilter) and that the current stream then waits for. The frames write disjoint parts of the buffers: the same bits.
        aggregation="sgm": a frame runs volume -> aggregate -> select on its stream instead, in scratch that is allocated once per
        stream (SgmScratch, 6 bytes per pixel and plane of the largest frame); penalties default to sgm_penalties() of each frame."""
        if aggregation not in (None, "none", "sgm"):
            raise ValueError(f"aggregation must be None or 'sgm', got {aggregation!r}")
        sgm = aggregation == "sgm"
        paths = SGM_PATHS if sgm_paths is None else int(sgm_paths)
        if sgm and paths not in (4, 8):
            raise ValueError("sgm_paths must be 4 or 8")
        if not jobs:
            return self
        main = torch.cuda.current_stream(self.device)
        side = [torch.cuda.Stream(self.device) for _ in range(max(1, min(int(streams), len(jobs))))]
        if sgm:
            elements = max(self.sizes[job[0]][0] * self.sizes[job[0]][1] for job in jobs) * int(planes)
            self.sgm_scratch_bytes = len(side) * SgmScratch.nbytes(elements)
            scratch = [SgmScratch(elements, self.device) for _ in side]
        for s in side:
            s.wait_stream(main)
        for i, (ref, sources, z_near, z_far, keep) in enumerate(jobs):
            with torch.cuda.stream(side[i % len(side)]):
                if sgm:
                    keep_f = -(-len(sources) // 2) if keep is None else int(keep)
                    p1, p2 = sgm_penalties(keep_f, window, sgm_p1, sgm_p2)
                    sc = scratch[i % len(side)]
                    self.volume(ref, sources, z_near, z_far, sc, planes, window, truncation, keep_f)
                    self.aggregate(ref, sc, planes, paths, p1, p2)
                    self.select(ref, z_near, z_far, sc, planes, uniqueness)
                else:
                    self.sweep(ref, sources, z_near, z_far, planes, window, truncation, keep, uniqueness)
        for s in side:
            main.wait_stream(s)
        return self

    def check(self, ref, sources, tolerance=0.01, min_consistent=2, depth_unit=0.001):
        src = (C.c_int32 * max(len(sources), 1))(*[int(s) for s in sources])
        with torch.cuda.device(self.device):
            N.check(N.lib().acez_mvs_check(_ptr(self.depth), self.n_pixels, self.rows, self.n, int(ref), src, len(sources), float(tolerance),
                                           int(min_consistent), float(depth_unit), _ptr(self.out), _stream()))
        return self

    def frame(self, buffer, f):
        """Frame f of one of the packed buffers as a host array [h,w] (`out` as uint16)."""
        h, w = self.sizes[f]
        a = buffer[self.offsets[f]:self.offsets[f] + h * w].reshape(h, w).cpu().numpy()
        return a.view(np.uint16) if a.dtype == np.int16 else a


def estimate_depth_maps(images, world_to_cam=None, cam_to_world=None, focals=None, ppx=None, ppy=None, sources=None, ranges=None, planes=128,
                        window=2, truncation=40, keep=None, uniqueness=5, tolerance=0.01, min_consistent=2, depth_unit=0.001, device="cuda",
                        aggregation=None, sgm_paths=None, sgm_p1=None, sgm_p2=None, info=None):
    """One uint16 depth map [h,w] per frame (0 = no depth), in units of depth_unit metres. images: a uint8 device tensor [n,h,w] or a
    list of uint8 [h,w] host arrays whose sizes may differ (grey). sources: select_sources' lists; ranges: per frame (near, far) or
    None. A frame without sources or range gets an all-zero map. keep: None = ceil(sources / 2) of each frame, else capped at the
    frame's number of sources. Upload, prefilter once, sweep every frame, check every frame, download. aggregation="sgm": every
    frame's costs are aggregated along sgm_paths (4 or 8) scanline directions with the penalties sgm_p1 <= sgm_p2 before the plane is
    chosen (section M; defaults: SGM_PATHS and sgm_penalties()); the check is unchanged. info: a dict that receives
    "sgm_scratch_bytes"."""
    if sources is None or ranges is None:
        raise ValueError("sources and ranges are required")
    fs = StereoFrames(images, world_to_cam, cam_to_world, focals, ppx, ppy, device)
    live = [f for f in range(fs.n) if len(sources[f]) and ranges[f] is not None]
    if live:
        fs.prefilter()
    fs.sweep_frames([(f, sources[f], ranges[f][0], ranges[f][1], None if keep is None else min(int(keep), len(sources[f]))) for f in live],
                    planes, window, truncation, uniqueness, aggregation=aggregation, sgm_paths=sgm_paths, sgm_p1=sgm_p1, sgm_p2=sgm_p2)
    if info is not None:
        info["sgm_scratch_bytes"] = getattr(fs, "sgm_scratch_bytes", 0)
    for f in live:
        fs.check(f, sources[f], tolerance, min_consistent, depth_unit)
    torch.cuda.synchronize(fs.device)
    return [fs.frame(fs.out, f) for f in range(fs.n)]
