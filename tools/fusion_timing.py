"""TSDF fusion on the box: the integration kernel with and without its frustum skip, the extraction, and fuse_depth.py as a whole
(DESIGN.md section 4j). HIP events around each call, median of the repetitions.

    python tools/fusion_timing.py [--frames 48] [--dim 256] [--reps 10] [--no_cli] [--sparse_only] [--voxel 0.02]

The scene is the analytic box room of tests/fusion_cases.py scaled to fill the volume, 640 x 480 depth at a Kinect's focal length,
the cameras on a small circle looking outwards, so that a frame sees about a sixth of the volume. The frames are on the device
before the timed calls: `integrate` times the table copy and the kernel. The bound printed beside it is the traffic of one pass over
the volume (tsdf, weight and three colour planes read and written: 40 bytes per voxel) at 6.3 TB/s, the streaming rate measured on
this chip. The sparse leg (fusion.SparseTSDFVolume) fuses the same frames into the same grid: mark, allocate (with its host
synchronisation, wall clock around a device synchronisation), integrate and extract, and the allocated blocks and bytes beside the
dense volume's. --sparse_only --voxel V runs that leg alone on the same room at another voxel size (the grid is then side / V
voxels wide): a grid the dense volume cannot hold. Prints one JSON line."""
import argparse
import json
import logging
import os
import re
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acezero_amd import cli, fusion  # noqa: E402
from tests import fusion_cases as FC  # noqa: E402
from tools.rgbd_timing import _time  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no_cli", action="store_true")
    ap.add_argument("--sparse_only", action="store_true")
    ap.add_argument("--voxel", type=float, default=0.02, help="voxel size of the sparse leg; the room keeps its size")
    a = ap.parse_args()
    n, dim, v, h, w, focal = a.frames, a.dim, 0.02, 480, 640, 525.0
    side = dim * v
    half = np.array([0.47, 0.31, 0.47]) * side                    # the room's walls lie inside the volume, a truncation from its faces
    c2w = FC.room_cameras(n, radius=0.1 * side)
    depth = np.stack([FC.room_depth(T, h, w, focal, half) for T in c2w])
    rgb = np.stack([FC.room_rgb(T, h, w, focal, half) for T in c2w])
    d_depth = torch.from_numpy(depth.view(np.int16)).cuda()
    d_rgb = torch.from_numpy(rgb).cuda()
    origin = (-0.5 * side + 0.5 * v,) * 3
    n_vox = dim ** 3
    out = {"frames": n, "volume": f"{dim}^3", "depth": f"{w}x{h}", "reps": a.reps,
           "pass_bound_ms": round(40.0 * n_vox / HBM_BYTES_PER_S * 1e3, 4)}

    def fresh():
        return fusion.TSDFVolume(origin, (dim, dim, dim), v, 4 * v, "cuda")

    def sparse_leg():
        sv = a.voxel
        sdim = int(round(side / sv))
        s_origin = (-0.5 * side + 0.5 * sv,) * 3
        frames = dict(cam_to_world=c2w, focals=focal, max_depth=0.75 * side)
        out["sparse_grid"], out["sparse_voxel_size"] = f"{sdim}^3", sv

        def marked():
            return fusion.SparseTSDFVolume(s_origin, (sdim, sdim, sdim), sv, 4 * sv, "cuda")

        svol = marked()
        out["sparse_mark_ms"] = _time(lambda: svol.mark(d_depth, frames_per_call=n, **frames), a.reps)
        times = []
        for _ in range(a.reps):
            svol = marked().mark(d_depth, frames_per_call=n, **frames)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            svol.allocate()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        out["sparse_allocate_ms"] = float(np.median(times))
        n_grid = svol.grid[0] * svol.grid[1] * svol.grid[2]
        out["sparse_blocks"], out["sparse_grid_blocks"] = svol.allocated_blocks, n_grid
        out["sparse_bytes"] = svol.allocated_blocks * fusion.BLOCK_VOXELS * 20 + n_grid * 5
        out["dense_bytes_same_grid"] = sdim ** 3 * 20
        for per_call in (n, 1):
            ms = _time(lambda: svol.integrate(d_depth, rgb=d_rgb, frames_per_call=per_call, **frames), a.reps)
            out[f"sparse_integrate_{'one_call' if per_call == n else 'call_per_frame'}_ms_per_frame"] = ms / n
        svol = marked().mark(d_depth, frames_per_call=n, **frames)
        svol.allocate()
        svol.integrate(d_depth, rgb=d_rgb, **frames)
        out["sparse_extract_ms"] = _time(lambda: svol.extract_mesh(2.0), a.reps)
        vert, _, faces = svol.extract_mesh(2.0)
        out["sparse_vertices"], out["sparse_faces"] = int(vert.shape[0]), int(faces.shape[0])
        out["sparse_peak_device_bytes"] = int(torch.cuda.max_memory_allocated())

    if a.sparse_only:
        sparse_leg()
        print(json.dumps({k: (float(f"{x:.4g}") if isinstance(x, float) else x) for k, x in out.items()}))
        return
    vol = fresh()
    for name, kw in (("skip", dict(frustum_skip=True)), ("noskip", dict(frustum_skip=False))):
        for per_call in (n, 1):
            def run():
                vol.integrate(d_depth, cam_to_world=c2w, focals=focal, rgb=d_rgb, max_depth=0.75 * side, frames_per_call=per_call, **kw)
            ms = _time(run, a.reps)
            tag = f"integrate_{name}_{'one_call' if per_call == n else 'call_per_frame'}"
            out[f"{tag}_ms_per_frame"] = ms / n
            out[f"{tag}_voxel_frames_per_s"] = n_vox * n / (ms * 1e-3)
    vol = fresh().integrate(d_depth, cam_to_world=c2w, focals=focal, rgb=d_rgb, max_depth=0.75 * side)
    out["touched_voxels"] = int((vol.weight > 0).sum().item())
    out["extract_ms"] = _time(lambda: vol.extract_mesh(2.0), a.reps)
    vert, _, faces = vol.extract_mesh(2.0)
    out["vertices"], out["faces"] = int(vert.shape[0]), int(faces.shape[0])
    del vol
    sparse_leg()
    t0 = time.perf_counter()
    torch.from_numpy(depth.view(np.int16)).cuda(), torch.from_numpy(rgb).cuda()
    torch.cuda.synchronize()
    out["upload_s"] = time.perf_counter() - t0
    if not a.no_cli:
        with tempfile.TemporaryDirectory() as tmp:
            args = FC.write_room_scene(tmp, n, h, w, focal, rgb_scale=1)          # (the small room: what is timed is the file path)
            lines = []
            handler = logging.Handler()
            handler.emit = lambda record: lines.append(record.getMessage())
            logging.getLogger("fuse_depth").addHandler(handler)
            t0 = time.perf_counter()
            cli.fuse_depth_main(args)
            out["cli_total_s"] = time.perf_counter() - t0
            m = re.search(r"Decode ([\d.]+) s, upload \+ kernels \+ download ([\d.]+) s, write ([\d.]+) s", "\n".join(lines))
            out["cli_decode_s"], out["cli_device_s"], out["cli_write_s"] = (float(g) for g in m.groups())
            out["cli_log"] = [ln for ln in lines if "voxels" in ln]
    print(json.dumps({k: (float(f"{x:.4g}") if isinstance(x, float) else x) for k, x in out.items()}))


if __name__ == "__main__":
    main()
