"""Mesh rendering on the box: acez_meshrender on the meshes fuse_depth.py produces, for depth only and for all
planes, one call for all frames and one call per frame, beside the video rasteriser (acez_render_frame: one wavefront per triangle)
on the same triangles. HIP events around each call, median of the repetitions; mesh and frames are on the device before the timed calls.

    python tools/mesh_render_timing.py --mesh room|simplified|box [--frames 48] [--dim 256] [--sparse_voxel 0.0075] [--reps 10]
    python tools/mesh_render_timing.py --all          # every mesh in a fresh process under its own time limit, stopping at a failure

Meshes: the room of tools/fusion_timing.py fused into the block-sparse volume at --sparse_voxel (3.56 M faces at 7.5 mm), its
simplification at three voxels (22.5 mm), and the room's 12 exact triangles. Frames: 640 x 480 at a Kinect's focal length from the
fusing cameras. The yardstick renders ONE frame of the same triangles as a soup with the flat triangle layer of acez_render_frame,
whose yfov = pi / 3 camera stands at the first frame's pose (it sees a little more of the room: focal 416 px instead of 525). The
bytes beside the times are what one frame must move at least: the indices and vertices once, and the keys cleared, hit and read
(24 bytes per pixel). Prints one JSON line per mesh."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acezero_amd import _native as N  # noqa: E402
from acezero_amd import fusion, meshrender, simplify  # noqa: E402
from acezero_amd._device import ptr as _ptr, stream as _stream  # noqa: E402
from tests import fusion_cases as FC  # noqa: E402
from tools.rgbd_timing import _time  # noqa: E402

MESHES = ("box", "simplified", "room")
LIMIT_S = {"box": 240, "simplified": 400, "room": 500}
ALL_PLANES = ("depth", "face", "depth_u16", "normal", "colour")


def box_mesh(half):
    v = np.array([[sx * half[0], sy * half[1], sz * half[2]] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float32)
    walls = [(0, 2, 6, 4), (1, 3, 7, 5), (0, 1, 5, 4), (2, 3, 7, 6), (0, 1, 3, 2), (4, 5, 7, 6)]
    faces = np.array([t for a, b, c, d in walls for t in ((a, b, c), (a, c, d))], np.int32)
    return torch.from_numpy(v).cuda(), torch.full((8, 3), 200, dtype=torch.uint8, device="cuda"), torch.from_numpy(faces).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", choices=MESHES, default="room")
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--sparse_voxel", type=float, default=0.0075)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if a.all:
        for name in MESHES:
            cmd = [sys.executable, os.path.abspath(__file__), "--mesh", name, "--frames", str(a.frames), "--dim", str(a.dim), "--sparse_voxel",
                   str(a.sparse_voxel), "--reps", str(a.reps)]
            r = subprocess.run(cmd, timeout=LIMIT_S[name])
            if r.returncode != 0:
                return r.returncode
        return 0
    n, dim, v, h, w, focal = a.frames, a.dim, 0.02, 480, 640, 525.0
    side = dim * v
    half = np.array([0.47, 0.31, 0.47]) * side
    c2w = FC.room_cameras(n, radius=0.1 * side)
    if a.mesh == "box":
        vertices, colours, faces = box_mesh(half)
    else:
        depth = np.stack([FC.room_depth(T, h, w, focal, half) for T in c2w])
        rgb = np.stack([FC.room_rgb(T, h, w, focal, half) for T in c2w])
        d_depth, d_rgb = torch.from_numpy(depth.view(np.int16)).cuda(), torch.from_numpy(rgb).cuda()
        frames = dict(cam_to_world=c2w, focals=focal, max_depth=0.75 * side)
        sv = a.sparse_voxel
        sdim = int(round(side / sv))
        svol = fusion.SparseTSDFVolume((-0.5 * side + 0.5 * sv,) * 3, (sdim, sdim, sdim), sv, 4 * sv, "cuda")
        svol.mark(d_depth, **frames)
        svol.allocate()
        svol.integrate(d_depth, rgb=d_rgb, **frames)
        vertices, colours, faces = svol.extract_mesh(2.0)
        del svol, d_depth, d_rgb
        if a.mesh == "simplified":
            vertices, colours, faces, _ = simplify.simplify_mesh(vertices, colours, faces, 3 * sv, "quadric")
    k, m = int(faces.shape[0]), int(vertices.shape[0])
    out = {"mesh": a.mesh, "faces": k, "vertices": m, "frames": n, "size": f"{w}x{h}", "reps": a.reps}
    common = dict(focals=focal, sizes=(h, w), min_depth=0.05, max_depth=0.75 * side)
    for tag, outputs in (("depth", ("depth_u16",)), ("all", ALL_PLANES)):
        for per_call in (n, 1):
            def run():
                meshrender.render_mesh(vertices, faces, cam_to_world=c2w, colours=colours, outputs=outputs, frames_per_call=per_call, **common)
            ms = _time(run, a.reps)
            name = f"{tag}_{'one_call' if per_call == n else 'call_per_frame'}"
            out[f"{name}_ms_per_frame"] = ms / n
            out[f"{name}_triangle_frames_per_s"] = k * n / (ms * 1e-3)
    out["single_frame_depth_ms"] = _time(lambda: meshrender.render_mesh(vertices, faces, cam_to_world=c2w[:1], outputs=("depth_u16",), **common), a.reps)
    planes = meshrender.render_mesh(vertices, faces, cam_to_world=c2w[:1], outputs=("face",), **common)
    out["first_frame_pixels_hit"] = int((planes["face"][0] >= 0).sum().item())
    out["stream_once_bytes_per_frame"] = 12 * k + 12 * m + 24 * h * w
    # the yardstick: the video rasteriser's flat triangle layer on the same triangles, one frame
    flip = np.diag([1.0, -1.0, -1.0, 1.0])
    soup = (vertices[faces.long().reshape(-1)].reshape(k, 3, 3) * torch.tensor([1.0, -1.0, -1.0], device="cuda")).contiguous()
    rgba = torch.full((k, 4), 255, dtype=torch.uint8, device="cuda")
    work = torch.empty(2 * h * w, dtype=torch.int64, device="cuda")
    frame = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    cam = (C.c_double * 16)(*(flip @ c2w[0] @ flip).reshape(16).tolist())
    lib = N.lib()

    def yardstick():
        N.check(lib.acez_render_frame(None, None, 0, _ptr(soup), _ptr(rgba), k, cam, 0.05, float(0.75 * side), w, h, 0, _ptr(work), _ptr(frame), _stream()))
    out["render_frame_ms"] = _time(yardstick, a.reps)
    out["render_frame_pixels_hit"] = int(frame.any(-1).sum().item())
    print(json.dumps({key: (float(f"{x:.4g}") if isinstance(x, float) else x) for key, x in out.items()}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
