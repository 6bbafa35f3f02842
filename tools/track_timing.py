"""Frame-to-model tracking on the box: one ACCUMULATE over all frames, one UPDATE, the pair, and a whole
`track` call, beside one iteration of the numpy restatement (tests/track_restated.py) on the same machine. HIP events around each
call, median of the repetitions.

    python tools/track_timing.py [--frames 48] [--dim 256] [--reps 10] [--numpy_frames 2] [--out profiles/track_timing.json]

The scene is tools/fusion_timing.py's: the analytic box room scaled to fill a dim^3 volume of 2 cm voxels, 640 x 480 depth at a
Kinect's focal length, fused under the true poses; the tracked poses are those moved by N(0, 1 cm) and N(0, 0.5 degrees) per axis.
The frames are on the device before the timed calls, and the frame table is uploaded before them (ACCUMULATE is timed without its
upload, as iterations 2 .. of a loop run it). `update` is timed with a copy that puts the state back to a running one at record 0,
and that copy's time is taken off. The whole call is timed on the wall clock, from the call to the read-back, once with the default
tolerance (frames stop when they have converged; the launches after that pass over them) and once with a tolerance of 0 (every
frame runs all its iterations). Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acezero_amd import _native as N  # noqa: E402
from acezero_amd import fusion  # noqa: E402
from acezero_amd._device import ptr as _ptr, stream as _stream  # noqa: E402
from tests import fusion_cases as FC  # noqa: E402
from tests import track_cases as TC  # noqa: E402
from tests import track_restated as T  # noqa: E402
from tools.rgbd_timing import _time  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--numpy_frames", type=int, default=2, help="frames the numpy restatement is timed on (0: skip it)")
    ap.add_argument("--out", default=os.path.join("profiles", "track_timing.json"))
    a = ap.parse_args()
    n, dim, v, h, w, focal = a.frames, a.dim, 0.02, 480, 640, 525.0
    side = dim * v
    half = np.array([0.47, 0.31, 0.47]) * side
    truth = FC.room_cameras(n, radius=0.1 * side)
    poses = TC.perturb(truth, 11)
    depth = np.stack([FC.room_depth(M, h, w, focal, half) for M in truth])
    d_depth = torch.from_numpy(depth.view(np.int16)).cuda()
    origin = (-0.5 * side + 0.5 * v,) * 3
    frames = dict(focals=focal, max_depth=0.75 * side)
    vol = fusion.TSDFVolume(origin, (dim, dim, dim), v, 4 * v, "cuda").integrate(d_depth, cam_to_world=truth, **frames)
    out = {"frames": n, "volume": f"{dim}^3", "depth": f"{w}x{h}", "reps": a.reps, "pixels": n * h * w}

    (packed, _, rows, d_rows, k), = fusion.calls(d_depth, None, poses, focal, None, None, None, n, vol.device)
    tiles = (h * w + 255) // 256
    state_h = np.zeros((n, fusion.TRACK_STATE))
    state_h[:, :12] = poses[:, :3].reshape(n, 12)
    start_state = torch.from_numpy(state_h).cuda()
    state = start_state.clone()
    partials = torch.empty((n, tiles, fusion.TRACK_TERMS), dtype=torch.float64, device="cuda")
    history = torch.zeros((n, 10, fusion.TRACK_RECORD), dtype=torch.float64, device="cuda")

    def accumulate(upload=0):
        vol._track_accumulate(_ptr(packed), packed.numel(), rows, n, _ptr(d_rows), upload, 0.001, float(frames["max_depth"]), 1.0, _ptr(state),
                              _ptr(partials), _stream())

    def reset():
        state.copy_(start_state)

    def update():
        reset()
        N.check(N.lib().acez_tsdf_track_update(_ptr(partials), tiles, _ptr(d_rows), n, 0.0, 1e-4, 64, 10, _ptr(state), _ptr(history), _stream()))

    def pair():
        accumulate()
        update()

    accumulate(upload=1)
    torch.cuda.synchronize()
    ms = {name: [] for name in ("accumulate", "reset_and_update", "reset", "reset_and_pair")}
    for _ in range(3):                                             # alternate
        reset()
        ms["accumulate"].append(_time(accumulate, a.reps))
        ms["reset_and_update"].append(_time(update, a.reps))
        ms["reset"].append(_time(reset, a.reps))
        ms["reset_and_pair"].append(_time(pair, a.reps))
    for name, vals in ms.items():
        out[f"{name}_ms"], out[f"{name}_ms_rounds"] = float(np.median(vals)), vals
    out["update_ms"] = out["reset_and_update_ms"] - out["reset_ms"]
    out["pair_ms"] = out["reset_and_pair_ms"] - out["reset_ms"]
    reset()
    accumulate()
    torch.cuda.synchronize()
    samples = int(partials[:, :, 0].sum().item())
    out["samples_first_iteration"] = samples
    out["accumulate_samples_per_s"] = samples / (out["accumulate_ms"] * 1e-3)
    out["accumulate_voxel_bytes_per_s"] = 64.0 * samples / (out["accumulate_ms"] * 1e-3)     # eight (tsdf, weight) pairs of fp32 per sample

    def whole(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = vol.track(d_depth, poses, frames_per_call=n, **frames, **kw)
        return (time.perf_counter() - t0) * 1e3, got

    whole()                                                        # warm
    runs = [whole() for _ in range(5)]
    out["track_default_tolerance_ms"] = float(np.median([r[0] for r in runs]))
    info = runs[0][1][1]
    out["track_default_tolerance_iterations"] = [min(i["iterations"] for i in info), max(i["iterations"] for i in info)]
    out["track_statuses"] = {s: sum(i["status"] == s for i in info) for s in ("converged", "max_iterations", "degenerate")}
    dt0, dr0 = T.pose_errors(poses, truth)
    dt, dr = T.pose_errors(runs[0][1][0], truth)
    out["translation_error_mm"], out["rotation_error_deg"] = [1e3 * dt0.mean(), 1e3 * dt.mean()], [dr0.mean(), dr.mean()]
    out["rms_mm"] = [1e3 * float(np.mean([i["rms_first"] for i in info])), 1e3 * float(np.mean([i["rms_last"] for i in info]))]
    runs = [whole(rel_rms=0.0) for _ in range(5)]
    out["track_10_iterations_ms"] = float(np.median([r[0] for r in runs]))
    if a.numpy_frames:
        tsdf, weight = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()
        its = []
        for f in range(a.numpy_frames):
            st, hist = T.new_state(poses[f, :3]), np.zeros((10, T.RECORD))
            t0 = time.perf_counter()
            t = T.terms(tsdf, weight, origin, v, 4 * v, depth[f], st[:12], focal, w / 2.0, h / 2.0, max_depth=frames["max_depth"])
            T.update(st, T.totals(T.block_sums(t)), 0.0, 1e-4, 64, hist)
            its.append(time.perf_counter() - t0)
        out["numpy_iteration_s_per_frame"], out["numpy_iteration_s_per_frame_each"] = float(np.median(its)), its
        out["numpy_iteration_s_all_frames"] = float(np.median(its)) * n
    line = json.dumps({key: (float(f"{x:.4g}") if isinstance(x, float) else x) for key, x in out.items()})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
