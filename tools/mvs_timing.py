"""Plane-sweep stereo on the box: prefilter, sweep and consistency check on their own, and estimate_depth.py as a whole (DESIGN.md
section 4k). HIP events around each call, median of the repetitions; the frames are on the device before the timed calls.

    python tools/mvs_timing.py [--frames 48] [--planes 128] [--sources 4] [--window 2] [--reps 10] [--no_cli] [--out profiles/mvs_timing.json]
    python tools/mvs_timing.py --sgm           (adds the legs of --aggregation sgm: volume, aggregate with 4 and 8 paths, select, on one
                                                frame and over all frames on four streams; writes profiles/mvs_timing_sgm.json)

The scene is the wall and box of tests/mvs_cases.py at 240 x 320 px, the cameras on a line. Prints one JSON line and writes it to --out."""
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
from acezero_amd import cli, mvs  # noqa: E402
from tests import mvs_cases as MC  # noqa: E402
from tools.rgbd_timing import _time  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--planes", type=int, default=128)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--window", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no_cli", action="store_true")
    ap.add_argument("--sgm", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mvs_timing_sgm.json" if a.sgm else "mvs_timing.json")
    n, h, w, focal = a.frames, 240, 320, MC.FOCAL * 2.5
    c2w = MC.cameras(n, spacing=0.05)
    images = np.stack([MC.render(T, h, w, focal)[0] for T in c2w])
    sources = MC.nearest_sources(n, a.sources)
    fs = mvs.StereoFrames(torch.from_numpy(images).cuda(), cam_to_world=c2w, focals=focal)
    out = {"frames": n, "size": f"{w}x{h}", "planes": a.planes, "sources": a.sources, "window_radius": a.window, "reps": a.reps}
    out["prefilter_ms"] = _time(fs.prefilter, a.reps)

    def sweep_all():
        for f in range(n):
            fs.sweep(f, sources[f], MC.Z_NEAR, MC.Z_FAR, a.planes, window=a.window)

    def check_all():
        for f in range(n):
            fs.check(f, sources[f])

    jobs = [(f, sources[f], MC.Z_NEAR, MC.Z_FAR, None) for f in range(n)]
    out["sweep_one_stream_ms"] = _time(sweep_all, a.reps)
    for streams in (2, 4, 8):
        out[f"sweep_{streams}_streams_ms"] = _time(lambda: fs.sweep_frames(jobs, a.planes, a.window, streams=streams), a.reps)
    out["sweep_ms"] = out[f"sweep_{mvs.SWEEP_STREAMS}_streams_ms"]                            # what estimate_depth_maps runs
    out["sweep_ms_per_frame"] = out["sweep_ms"] / n
    out["sweep_one_frame_ms"] = _time(lambda: fs.sweep(n // 2, sources[n // 2], MC.Z_NEAR, MC.Z_FAR, a.planes, window=a.window), a.reps)
    out["sweep_samples_per_s"] = n * h * w * a.planes * a.sources / (out["sweep_ms"] * 1e-3)     # pixel x plane x source
    out["check_ms"] = _time(check_all, a.reps)
    out["pixels_with_depth_nearest_sources"] = float((fs.out != 0).float().mean().item())     # (the command line picks wider baselines)
    if a.sgm:
        mid = n // 2
        keep = -(-len(sources[mid]) // 2)
        p1, p2 = mvs.sgm_penalties(keep, a.window)
        sc = mvs.SgmScratch(h * w * a.planes, fs.device)
        out["sgm_p1_p2"] = [p1, p2]
        out["sgm_scratch_bytes_per_stream"] = mvs.SgmScratch.nbytes(sc.elements)
        out["volume_one_frame_ms"] = _time(lambda: fs.volume(mid, sources[mid], MC.Z_NEAR, MC.Z_FAR, sc, a.planes, a.window), a.reps)
        out["zero_s_one_frame_ms"] = _time(lambda: sc.s.zero_(), a.reps)
        for paths in (4, 8):                                      # (includes zeroing S)
            out[f"aggregate_{paths}_paths_one_frame_ms"] = _time(lambda: fs.aggregate(mid, sc, a.planes, paths, p1, p2), a.reps)
        out["select_on_s_one_frame_ms"] = _time(lambda: fs.select(mid, MC.Z_NEAR, MC.Z_FAR, sc, a.planes), a.reps)
        out["select_on_c_one_frame_ms"] = _time(lambda: fs.select(mid, MC.Z_NEAR, MC.Z_FAR, sc, a.planes, aggregated=False), a.reps)
        for paths in (4, 8):
            run = lambda: fs.sweep_frames(jobs, a.planes, a.window, aggregation="sgm", sgm_paths=paths)
            out[f"sgm_{paths}_paths_ms"] = _time(run, a.reps)
            out[f"sgm_{paths}_paths_ms_per_frame"] = out[f"sgm_{paths}_paths_ms"] / n
            check_all()
            torch.cuda.synchronize()
            out[f"pixels_with_depth_sgm_{paths}_paths"] = float((fs.out != 0).float().mean().item())
        out["sgm_scratch_bytes"] = fs.sgm_scratch_bytes
    if not a.no_cli:
        with tempfile.TemporaryDirectory() as tmp:
            from PIL import Image
            from acezero_amd.session import write_pose_file
            names = [os.path.join(tmp, f"frame_{k:03d}.png") for k in range(n)]
            for name, im in zip(names, images):
                Image.fromarray(np.stack([im] * 3, -1)).save(name)
            write_pose_file(os.path.join(tmp, "poses.txt"), names, c2w, [5000] * n, focal)
            lines = []
            handler = logging.Handler()
            handler.emit = lambda record: lines.append(record.getMessage())
            logging.getLogger("estimate_depth").addHandler(handler)
            t0 = time.perf_counter()
            cli.estimate_depth_main([os.path.join(tmp, "poses.txt"), os.path.join(tmp, "frame_*.png"), os.path.join(tmp, "depth"), "--image_resolution",
                                     str(h), "--depth_range", str(MC.Z_NEAR), str(MC.Z_FAR), "--planes", str(a.planes), "--sources", str(a.sources),
                                     "--window", str(a.window)] + (["--aggregation", "sgm"] if a.sgm else []))
            out["cli_total_s"] = time.perf_counter() - t0
            m = re.search(r"Decode ([\d.]+) s, upload \+ kernels \+ download ([\d.]+) s, write ([\d.]+) s", "\n".join(lines))
            out["cli_decode_s"], out["cli_device_s"], out["cli_write_s"] = (float(g) for g in m.groups())
            out["cli_log"] = [ln for ln in lines if ln.startswith(("Estimated", "Pixels", "Aggregation"))]
    line = json.dumps({k: (float(f"{x:.4g}") if isinstance(x, float) else x) for k, x in out.items()})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
