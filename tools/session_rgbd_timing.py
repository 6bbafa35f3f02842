"""The registration leg of one reconstruction round in RGB-D mode against the RGB registration of the same frames on the same box:
ReconstructionSession.register(head, focal, use_depth=True) and register(head, focal) on a session over the synthetic room, HIP
events around each call, median of the repetitions; and the depth -> camera-coordinate launch against the torch ops it replaces.

    python tools/session_rgbd_timing.py [--frames 256] [--reps 10]

The head is mapped once from the known poses with depth (a few thousand steps), so both estimators register the frames. Prints one
JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acezero_amd import dsacstar, synth  # noqa: E402
from acezero_amd.session import ReconstructionSession, default_options  # noqa: E402
from tools.rgbd_timing import _time  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=3000)
    a = ap.parse_args()
    n = a.frames
    seq = synth.render_room_sequence(seed=2089, n_frames=n, arc_deg=36.0, device="cuda")
    esd = {k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}
    it = a.iterations
    opt = default_options(rgbd=True, use_external_focal_length=seq["focal"], iterations=it, learning_rate_warmup_iterations=it // 5,
                          cooldown_iterations=it // 5, aug_rotation=2, aug_scale=1.06, aug_black_white=0.02, use_aug=False)
    ses = ReconstructionSession(esd, seq["images"], opt=opt, depth=seq["depth"])
    ids = list(range(0, n, 2))
    m = ses.map(ids, seq["poses"][ids].cpu(), seq["focal"], iterations=it, loss_type="tanh", schedule="1cyclepoly", lr_max=0.003, with_depth=True)
    head, focal = m["head"], seq["focal"]
    out = {"frames": n, "cells": f"{ses.oh}x{ses.ow}", "hyps": opt.ransac_iterations, "reps": a.reps}
    for name, kw in (("rgbd", dict(use_depth=True)), ("rgb", {})):
        out[f"register_{name}_ms"] = _time(lambda: ses.register(head, focal, **kw), a.reps)
        _, inl = ses.register(head, focal, **kw)
        out[f"register_{name}_rate"] = float((inl > opt.registration_confidence).mean())
        out[f"register_{name}_median_inliers"] = float(np.median(inl))
    # the parts: head forward (shared), the estimator alone, the camera coordinates
    sc = ses.scene_coordinates(head, np.arange(n))
    depth = ses.frame_depth(np.arange(n))
    fl = [focal] * n
    out["head_forward_ms"] = _time(lambda: ses.scene_coordinates(head, np.arange(n)), a.reps)
    out["camera_coordinates_launch_ms"] = _time(lambda: dsacstar.camera_coordinates_device(depth, fl, ses.ppx, ses.ppy), a.reps)
    out["camera_coordinates_torch_ops_ms"] = _time(lambda: dsacstar.camera_coordinates(depth, fl, ses.ppx, ses.ppy), a.reps)
    cc = dsacstar.camera_coordinates_device(depth, fl, ses.ppx, ses.ppy)
    prm = dict(hyps=opt.ransac_iterations, thr=opt.ransac_threshold, alpha=opt.inlieralpha, max_reproj=opt.maxpixelerror)
    keys = list(range(n))
    out["estimator_rgbd_ms"] = _time(lambda: dsacstar.register_batch_rgbd(sc, cc, prm, 1305, keys, want_masks=False), a.reps)
    out["estimator_rgb_ms"] = _time(lambda: dsacstar.register_batch(sc, [(focal, ses.ppx, ses.ppy)] * n, dict(prm, sub=8, max_tries=16), 1305, keys,
                                                                    want_masks=False), a.reps)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
