"""The bench's in-process reconstruction leg with the session's INFO log: python tools/session_timing.py [frames] [--portrait-every K]

--portrait-every K: the same reconstruction (sequence, options) built here, with every K-th frame rendered portrait (h and w swapped, same
focal): a folder of two size classes. K = 0 builds the one-size sequence through the same code. Both print the session's per-phase
seconds (encode, buffer creation, training loop, registration)."""
import logging
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402


def mixed_session(n, every, device):
    """bench.bench_session's reconstruction, frames i % every == every - 1 portrait (every = 0: none)."""
    from acezero_amd import synth
    from acezero_amd.session import ReconstructionSession, default_options
    it = 4000
    seq = synth.render_room_sequence(seed=2089, n_frames=n, arc_deg=0.5 * n, device=str(device))
    por = np.arange(every - 1, n, every) if every > 0 else np.zeros(0, np.int64)
    if len(por):
        tall = synth.render_room_sequence(seed=2089, n_frames=n, arc_deg=0.5 * n, h=640, w=480, focal=seq["focal"], device=str(device),
                                          pose_override=seq["poses"])
        land = np.setdiff1d(np.arange(n), por)
        images = [(land, seq["images"][land]), (por, tall["images"][por])]
        tall_ids = set(por.tolist())
        depth = [(tall if i in tall_ids else seq)["depth"][i] for i in range(n)]
    else:
        images, depth = seq["images"], seq["depth"]
    esd = {k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}
    opt = default_options(use_external_focal_length=seq["focal"], try_seeds=2, seed_iterations=it, iterations=it, refit_iterations=it,
                          iterations_max=8, final_refit_posewait=it // 5, learning_rate_warmup_iterations=it // 5, cooldown_iterations=it // 5,
                          aug_rotation=2, aug_scale=1.06, aug_black_white=0.02)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ses = ReconstructionSession(esd, images, opt=opt, depth=depth)
    res = ses.reconstruct()
    torch.cuda.synchronize()
    return {"value": time.perf_counter() - t0, "frames": n, "portrait": int(len(por)), "size_classes": len(ses.classes),
            "registration_rates": [round(h["registration_rate"], 3) for h in res["history"]],
            "timings": {k: round(v, 3) for k, v in res["timings"].items()}}


logging.basicConfig(level=logging.INFO)
torch.cuda.set_device(0)
t0 = time.perf_counter()
argv = sys.argv[1:]
every = None
if "--portrait-every" in argv:
    k = argv.index("--portrait-every")
    every = int(argv[k + 1])
    del argv[k:k + 2]
frames = int(argv[0]) if argv else 120
if every is None:
    out = bench.bench_session(SimpleNamespace(session_frames=frames), torch.device("cuda", 0))
else:
    out = mixed_session(frames, every, torch.device("cuda", 0))
print({k: v for k, v in out.items() if k not in ("note", "metric")}, "wall incl. render %.2f s" % (time.perf_counter() - t0))
