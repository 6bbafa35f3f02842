"""Seed trials side by side (HeadGroup) against one after the other, on one GPU. Prints one JSON line:
  per_head_step_us[dtype][H] = {"single": us per head-step of H trainers stepped alone, "group": the same trainers as one group step}
  at B = 5120 on 10 240-row seed-shaped buffers (announced next batches, the session's loop), H = 1..5, bf16 and fp16;
  seed_stage_s[workers] = the session's seed stage (map + score of --try_seeds 5) on the synthetic room, workers 1 and 3.

    python tools/seed_group_timing.py                       # everything
    python tools/seed_group_timing.py --group-only 3 bf16   # only group steps of 3 members (for a rocprofv3 --kernel-trace --stats run)
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from acezero_amd import synth  # noqa: E402
from acezero_amd.head import HeadGroup, HeadTrainer, epoch_batches  # noqa: E402

ROWS, B = 10240, 5120


def member(k, dtype):
    prob = synth.make_training_problem(seed=2089 + 97 * k, n_images=10, views_per_image=2, patches_per_view=ROWS // 20)
    tr = HeadTrainer(prob["mean"], loss_type="tanh", schedule="1cyclepoly", iterations=100000, warmup_iterations=100, dtype=dtype)
    g = torch.Generator().manual_seed(1023 + k)
    tr.load_flat((torch.rand(tr.n_params, generator=g) * 2 - 1) / math.sqrt(512.0))
    tr.set_buffer(prob["features"], prob["target_px"], prob["view_idx"], prob["view_aug_inv"], prob["view_K"], prob["view_Kinv"],
                  prob["view_image"], prob["image_pose_inv"], target_crds=prob["target_crds"])
    return tr


def time_steps(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / steps


def per_head_step(dtype, H, steps, warmup, single=True):
    ms = [member(k, dtype) for k in range(H)]
    streams = [epoch_batches(ROWS, B, 8191 + k, ms[0].device) for k in range(H)]
    out = {}
    if single:
        def one_by_one():
            for tr, s in zip(ms, streams):
                tr.step(*next(s))
        out["single"] = time_steps(one_by_one, steps, warmup) / H
    with HeadGroup(ms) as grp:
        def group():
            pairs = [next(s) for s in streams]
            grp.step([p[0] for p in pairs], [p[1] for p in pairs])
        out["group"] = time_steps(group, steps, warmup) / H
    for tr in ms:
        assert tr.seq_status()["faults"] == 0 and not tr.state()["nan"]
        tr.close()
    return out


def seed_stage(workers, seed_iterations):
    from acezero_amd.session import ReconstructionSession, default_options
    seq = synth.render_room_sequence(seed=2089, n_frames=72, arc_deg=36.0, device="cuda")
    esd = {k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}
    opt = default_options(use_external_focal_length=seq["focal"], try_seeds=5, seed_iterations=seed_iterations, aug_rotation=2,
                          aug_scale=1.06, aug_black_white=0.02)
    ses = ReconstructionSession(esd, seq["images"], opt=opt, depth=seq["depth"])
    np.random.seed(opt.random_seed)
    seeds = np.random.uniform(size=opt.try_seeds)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trials = ses.run_seed_trials(list(range(len(seeds))), list(seeds), workers)
    torch.cuda.synchronize()
    return {"seconds": time.perf_counter() - t0, "buffer_s": ses.timings["buffer_s"], "loop_s": ses.timings["loop_s"],
            "register_s": ses.timings["register_s"], "rates": [r for _, r in trials]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--seed-iterations", type=int, default=2000)
    ap.add_argument("--group-only", nargs=2, metavar=("H", "DTYPE"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.group_only:
        print(json.dumps({"group_only": per_head_step(a.group_only[1], int(a.group_only[0]), a.steps, a.warmup, single=False)}))
        return
    res = {"per_head_step_us": {}, "B": B, "rows": ROWS, "steps": a.steps}
    for dtype in ("bf16", "fp16"):
        res["per_head_step_us"][dtype] = {H: per_head_step(dtype, H, a.steps, a.warmup) for H in range(1, 6)}
    res["seed_iterations"] = a.seed_iterations
    res["seed_stage_s"] = {w: seed_stage(w, a.seed_iterations) for w in (1, 3)}
    res["seed_stage_identical"] = res["seed_stage_s"][1]["rates"] == res["seed_stage_s"][3]["rates"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
