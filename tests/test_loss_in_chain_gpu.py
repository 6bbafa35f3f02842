"""GPU: rowseq_loss_kernel (head_kernels.hip) -- the fused step's loss as stage -1 of the input-gradient chain's launch and the next
batch's gather in that launch's idle loader waves: three launches per step -- against the four-launch flow it replaces
(ACEZ_LOSS_IN_CHAIN=0: loss_gather_kernel between the two chains). A row tile runs loss_kernel's own five 16-row blocks with their own
indices, so every partial lands in the slot it had and every sum keeps its order: parameters, both moments, the step's scalars and the
scene coordinates of the batch must agree bit for bit after EVERY step. Three steps with the next batch announced: step 2 consumes the
rows step 1 gathered inside its chain.

Batch sizes: 16 = one loss block (three sibling workgroups whose block lies past the batch must still bump the hand-off counter);
81 = a second row tile that holds one row; 357 = 4 tiles + 37 rows, a partly filled block in the last tile; 400 = exact tiles."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import big_problem as _big_problem

pytestmark = pytest.mark.gpu

_PROB = {}


def _problem(dtype):
    if dtype not in _PROB:
        prob = _big_problem(n_images=8, patches_per_view=256)
        if dtype == "fp16":
            prob = dict(prob)
            prob["features"] = prob["features"].astype(np.float16).astype(np.float32)
        _PROB[dtype] = prob
    return _PROB[dtype]


def _trainer(prob, dtype, in_chain):
    from acezero_amd.head import HeadTrainer
    from acezero_amd import synth
    os.environ["ACEZ_LOSS_IN_CHAIN"] = "1" if in_chain else "0"
    try:
        tr = HeadTrainer(prob["mean"], num_head_blocks=1, use_homogeneous=True, max_batch=512, loss_type="tanh", schedule="1cyclepoly",
                         iterations=50, lr_min=1e-4, lr_max=6e-4, warmup_iterations=10, cooldown_iterations=10, dtype=dtype)
    finally:
        os.environ.pop("ACEZ_LOSS_IN_CHAIN", None)
    tr.load_flat(torch.from_numpy(synth.init_head_params(11, num_head_blocks=1, use_homogeneous=True)))
    tr.set_buffer(prob["features"], prob["target_px"], prob["view_idx"], prob["view_aug_inv"], prob["view_K"], prob["view_Kinv"],
                  prob["view_image"], prob["image_pose_inv"])
    return tr


def _run(tr, batches):
    """Step through `batches`, each step announcing its successor; the trainer's observable state after every step."""
    tr.set_profiling(True)
    seen = []
    for i, idx in enumerate(batches):
        tr.step(idx, batches[i + 1] if i + 1 < len(batches) else None)
        st = tr.state()
        torch.cuda.synchronize()
        seen.append((tr.params.clone(), tr.adam_m.clone(), tr.adam_v.clone(),
                     {k: st[k] for k in ("iteration", "loss", "batch_inliers", "lr", "grad_scale", "nan", "opt_steps")},
                     tr.last_scene_coords(int(idx.numel()))))
    return seen, tr.get_profile()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("sizes", [(16, 16, 16), (81, 81, 81), (357, 357, 357), (400, 400, 400), (357, 81, 357)],
                         ids=lambda s: "n" + "_".join(map(str, s)))
def test_three_launch_step_equals_the_four_launch_step_bit_for_bit(sizes, dtype):
    prob = _problem(dtype)
    rng = np.random.default_rng(17 + sum(sizes))
    rows = prob["features"].shape[0]
    batches = [torch.from_numpy(rng.permutation(rows)[:n].astype(np.int64)).cuda() for n in sizes]
    new = _trainer(prob, dtype, True)
    ref = _trainer(prob, dtype, False)
    assert new.seq_status()["enabled"] and ref.seq_status()["enabled"]
    got, prof_new = _run(new, batches)
    want, prof_ref = _run(ref, batches)
    # the flows under test are the ones that ran: no loss launch of its own in the three-launch flow (its time is part of gemm_dgrad)
    assert prof_new["loss"] == (0.0, 0) and prof_ref["loss"][1] == len(batches) and prof_ref["loss"][0] > 0.0
    assert prof_new["gemm_dgrad"][0] > 0.0
    assert new.seq_status()["faults"] == 0 and ref.seq_status()["faults"] == 0
    for step, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g[0], w[0]), "parameters, step %d" % step
        assert torch.equal(g[1], w[1]) and torch.equal(g[2], w[2]), "moments, step %d" % step
        assert g[3] == w[3], "scalars, step %d: %r != %r" % (step, g[3], w[3])
        assert g[3]["iteration"] == step + 1 and not g[3]["nan"]
        assert np.array_equal(g[4], w[4]), "scene coordinates, step %d" % step
