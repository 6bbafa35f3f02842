"""GPU: rowstep_kernel (head_kernels.hip) -- the forward chain, the loss and the input-gradient chain of the plain fused step as ONE
launch, two launches per step -- against the three-launch flow it replaces (ACEZ_STEP_CHAIN=0: rowseq_kernel<false>, then
rowseq_loss_kernel). Same layer bodies, same loss blocks, same slots for every partial: parameters, both moments, the step's scalars
and the scene coordinates of the batch must agree bit for bit after EVERY step. Three steps with the next batch announced: step 2
consumes the rows step 1 gathered inside its launch.

Batch sizes: 16 = one loss block (three sibling workgroups whose block lies past the batch must still bump the hand-off counter);
81 = a second row tile that holds one row; 357 = 4 tiles + 37 rows; 357, 81, 357 = a changing tile count (per-tile bases); 400 = exact
tiles; 641 with max_batch 768 = nine row tiles, two per XCD slot: the rounded-up grid has workgroups that own no tile and must leave
without touching a counter.

The second test switches one trainer between the two flows in mid-run (profiling on = the three-launch flow): the counter bases must
stay right across the switch."""
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


def _trainer(prob, dtype, step_chain, max_batch=512):
    from acezero_amd.head import HeadTrainer
    from acezero_amd import synth
    os.environ["ACEZ_STEP_CHAIN"] = "1" if step_chain else "0"
    try:
        tr = HeadTrainer(prob["mean"], num_head_blocks=1, use_homogeneous=True, max_batch=max_batch, loss_type="tanh", schedule="1cyclepoly",
                         iterations=50, lr_min=1e-4, lr_max=6e-4, warmup_iterations=10, cooldown_iterations=10, dtype=dtype)
    finally:
        os.environ.pop("ACEZ_STEP_CHAIN", None)
    tr.load_flat(torch.from_numpy(synth.init_head_params(11, num_head_blocks=1, use_homogeneous=True)))
    tr.set_buffer(prob["features"], prob["target_px"], prob["view_idx"], prob["view_aug_inv"], prob["view_K"], prob["view_Kinv"],
                  prob["view_image"], prob["image_pose_inv"])
    return tr


def _observe(tr, n):
    st = tr.state()
    torch.cuda.synchronize()
    return (tr.params.clone(), tr.adam_m.clone(), tr.adam_v.clone(),
            {k: st[k] for k in ("iteration", "loss", "batch_inliers", "lr", "grad_scale", "nan", "opt_steps")},
            tr.last_scene_coords(n))


def _run(tr, batches, first=0, count=None):
    """Steps first .. first + count - 1 of `batches`, each announcing its successor; the trainer's observable state after every step."""
    seen = []
    for i in range(first, len(batches) if count is None else first + count):
        tr.step(batches[i], batches[i + 1] if i + 1 < len(batches) else None)
        seen.append(_observe(tr, int(batches[i].numel())))
    return seen


def _assert_equal(got, want):
    assert len(got) == len(want)
    for step, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g[0], w[0]), "parameters, step %d" % step
        assert torch.equal(g[1], w[1]) and torch.equal(g[2], w[2]), "moments, step %d" % step
        assert g[3] == w[3], "scalars, step %d: %r != %r" % (step, g[3], w[3])
        assert g[3]["iteration"] == step + 1 and not g[3]["nan"]
        assert np.array_equal(g[4], w[4]), "scene coordinates, step %d" % step


def _batches(prob, sizes, seed):
    rng = np.random.default_rng(seed)
    rows = prob["features"].shape[0]
    return [torch.from_numpy(rng.permutation(rows)[:n].astype(np.int64)).cuda() for n in sizes]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("sizes,max_batch", [((16, 16, 16), 512), ((81, 81, 81), 512), ((357, 81, 357), 512), ((400, 400, 400), 512),
                                             ((641, 641, 641), 768)],
                         ids=lambda v: "n" + "_".join(map(str, v)) if isinstance(v, tuple) else "max%d" % v)
def test_two_launch_step_equals_the_three_launch_step_bit_for_bit(sizes, max_batch, dtype):
    prob = _problem(dtype)
    batches = _batches(prob, sizes, 23 + sum(sizes))
    new = _trainer(prob, dtype, True, max_batch)
    ref = _trainer(prob, dtype, False, max_batch)
    assert new.seq_status()["enabled"] and ref.seq_status()["enabled"]
    assert new.seq_status(step_chain=True)["step_chain"] and not ref.seq_status(step_chain=True)["step_chain"]
    got = _run(new, batches)
    want = _run(ref, batches)
    # the flows under test are the ones that ran
    assert new.seq_status(step_chain=True)["step_chain_steps"] == 3 and ref.seq_status(step_chain=True)["step_chain_steps"] == 0
    assert new.seq_status()["faults"] == 0 and ref.seq_status()["faults"] == 0
    _assert_equal(got, want)


def test_switching_flows_in_mid_run_keeps_the_counter_bases_right():
    prob = _problem("bf16")
    batches = _batches(prob, (357, 81, 400, 357, 16, 357), 5)
    new = _trainer(prob, "bf16", True)
    ref = _trainer(prob, "bf16", False)
    got = _run(new, batches, 0, 2)
    new.set_profiling(True)      # the chains' event pairs are timed: the three-launch flow
    got += _run(new, batches, 2, 2)
    assert new.seq_status(step_chain=True)["step_chain_steps"] == 2
    prof = new.get_profile()
    assert prof["gemm_fwd"][1] > 0 and prof["gemm_dgrad"][0] > 0.0 and prof["loss"] == (0.0, 0)
    new.set_profiling(False)
    got += _run(new, batches, 4, 2)
    want = _run(ref, batches)
    assert new.seq_status(step_chain=True)["step_chain_steps"] == 4 and ref.seq_status(step_chain=True)["step_chain_steps"] == 0
    assert new.seq_status()["faults"] == 0 and ref.seq_status()["faults"] == 0
    _assert_equal(got, want)
