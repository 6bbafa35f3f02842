"""GPU: what a training step leaves for the next one (acez_trainer::carry, head_api.hip: the pending schedule wave and the batch gathered
ahead) through every transition of the record, in one fixed script: an announcement the next call does not take, a state read between an
announcement and the call that consumes it, fused -> split -> fused steps with announcements (acez_train_update_next among them), and
sync_weights between two announced steps. Parameters, moments, pose parameters, the schedule state and the log must equal the same trainer
driven by plain acez_train_step calls bit for bit, for every pose-refinement mode."""
import numpy as np
import pytest
import torch

from oracle import head_oracle
from tests import helpers
from tests.test_head_gpu import _trainer

pytestmark = pytest.mark.gpu

N_STEPS = 12


def _script(piped, batches, other, i):
    """Step i of the announcing trainer; returns whether the state is compared after it."""
    nxt = batches[i + 1] if i + 1 < len(batches) else None
    if i == 2:
        piped.step(batches[i], other)            # announced, then a call with different indices
    elif i == 5:
        piped.backward(batches[i])               # fused (announced) -> split with the next batch announced to the update
        piped.update(nxt)
    elif i == 7:
        piped.backward(batches[i])               # fused (announced) -> split without an announcement
        piped.update()
    else:
        piped.step(batches[i], nxt)              # fused after a split announcement (6), announced steps elsewhere
    return i in (3, 6)                           # a state read between an announcement and the call that consumes it


@pytest.mark.parametrize("name,dtype", [("head_tanh_1cyclepoly", "bf16"), ("head_tanh_posenaive", "bf16"), ("head_tanh_posemlp", "bf16"),
                                        ("head_tanh_1cyclepoly", "fp16")])
def test_record_transitions_equal_plain_steps_bitwise(name, dtype):
    prob = helpers.big_problem(n_images=8, patches_per_view=512)
    flat0 = head_oracle.init_params(helpers.SEED + 1)
    cfg = helpers.full_cfg(helpers.HEAD_CONFIGS[name], prob)
    cfg.update(global_batch=2048, iterations=60, pose_refinement_wait=1)
    plain, piped = (_trainer(prob, flat0, cfg, max_batch=2048, dtype=dtype) for _ in range(2))
    rng = np.random.default_rng(41)
    N = prob["features"].shape[0]
    batches = [torch.from_numpy(rng.permutation(N)[:(2048 if i % 4 else 1111)].astype(np.int64)).cuda() for i in range(N_STEPS)]
    other = torch.from_numpy(rng.permutation(N)[:2048].astype(np.int64)).cuda()
    for i, b in enumerate(batches):
        plain.step(b)
        if _script(piped, batches, other, i):
            assert plain.state() == piped.state(), i
        if i == 8:   # between two announced steps: a restart point drops the batch gathered ahead
            plain.sync_weights()
            piped.sync_weights()
    torch.cuda.synchronize()
    for a, b in ((plain.params, piped.params), (plain.adam_m, piped.adam_m), (plain.adam_v, piped.adam_v),
                 (plain.pose_params, piped.pose_params), (plain.pose_m, piped.pose_m), (plain.pose_v, piped.pose_v)):
        assert (a is None and b is None) or torch.equal(a, b)
    sp, sq = plain.state(), piped.state()
    assert sp == sq and sp["iteration"] > N_STEPS // 2   # (1cyclepoly's cool-down may end the schedule before the script does)
    lp, lq = plain.log(0, sp["iteration"]), piped.log(0, sp["iteration"])
    assert np.array_equal(lp[0], lq[0]) and np.array_equal(lp[1], lq[1])
    if cfg["pose_refinement"] != "none":
        np.testing.assert_array_equal(plain.current_poses(), piped.current_poses())
