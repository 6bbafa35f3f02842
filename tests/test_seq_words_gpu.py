"""GPU: the progress words of the same-XCD hand-off (head_seq.h: seq_post, seq_poll_expired, seq_catch_up;
rowstep_kernel, rowseq_kernel, rowseq_loss_kernel). Word 8 nt + w of a row tile's 128-byte line belongs to wave w of column tile nt and
holds the last seam that wave has completed, as an absolute number; the host keeps the number of seams completed per row tile
(head_api.hip seq_account). So after EVERY step, live or dead, all 32 words of every row tile of the batch must equal the host's base of
that tile, the lines of the other row tiles must never have been written, and the fault word must be down -- read through
acez_trainer_debug_read kind 10.

Batch sizes, where the word layout can go wrong: 16 rows = one loss block (the blocks of three sibling workgroups lie past the batch:
they must still write their words, and their loader partners'); 81 = a second row tile that holds one row; 641 with max_batch 768 =
nine row tiles, two of them on XCD 0, a ragged last tile, and workgroups of the rounded-up grid that own no tile. Each in the fused
two-launch flow and in the three-launch flow (ACEZ_STEP_CHAIN=0), both operand types: three steps, then a step past the schedule's end
(a launch that returns at entry and must leave exactly a live launch's words). Parameters and both moments are compared bit for bit
with a trainer on per-layer launches (ACEZ_SEQ=0) after every step."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import big_problem as _big_problem

pytestmark = pytest.mark.gpu

_PROB = {}
_REF = {}


def _problem(dtype):
    if dtype not in _PROB:
        prob = _big_problem(n_images=8, patches_per_view=256)
        if dtype == "fp16":
            prob = dict(prob)
            prob["features"] = prob["features"].astype(np.float16).astype(np.float32)
        _PROB[dtype] = prob
    return _PROB[dtype]


def _trainer(prob, dtype, max_batch, env):
    from acezero_amd.head import HeadTrainer
    from acezero_amd import synth
    os.environ.update(env)
    try:
        tr = HeadTrainer(prob["mean"], num_head_blocks=1, use_homogeneous=True, max_batch=max_batch, loss_type="tanh", schedule="constant",
                         iterations=3, lr_min=3e-4, dtype=dtype)
    finally:
        for k in env:
            os.environ.pop(k, None)
    tr.load_flat(torch.from_numpy(synth.init_head_params(11, num_head_blocks=1, use_homogeneous=True)))
    tr.set_buffer(prob["features"], prob["target_px"], prob["view_idx"], prob["view_aug_inv"], prob["view_K"], prob["view_Kinv"],
                  prob["view_image"], prob["image_pose_inv"])
    return tr


def _batches(prob, n):
    rng = np.random.default_rng(31 + n)
    return [torch.from_numpy(rng.permutation(prob["features"].shape[0])[:n].astype(np.int64)).cuda() for _ in range(4)]


def _observe(tr):
    st = tr.state()
    torch.cuda.synchronize()
    return tr.params.clone(), tr.adam_m.clone(), tr.adam_v.clone(), st["iteration"]


def _reference(dtype, n, max_batch):
    """Per-layer launches (ACEZ_SEQ=0) over the same four batches, computed once per (dtype, n) and shared by both flows."""
    if (dtype, n) not in _REF:
        prob = _problem(dtype)
        ref = _trainer(prob, dtype, max_batch, {"ACEZ_SEQ": "0"})
        assert not ref.seq_status()["enabled"]
        seen = []
        for idx in _batches(prob, n):
            ref.step(idx)
            seen.append(_observe(ref))
        _REF[(dtype, n)] = seen
    return _REF[(dtype, n)]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("step_chain", [True, False], ids=["fused", "three_launch"])
@pytest.mark.parametrize("n,max_batch", [(16, 512), (81, 512), (641, 768)])
def test_every_word_of_the_batchs_row_tiles_equals_the_hosts_base_after_every_step(n, max_batch, step_chain, dtype):
    prob = _problem(dtype)
    want = _reference(dtype, n, max_batch)
    tr = _trainer(prob, dtype, max_batch, {"ACEZ_STEP_CHAIN": "1" if step_chain else "0"})
    assert tr.seq_status()["enabled"] and bool(tr.seq_status(step_chain=True)["step_chain"]) == step_chain
    tiles = (n + 79) // 80
    words, fault, base = tr.seq_words()
    assert not words.any() and fault == 0 and not base.any()   # a new trainer: nothing has been handed off
    per_step = None
    for step, idx in enumerate(_batches(prob, n)):   # the schedule ends after three of them
        before = base
        tr.step(idx)
        got = _observe(tr)
        words, fault, base = tr.seq_words()
        print("n %d %s %s step %d: base %s words min %s max %s fault %d" % (n, dtype, "fused" if step_chain else "three-launch", step,
              base[:tiles], words[:tiles].min(1), words[:tiles].max(1), fault))
        assert fault == 0, step
        assert (words[:tiles] == base[:tiles, None]).all(), (step, np.argwhere(words[:tiles] != base[:tiles, None])[:8])
        assert not words[tiles:].any() and not base[tiles:].any(), step   # row tiles outside the batch: never touched
        # the same seams per step on every row tile, live or dead (dead: step 3)
        inc = base[:tiles] - before[:tiles]
        per_step = int(inc[0]) if per_step is None else per_step
        assert per_step > 0 and (inc == per_step).all(), (step, inc)
        assert got[3] == min(step + 1, 3) == want[step][3]
        assert torch.equal(got[0], want[step][0]), "parameters, step %d" % step
        assert torch.equal(got[1], want[step][1]) and torch.equal(got[2], want[step][2]), "moments, step %d" % step
    assert tr.seq_status()["faults"] == 0
    steps = tr.seq_status(step_chain=True)["step_chain_steps"]   # the flow under test is the one that ran
    assert steps >= 3 if step_chain else steps == 0
