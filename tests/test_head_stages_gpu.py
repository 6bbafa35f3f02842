"""GPU: the 512-wide GEMM stages of the head's training step, judged per element from their own operands (tests/head_stage_restated.py;
the checker itself is proven on the CPU by tests/test_head_stages_cpu.py).

The product library runs backward() -- the split flow, so that the weight-gradient slabs and tr.grad exist -- and every element of every
kept activation, residual stream, unkept layer's mask, propagated gradient, slab, bias partial and wide-layer entry of tr.grad must lie
in the interval its own stored operands allow. Row counts: the 80-row tile of rowgemm80 (80, 81; ragged last tiles of 37 and 77 rows at
357 and 637; five full tiles at 400), the 64-row stage and the slab split of wgrad_kloop (64: slab 1 empty, 65: one row, 128, 129), the
16-row fragment, one row, the 20-row groups of the bias sum. No 5120-row case: there the derived bound, about n * 2^-23, is the size of
one row's contribution.

A configuration runs all its row counts in turn, with a trainer per row count, because global_batch -- which equals the row count here --
is fixed at creation. Each trainer first runs a full 640-row backward(), so that every buffer holds another batch's values in the rows
past n: a kernel that reads row n of a ragged tile then reads something."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import head_oracle
from tests import head_stage_restated as hs
from tests import helpers
from tests.test_head_gpu import _trainer

pytestmark = pytest.mark.gpu

ROWS = [1, 16, 64, 65, 80, 81, 128, 129, 357, 400, 637]
MAX_BATCH = 640


@functools.lru_cache(maxsize=None)
def _inputs(regime, nb):
    if regime == "trained":
        prob, flat0 = helpers.trained_problem(nb)
        return prob, flat0, helpers.TRAINED_CONFIGS["head_trained_1cyclepoly"]
    return helpers.big_problem(), head_oracle.init_params(helpers.SEED + 1, nb), helpers.HEAD_CONFIGS["head_tanh_1cyclepoly"]


def _judge(dtype, regime, nb, n, seq=True):
    """The results of one case: a fresh trainer, a 640-row backward() to fill the buffers, (trained regime) three steps, the judged backward()."""
    prob, flat0, c = _inputs(regime, nb)
    cfg = helpers.full_cfg(c, prob)
    cfg.update(global_batch=n, num_head_blocks=nb)
    if not seq:
        os.environ["ACEZ_SEQ"] = "0"
    try:
        tr = _trainer(prob, flat0, cfg, max_batch=MAX_BATCH, dtype=dtype)
    finally:
        os.environ.pop("ACEZ_SEQ", None)
    assert "diag" not in os.path.basename(tr.lib._name) and tr.seq_status()["enabled"] is seq
    rng = np.random.default_rng(1000 * nb + n)
    batch = lambda k: torch.from_numpy(rng.permutation(prob["features"].shape[0])[:k].astype(np.int64)).cuda()
    tr.backward(batch(MAX_BATCH))
    idx = batch(n)
    if regime == "trained":
        # three steps on the judged rows: the 16-bit copies then come from the device's own recast, and in fp16 the gradient scale has
        # settled on this batch (a step that overflows at the initial scale is abandoned, as designed, and lowers it: hence >= 1 below)
        for _ in range(3):
            tr.step(idx)
    snap = helpers.trainer_snapshot(tr)     # (its state read runs the pending schedule wave: grad_scale is the next step's)
    assert not snap["nan"] and (regime != "trained" or snap["opt_steps"] >= 1), snap["opt_steps"]
    tr.backward(idx)
    torch.cuda.synchronize()
    cap = hs.capture_trainer(tr, n, snap["w16"], snap["params"].view(np.float32), snap["grad_scale"])
    assert cap.nslabs == (2 if nb == 1 else 1) and tr.L == (8 if nb == 1 else 11)
    results = hs.check_all(cap)
    what = "%s %s blocks=%d n=%d seq=%d" % (dtype, regime, nb, n, seq)
    for stage, d in hs.summary(results).items():
        print("STAGES %s %s: %d elements" % (what, stage, d["elements"])
              + ("" if d["worst"] is None else ", worst |got - v| / s = %.4f" % d["worst"])
              + ("" if d["flips"] is None else ", %d rounding flips" % d["flips"])
              + (", %d left out" % d["left_out"] if stage == "mask" else ""))
    # every buffer, every layer: kept activations, residual streams, masks and dZ of l < L - 1, slabs + tr.grad (interval and bits), partials, biases
    assert len(results) == (tr.L - nb - 1) + (nb + 1) + 2 * (tr.L - 1) + (2 + cap.nslabs) * tr.L + 2 * tr.L - 1
    hs.assert_clean(results, what)
    tr.close()
    return results


def _configuration(dtype, regime, nb, rows, seq=True):
    """Every row count judged element by element; the undecided mask bits of every layer, over the configuration's row counts, within the
    cap. (Per row count the cap would be decided by chance: one layer of one row has 512 bits, so a single undecided bit is 0.2 %, while
    the share that follows from the operands and s is about 0.05 %.)"""
    results = []
    for n in rows:
        results += _judge(dtype, regime, nb, n, seq)
    hs.assert_left_out_capped(results, "%s %s blocks=%d" % (dtype, regime, nb))


@pytest.mark.parametrize("regime", ["untrained", "trained"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_every_stage_element_lies_in_the_interval_of_its_operands(dtype, regime):
    """One head block: L = 8, two slabs, the one-launch chains; all row counts in turn."""
    _configuration(dtype, regime, 1, ROWS)


def test_two_blocks_two_chain_launches_one_slab():
    """L = 11: one slab, two launches per chain, the residual gradient passes through two blocks."""
    _configuration("bf16", "untrained", 2, [81, 357])


def test_per_layer_launches():
    _configuration("bf16", "untrained", 1, [81], seq=False)
