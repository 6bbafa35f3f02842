"""GPU: the abandoned-step contract of the data-parallel (split) flow with pose and calibration refinement, on the product library.

A rank whose hand-off poll expires abandons its step and says so in statistics slot 3 of the gradient bucket, grad[n_params + 3]; after
the all-reduce the slot holds  #ranks that abandoned + 1024 * #ranks whose fp16 chain overflowed,  and EVERY rank must skip the same
step so that the replicas stay bit-identical. One process plays the healthy rank of a two-rank job here, with no injection switch: it
runs backward(), its bucket is overwritten in place with what the all-reduce would have delivered -- slot 3 set to the value under
test, everything else its own gradient plus a peer's leftover (a fixed finite vector of magnitude 1e3 over the whole bucket, the pose
slice included, or a few infinities) -- and then it closes the step in each form a split step can be closed with. Required:

  slot 3 % 1024 != 0            the whole snapshot unchanged (head and pose parameters, all moments, 16-bit copies, refined poses, every
                                field of state(), the log); state() then falls back to per-layer launches, and the steps that follow are
                                bitwise those of a per-layer trainer that was fed the surviving batches only
  slot 3 = 1024 k, fp16         overflow only: the head's parameters, moments, 16-bit copies and opt_steps unchanged; the iteration is
                                counted, and pose parameters, their moments and the calibration scalar are stepped (outside the scaler,
                                ace_trainer.py:634-640): everything but the head equals the control trainer's. The gradient scale is the
                                schedule wave's: it drops by 2^8 on the rank whose OWN chain overflowed and follows the rank's own largest
                                gradient elsewhere, so on this rank it equals the control's
  slot 3 = 1024, bf16           the flag means nothing without fp16: equals the control in everything

Every case carries its control: a twin trainer in the same state that receives the same bucket with slot 3 = 0 and must have moved
-- head parameters, pose parameters and the calibration scalar where the configuration trains them. No tolerance anywhere."""
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import head_oracle
from tests import helpers
from tests.test_head_gpu import _trainer

pytestmark = pytest.mark.gpu

N = 2048
# the configuration's name in helpers.HEAD_CONFIGS -> what the case changes in it
CONFIGS = {"head_tanh_1cyclepoly": {}, "head_tanh_calib": {}, "head_tanh_posemlp": {"refine_calibration": True},
           "head_tanh_posemlp_procrustes": {}, "head_tanh_posenaive": {}}
HEAD_KEYS = ("params", "m", "v", "w16", "opt_steps")   # what an fp16 overflow leaves alone
CASES = [(name, dtype, slot) for name in CONFIGS for dtype, slots in (("bf16", (1, 2, 1024)), ("fp16", (1, 2, 1025, 2049, 1024, 2048)))
         for slot in slots]

_cache = {}


def _problem():
    if "prob" not in _cache:
        prob = helpers.big_problem(n_images=8, patches_per_view=256)
        rng = np.random.default_rng(23)
        rows = prob["features"].shape[0]
        _cache["prob"] = prob
        _cache["flat0"] = head_oracle.init_params(helpers.SEED + 1)
        _cache["batches"] = [torch.from_numpy(rng.permutation(rows)[:N].astype(np.int64)).cuda() for _ in range(9)]
        _cache["empty"] = torch.zeros(0, dtype=torch.int64, device="cuda")
    return _cache["prob"], _cache["flat0"], _cache["batches"]


def _make(name, dtype, per_layer=False):
    """A trainer of the configuration after three healthy split steps (batches 0-2): the pose optimiser is enabled from the third on."""
    prob, flat0, batches = _problem()
    cfg = helpers.full_cfg(helpers.HEAD_CONFIGS[name], prob)
    cfg.update(global_batch=N, iterations=60, pose_refinement_wait=1)
    cfg.update(CONFIGS[name])
    if per_layer:
        os.environ["ACEZ_SEQ"] = "0"
    try:
        tr = _trainer(prob, flat0, cfg, max_batch=N, dtype=dtype)
    finally:
        os.environ.pop("ACEZ_SEQ", None)
    assert "diag" not in os.path.basename(tr.lib._name) and tr.seq_status()["enabled"] is not per_layer
    for b in batches[:3]:
        tr.backward(b)
        tr.update()
    return tr


def _peer(tr, inf):
    """What the other rank's bucket adds: finite leftovers of magnitude 1e3 in every slot, or infinities in a few head and pose entries."""
    g = torch.Generator().manual_seed(77)
    add = ((torch.rand(tr.grad.numel(), generator=g) * 2 - 1) * 1e3).cuda()
    if inf:
        add.zero_()
        where = [0, 262144 + 5, tr.n_params - 1]
        if tr.n_pose:
            where += [tr.n_params + 4, tr.n_params + 4 + tr.n_pose // 2, tr.n_params + 4 + tr.n_pose - 1]
        add[where] = float("inf")
    return add


def _deliver(tr, slot3, inf=False):
    """The all-reduce, emulated in place."""
    tr.grad.add_(_peer(tr, inf))
    tr.grad[tr.n_params + 3] = float(slot3)


def _close(tr, form):
    _, _, batches = _problem()
    if form == "update":
        tr.update()
    elif form == "next":
        tr.update(batches[4])          # the rows the following backward() does ask for
    elif form == "wrong":
        tr.update(batches[8])          # ... and rows it does not
    elif form == "empty":
        tr.update(_cache["empty"])
    else:
        tr.update_layers(0, tr.L)


def _run(name, dtype, slot3, form, inf=False):
    """(trainer, snapshot in front of the step, snapshot behind it): backward on batch 3, the emulated all-reduce, the update under
    test; after an abandoned step also a backward on batch 4, issued before any state read."""
    _, _, batches = _problem()
    tr = _make(name, dtype)
    before = helpers.trainer_snapshot(tr)
    tr.backward(batches[3])
    _deliver(tr, slot3, inf)
    _close(tr, form)
    if slot3 % 1024:
        tr.backward(batches[4])
    return tr, before, helpers.trainer_snapshot(tr)


def _assert_moved(tr, name, before, after, what):
    moved = helpers.snapshot_differences(before, after)
    want = {"params", "m", "v", "w16", "iteration", "opt_steps", "log"}
    if tr.n_pose:
        want |= {"pose_params", "pose_m", "pose_v", "poses"}
    if helpers.HEAD_CONFIGS[name]["refine_calibration"] or CONFIGS[name].get("refine_calibration"):
        want.add("focal_scale")
    assert want <= set(moved), (what, sorted(want - set(moved)))
    assert after["iteration"] == before["iteration"] + 1 == 4
    assert tr.seq_status() == {"enabled": True, "probe": 1, "faults": 0}


def _digests(snap):
    """A snapshot with its arrays replaced by digests of their bytes (what the cached controls keep: an array set is 30 MB)."""
    d = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return {k: d(v) if isinstance(v, np.ndarray) else tuple(d(x) for x in v) if isinstance(v, tuple) else v for k, v in snap.items()}


def _control(name, dtype, form, inf=False):
    """The twin that receives the same bucket with slot 3 = 0, once per (configuration, format, form): it must have moved.
    Returns the digests of its snapshots in front of and behind the step."""
    key = (name, dtype, form, inf)
    if key not in _cache:
        tr, before, after = _run(name, dtype, 0, form, inf)
        _assert_moved(tr, name, before, after, key)
        _cache[key] = (_digests(before), _digests(after))
    return _cache[key]


def _check(name, dtype, slot3, form, inf=False):
    c_before, c_after = _control(name, dtype, form, inf)
    tr, before, after = _run(name, dtype, slot3, form, inf)
    what = (name, dtype, slot3, form, inf)
    helpers.assert_snapshots_equal(_digests(before), c_before, what + ("the twins start from one state",))
    if slot3 % 1024:          # abandoned (it wins over an overflow flag in the same slot)
        helpers.assert_snapshots_equal(after, before, what + ("abandoned step",))
        assert tr.seq_status() == {"enabled": False, "probe": 1, "faults": 1}, what
    elif dtype == "fp16" and slot3 >= 1024:
        mine = _digests(after)
        for k in after:
            assert helpers.same_bits(after[k], before[k]) if k in HEAD_KEYS else helpers.same_bits(mine[k], c_after[k]), what + ("overflow only", k)
        assert after["iteration"] == before["iteration"] + 1
    else:
        helpers.assert_snapshots_equal(_digests(after), c_after, what + ("the overflow flag without fp16",))
    return tr, after


@pytest.mark.parametrize("name,dtype,slot3", CASES)
def test_update_on_a_reduced_bucket(name, dtype, slot3):
    """Every form that closes a split step: update(), update(next) with a right, a wrong and an empty announcement, update_layers."""
    for form in (("update", "next", "wrong", "empty", "layers") if slot3 in (1, 1024) else ("update", "next")):
        _check(name, dtype, slot3, form)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_infinities_in_an_abandoned_bucket_reach_nothing(name, dtype):
    _check(name, dtype, 1, "update", inf=True)
    _check(name, dtype, 1, "next", inf=True)


@pytest.mark.parametrize("form", ["update", "next"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_steps_after_the_skip_are_the_per_layer_trainers(name, dtype, form):
    """state() has performed the fall-back (inside _check's snapshot). Three more split steps are then bitwise -- over the whole
    snapshot -- those of a trainer created with ACEZ_SEQ=0 that went through the same three first steps and never saw batch 3
    (nor batch 4, whose backward ran under the fault word)."""
    _, _, batches = _problem()
    tr, after = _check(name, dtype, 1, form)
    ref = _make(name, dtype, per_layer=True)
    helpers.assert_snapshots_equal(helpers.trainer_snapshot(ref), after, (name, dtype, form, "per-layer twin in front of the skip"))
    for i, b in enumerate(batches[5:8]):
        for t in (tr, ref):
            t.backward(b)
            t.update(batches[6 + i] if form == "next" and i < 2 else None)
    got = helpers.trainer_snapshot(tr)
    helpers.assert_snapshots_equal(got, helpers.trainer_snapshot(ref), (name, dtype, form, "three steps behind the skip"))
    assert got["iteration"] == after["iteration"] + 3 and helpers.snapshot_differences(got, after)
    assert tr.seq_status() == {"enabled": False, "probe": 1, "faults": 1}


@pytest.mark.parametrize("form", ["update", "next"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_both_ranks_of_an_abandoned_step_stay_replicas(name, dtype, form):
    """The second trainer plays the abandoning rank without any switch: its bucket's slot 3 is 1.0, as the reduction tail of a rank whose
    poll expired leaves it, and its bucket otherwise holds whatever it held. Its own fault word is DOWN -- it, too, learns of the
    abandonment from the summed bucket, which is the case the word alone cannot decide. Both replicas stay where they were."""
    _, _, batches = _problem()
    a, b = _make(name, dtype), _make(name, dtype)
    before = helpers.trainer_snapshot(b)
    helpers.assert_snapshots_equal(helpers.trainer_snapshot(a), before, (name, dtype, "replicas in front of the step"))
    a.backward(batches[3])
    b.backward(batches[3])
    a.grad.add_(_peer(a, False))                # leftovers in the abandoning rank's bucket
    a.grad[a.n_params + 3] = 1.0
    assert float(b.grad[b.n_params + 3]) == 0.0
    total = a.grad + b.grad                     # the all-reduce
    assert float(total[a.n_params + 3]) == 1.0
    a.grad.copy_(total)
    b.grad.copy_(total)
    for t in (a, b):
        _close(t, form)
        t.backward(batches[4])
    sa, sb = helpers.trainer_snapshot(a), helpers.trainer_snapshot(b)
    helpers.assert_snapshots_equal(sa, sb, (name, dtype, form, "replicas behind the abandoned step"))
    helpers.assert_snapshots_equal(sb, before, (name, dtype, form, "abandoned step"))
    assert a.seq_status()["faults"] == 1 and b.seq_status()["faults"] == 1
    c = _make(name, dtype)                      # the control: the same summed bucket with a clean slot moves every trained tensor
    c.backward(batches[3])
    c.grad.copy_(total)
    c.grad[c.n_params + 3] = 0.0
    _close(c, form)
    _assert_moved(c, name, before, helpers.trainer_snapshot(c), (name, dtype, form, "control"))
