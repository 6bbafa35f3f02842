"""GPU: a HeadGroup step is bitwise what HeadTrainer.step on each member, one after the other, produces -- weights, optimiser state,
16-bit copies, the step's activations and gradients, schedule state, log and scene coordinates -- for mixed member configurations,
announced batches, ragged batch sizes, single and group steps mixed, and with the one-launch chains off."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from acezero_amd import _native as N
from acezero_amd import synth
from acezero_amd.head import HeadGroup, HeadTrainer
from tests import helpers

pytestmark = pytest.mark.gpu

ROWS = 10240   # a seed trial's buffer: one image, 10 passes x 1024 samples


def _member(k, dtype, iterations=40, batch=5120, **over):
    """Member k: its own problem, weights and settings (tanh / dyntanh alternate, even members with depth targets)."""
    prob = synth.make_training_problem(seed=2089 + 97 * k, n_images=10, views_per_image=2, patches_per_view=ROWS // 20)
    kw = dict(loss_type="tanh" if k % 2 == 0 else "dyntanh", schedule="1cyclepoly", lr_min=0.0001, lr_max=0.003, warmup_iterations=5,
              warmup_lr=0.0005, cooldown_iterations=10, cooldown_trigger_percent=0.7, iterations=iterations, max_batch=5120,
              global_batch=batch, dtype=dtype)
    kw.update(over)
    tr = HeadTrainer(prob["mean"], **kw)
    g = torch.Generator().manual_seed(1023 + k)
    tr.load_flat((torch.rand(tr.n_params, generator=g) * 2 - 1) / math.sqrt(512.0))
    if not kw.get("inference_only"):
        tr.set_buffer(prob["features"], prob["target_px"], prob["view_idx"], prob["view_aug_inv"], prob["view_K"], prob["view_Kinv"],
                      prob["view_image"], prob["image_pose_inv"], target_crds=prob["target_crds"] if k % 2 == 0 else None)
    return tr


def _batches(k, n, steps):
    g = torch.Generator(device="cuda").manual_seed(8191 + k)
    return [torch.randperm(ROWS, generator=g, device="cuda")[:n].contiguous() for _ in range(steps + 1)]


def _snapshot(tr, n):
    out = helpers.trainer_snapshot(tr)   # the trained state; below: what the last step left in the trainer's work buffers
    for l in range(tr.L):
        if l < 3 * (tr.nb + 1) and l % 3 == 2:
            continue    # (a block's last activation is not stored by a training forward, only its mask bits)
        out[f"out{l}"] = tr.debug_read("out", l, n)
        out[f"dZ{l}"] = tr.debug_read("dZ", l, n)
    for b in range(tr.nb + 2):
        out[f"R{b}"] = tr.debug_read("R", b, n)
    out["xyz"] = tr.last_scene_coords(n).view(np.int32).copy()
    return out


_assert_same = helpers.assert_snapshots_equal


def _run(dtype, H, steps=40, announce=False, sizes=None, iters=None, mixed=False):
    """H members stepped as a group, H clones stepped alone; compared every 10 steps. Returns the group members' last snapshots."""
    sizes = sizes or [5120] * H
    iters = iters or [25 if k == 1 else steps for k in range(H)]
    grp_m = [_member(k, dtype, iters[k], sizes[k]) for k in range(H)]
    ref_m = [_member(k, dtype, iters[k], sizes[k]) for k in range(H)]
    batches = [_batches(k, sizes[k], steps) for k in range(H)]
    snaps = None
    with HeadGroup(grp_m) as grp:
        for s in range(steps):
            nxt = [batches[k][s + 1] for k in range(H)] if announce else None
            if mixed and s in (12, 13):
                # single steps on member 0 between group steps: the group's bookkeeping of the member must be what its own step leaves
                grp_m[0].step(batches[0][s], nxt[0] if nxt else None)
                ref_m[0].step(batches[0][s], nxt[0] if nxt else None)
                continue
            grp.step([batches[k][s] for k in range(H)], nxt)
            for k in range(H):
                ref_m[k].step(batches[k][s], nxt[k] if nxt else None)
            if (s + 1) % 10 == 0:
                snaps = [_snapshot(t, sizes[k]) for k, t in enumerate(grp_m)]
                for k in range(H):
                    _assert_same(snaps[k], _snapshot(ref_m[k], sizes[k]), (dtype, H, s, k))
    return snaps


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("H", [1, 2, 3, 5])
def test_group_step_is_bitwise_the_members_own_steps(dtype, H):
    _run(dtype, H)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("H", [2, 3])
def test_announced_next_batches(dtype, H):
    _run(dtype, H, announce=True)


@pytest.mark.parametrize("announce", [False, True])
def test_ragged_batch_sizes_in_one_group(announce):
    _run("bf16", 3, sizes=[5120, 4096, 512], announce=announce)


@pytest.mark.parametrize("announce", [False, True])
def test_single_and_group_steps_mixed(announce):
    _run("bf16", 3, announce=announce, mixed=True)


def test_schedule_end_inside_the_run_stops_only_that_member():
    H = 3
    ms = [_member(k, "bf16", iterations=(12 if k == 1 else 40)) for k in range(H)]
    batches = [_batches(k, 5120, 30) for k in range(H)]
    with HeadGroup(ms) as grp:
        for s in range(30):
            grp.step([batches[k][s] for k in range(H)])
    alone = _member(1, "bf16", iterations=12)
    for s in range(30):
        alone.step(batches[1][s])
    ended = alone.state()["iteration"]
    assert ended < 30
    assert [m.state()["iteration"] for m in ms] == [30, ended, 30]


def test_per_layer_flow_is_bitwise_the_chained_one(monkeypatch):
    chained = _run("bf16", 3, steps=20, announce=True)
    monkeypatch.setenv("ACEZ_SEQ", "0")
    per_layer = _run("bf16", 3, steps=20, announce=True)
    for k in range(3):
        _assert_same(per_layer[k], chained[k], ("per-layer vs chained", k))


def _create(members, h=None):
    lib = N.lib()
    h = len(members) if h is None else h
    arr = (C.c_void_p * max(h, 1))(*[m._h.value for m in members][:max(h, 1)])
    g = C.c_void_p()
    rc = lib.acez_train_group_create(C.byref(g), arr, h)
    if rc == 0:
        lib.acez_train_group_destroy(g)
    return rc


def test_refusals_change_nothing():
    a, b = _member(0, "bf16"), _member(1, "bf16")
    ra, rb = _member(0, "bf16"), _member(1, "bf16")
    refused = [
        [_member(2, "fp16")],                                        # compute_dtype
        [_member(2, "bf16", num_head_blocks=2)],                     # num_head_blocks
        [_member(2, "bf16", use_homogeneous=False)],                 # use_homogeneous
        [_member(2, "bf16", pose_refinement="mlp")],                 # pose refinement
        [_member(2, "bf16", refine_calibration=True)],               # calibration refinement
        [_member(2, "bf16", inference_only=True)],                   # inference-only context
        [a],                                                         # the same trainer twice
    ]
    for extra in refused:
        assert _create([a, b] + extra) == -1, extra
        with pytest.raises(N.AcezError):
            HeadGroup([a, b] + extra)
    assert _create([a, b], h=0) == -1
    nine = [_member(2 + k, "bf16", iterations=4) for k in range(7)]
    assert _create([a, b] + nine) == -1
    # the refusals touched nothing: group steps on a and b still equal their clones' own steps
    batches = [_batches(k, 5120, 10) for k in range(2)]
    with HeadGroup([a, b]) as grp:
        for s in range(10):
            grp.step([batches[0][s], batches[1][s]])
            ra.step(batches[0][s])
            rb.step(batches[1][s])
    _assert_same(_snapshot(a, 5120), _snapshot(ra, 5120), "a after refusals")
    _assert_same(_snapshot(b, 5120), _snapshot(rb, 5120), "b after refusals")
