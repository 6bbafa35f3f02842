"""GPU: the loss stage of the head's training step (head_kernels.hip loss_body: fc3, the de-homogenisation, the projection, every loss
branch, ds, dZ of fc2, the fc3 / bias / statistics partials) judged per row and per element from its own operands by
tests/loss_stage_restated.py; the checker itself is proven on the CPU by tests/test_loss_stage_cpu.py on the same inputs
(tests/loss_stage_cases.py).

A configuration runs all its row counts in turn, a trainer per row count (global_batch, which is the row count here, is fixed at creation).
Each trainer first runs a full-size backward() over every buffer row: it fills the rows and partial slots past n with another batch's
values, and its scene coordinates are what the rows' poses, intrinsics and targets are then planted around (X depends on the features and
the weights only: it must come out bit for bit the same under the planted tables).

The second test carries the bitwise net of tests/test_loss_in_chain_gpu.py and tests/test_step_chain_gpu.py from one configuration to
all of them: the same observables after the other launch forms of loss_body must equal the backward() run's bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import loss_stage_cases as C
from tests import loss_stage_restated as ls

pytestmark = pytest.mark.gpu

F2 = 7          # fc2, the last wide layer of a head with one block
N_WIDE = 8 * 262656


def _trainer(name, dtype, n, env=None, poses=None):
    """poses [NBUF,16]: the parameters of a pose configuration (pose_refinement 'naive': the world -> camera matrices themselves)."""
    from acezero_amd.head import HeadTrainer
    cfg = C.CONFIGS[name]
    pose = {}
    if cfg.get("pose"):
        p0 = C.plant(name, np.zeros((C.NBUF, 3), np.float32))["T0"] if poses is None else poses
        pose = dict(pose_refinement="naive", initial_poses=np.ascontiguousarray(p0.reshape(-1, 4, 4)[:, :3]))
    feats, flat, _ = C.head_inputs(dtype, cfg["homog"])
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        tr = HeadTrainer(C.MEAN, num_head_blocks=1, use_homogeneous=cfg["homog"], max_batch=C.NBUF, global_batch=n, loss_type=cfg["loss_type"],
                         soft_clamp=50.0, soft_clamp_min=1.0, schedule="constant", iterations=100, lr_min=1e-4, lr_max=1e-3,
                         refine_calibration=cfg["calib"], focal_init=C.FOCAL_INIT, dtype=dtype, **pose)
    finally:
        for k in (env or {}):
            os.environ.pop(k, None)
    tr.load_flat(flat)
    assert "diag" not in os.path.basename(tr.lib._name)
    return tr, feats, flat


def _set_buffer(tr, feats, tabs):
    ar = np.arange(C.NBUF, dtype=np.int32)
    tr.set_buffer(feats, np.stack([tabs["tu"], tabs["tv"]], 1), ar, tabs["A"].reshape(-1, 3, 4), tabs["K"].reshape(-1, 3, 3),
                  tabs["Ki"].reshape(-1, 3, 3), ar, tabs["T0"].reshape(-1, 4, 4), target_crds=tabs["tc"])


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int64)).cuda()


def _full_pass(tr, feats, name, n):
    """A backward() over every buffer row under placeholder tables; the kernel's X per BUFFER row."""
    full, _ = C.batch_indices(n)
    _set_buffer(tr, feats, C.plant(name, np.zeros((C.NBUF, 3), np.float32)))
    tr.backward(_cuda(full))
    torch.cuda.synchronize()
    X = np.zeros((C.NBUF, 3), np.float32)
    X[full] = tr.last_scene_coords(C.NBUF)
    return X


@functools.lru_cache(maxsize=None)
def _planted(name, dtype):
    """(X of every buffer row as the kernel computes it, the tables planted around it), from a trainer of its own."""
    tr, feats, _ = _trainer(name, dtype, C.NBUF)
    X = _full_pass(tr, feats, name, C.NBUF)
    tr.close()
    assert np.isfinite(X).all()
    tabs = C.plant(name, X)
    if C.CONFIGS[name].get("pose"):
        # the loss reads the device's orthonormalisation of the planted matrices: a trainer with them as its parameters computes it in a
        # backward(), and the pixel targets are planted around the projection through THOSE matrices
        tr, feats, _ = _trainer(name, dtype, C.NBUF, poses=tabs["T0"])
        _set_buffer(tr, feats, tabs)
        tr.backward(_cuda(C.batch_indices(C.NBUF)[0]))
        torch.cuda.synchronize()
        poses = tr.debug_read("pose_cur", 0, C.NBUF)
        tr.close()
        assert np.isfinite(poses).all() and np.abs(poses - tabs["T0"]).max() < 1e-3 * max(1.0, np.abs(tabs["T0"]).max())
        tabs = C.plant(name, X, poses=poses)
    return X, tabs


def _observe(tr, n, no, pose=False):
    torch.cuda.synchronize()
    nblk = (n + ls.BLOCK - 1) // ls.BLOCK
    extra = dict(row_dT=tr.debug_read("row_dT", 0, n), row_image=tr.debug_read("row_image", 0, n)) if pose else {}
    return dict(**extra, X=tr.last_scene_coords(n), dZ=tr.debug_read("dZ", F2, n), bias_partials=tr.debug_read("bias_partials", F2, nblk),
                fc3_partials=tr.debug_read("fc3_partials", 0, nblk)[:, :no * 513], stat_partials=tr.debug_read("stat_partials", 0, nblk)[:, :3])


def _judge(name, dtype, n):
    cfg = C.CONFIGS[name]
    no = 4 if cfg["homog"] else 3
    X_all, tabs = _planted(name, dtype)
    tr, feats, flat = _trainer(name, dtype, n, poses=tabs["T0"])
    assert np.array_equal(_full_pass(tr, feats, name, n).view(np.uint32), X_all.view(np.uint32)), "X depends on more than features and weights"
    _, idx = C.batch_indices(n)
    _set_buffer(tr, feats, tabs)
    st = tr.state()
    assert st["iteration"] == 0 and not st["nan"]
    c = C.scalars(name, dtype, n, grad_scale=st["grad_scale"], calib_g=st["focal_scale"] - 1.0)
    tr.backward(_cuda(idx))
    cap = _observe(tr, n, no, cfg.get("pose"))
    assert np.array_equal(cap["X"].view(np.uint32), X_all[idx].view(np.uint32)), "X changed with the planted tables"
    if cfg.get("pose"):     # the matrices the loss read are the ones the targets were planted around
        assert np.array_equal(tr.debug_read("pose_cur", 0, C.NBUF).view(np.uint32), tabs["T"].view(np.uint32))
        cap["row_image_want"] = idx.astype(np.int32)
    grad = tr.grad.detach().cpu().numpy().copy()
    cap.update(out16=tr.debug_read("out", F2, n), W3=tr.debug_read("W3", 0, 0), b3=flat[N_WIDE + no * 512:].numpy().copy(),
               grad_fc3=grad[N_WIDE:N_WIDE + no * 513], grad_stats=grad[tr.n_params:tr.n_params + 3])
    tr.update()
    st2 = tr.state()
    assert st2["opt_steps"] == 1 or dtype == "fp16", "update() after backward() did not step"
    if st2["opt_steps"] == 1:      # (fp16 only: a step whose gradients overflow is abandoned as designed and logs nothing)
        cap.update(state_loss=st2["loss"], state_inliers=st2["batch_inliers"], global_batch=n)
    tr.close()
    V, und, o = ls.judge(ls.Fmt(dtype), cap, C.batch_tables(tabs, idx), c, n, no)
    what = "%s %s n=%d" % (name, dtype, n)
    print("\n".join(V.lines(what)))
    print("LOSS-STAGE %s: %d of %d rows undecided" % (what, int(und.sum()), n))
    assert not V.failed(), "\n".join(V.lines(what))
    return und, C.branch_counts(cfg, o["rec"], ~und)


def _cases():
    return [pytest.param(n, "bf16", id="%s-bf16" % n) for n in C.CONFIGS] + [pytest.param(n, "fp16", id="%s-fp16" % n) for n in C.FP16_CONFIGS]


@pytest.mark.parametrize("name,dtype", _cases())
def test_every_row_and_element_of_the_loss_stage_lies_in_its_interval(name, dtype):
    und_rows, rows, branches = 0, 0, {}
    for n in C.ROWS:
        und, br = _judge(name, dtype, n)
        und_rows, rows = und_rows + int(und.sum()), rows + n
        for k, v in br.items():
            branches[k] = branches.get(k, 0) + v
    print("LOSS-STAGE %s %s: undecided share %.5f, decided rows per branch %r" % (name, dtype, und_rows / rows, branches))
    assert und_rows <= C.UNDECIDED_CAP * rows, "%d of %d rows undecided" % (und_rows, rows)
    thin = {k: v for k, v in branches.items() if v < C.BRANCH_MIN}
    assert not thin, "branches with fewer than %d decided rows: %r" % (C.BRANCH_MIN, thin)


# launch form -> (environment at creation, profiling, the next batch announced)
FORMS = {
    "loss_kernel": ({"ACEZ_LOSS_IN_CHAIN": "0"}, True, False),
    "loss_gather_kernel": ({"ACEZ_LOSS_IN_CHAIN": "0"}, True, True),
    "rowseq_loss_kernel": ({"ACEZ_STEP_CHAIN": "0"}, True, True),
    "rowstep_kernel": ({"ACEZ_STEP_CHAIN": "1"}, False, True),
}


# pose refinement keeps the loss in a launch of its own (the one-launch forms need the fused optimiser, which it excludes)
POSE_FORMS = {"loss_kernel": ({}, True, False), "loss_gather_kernel": ({}, True, True)}


def _state(tr):
    st = tr.state()
    return {k: st[k] for k in ("loss", "batch_inliers", "opt_steps", "nan")}


def _form(name, dtype, n, form, tabs):
    pose = C.CONFIGS[name].get("pose")
    env, profiling, announce = (POSE_FORMS if pose else FORMS)[form]
    no = 4 if C.CONFIGS[name]["homog"] else 3
    tr, feats, _ = _trainer(name, dtype, n, env, poses=tabs["T0"])
    _set_buffer(tr, feats, tabs)
    full, idx = C.batch_indices(n)
    assert tr.seq_status()["enabled"]
    tr.set_profiling(profiling)
    tr.step(_cuda(idx), _cuda(full[:n]) if announce else None)
    got = _observe(tr, n, no, pose)
    got["state"] = _state(tr)
    prof, status = tr.get_profile(), tr.seq_status(step_chain=True)
    assert status["faults"] == 0
    # the form under test is the one that ran
    if form in ("loss_kernel", "loss_gather_kernel"):
        assert prof["loss"][1] == 1 and prof["loss"][0] > 0.0 and status["step_chain_steps"] == 0
    elif form == "rowseq_loss_kernel":
        assert prof["loss"] == (0.0, 0) and prof["gemm_dgrad"][0] > 0.0 and status["step_chain_steps"] == 0
    else:
        assert status["step_chain_steps"] == 1
    tr.close()
    return got


def _backward_form(name, dtype, n, tabs):
    no = 4 if C.CONFIGS[name]["homog"] else 3
    pose = C.CONFIGS[name].get("pose")
    tr, feats, _ = _trainer(name, dtype, n, poses=tabs["T0"])
    _set_buffer(tr, feats, tabs)
    tr.backward(_cuda(C.batch_indices(n)[1]))
    got = _observe(tr, n, no, pose)
    tr.update()
    got["state"] = _state(tr)      # loss and inlier fraction of the closed step: the reduced statistics of the same partials
    assert got["state"]["opt_steps"] == 1 or dtype == "fp16"
    tr.close()
    return got


@pytest.mark.parametrize("name,dtype", _cases())
def test_every_launch_form_of_the_loss_gives_the_bits_of_backward(name, dtype):
    """357 rows: five row tiles, 23 loss blocks, a ragged last block. tanh-homog also runs one block, one row past a tile and 65 blocks."""
    _, tabs = _planted(name, dtype)
    for n in ((16, 81, 357, 1025) if name == "tanh-homog" else (357,)):
        want = _backward_form(name, dtype, n, tabs)
        for form in (POSE_FORMS if C.CONFIGS[name].get("pose") else FORMS):
            got = _form(name, dtype, n, form, tabs)
            state = got.pop("state")
            assert state == want["state"], "%s %s n=%d: state() after %s: %r, after backward() + update(): %r" % (name, dtype, n, form, state, want["state"])
            for k in got:
                a, b = np.ascontiguousarray(want[k]), np.ascontiguousarray(got[k])
                same = a.view(np.uint8) == b.view(np.uint8)
                assert same.all(), "%s %s n=%d: %s after %s differs from backward() in %d bytes" % (name, dtype, n, k, form, int((~same).sum()))
