"""CPU: the head oracle (fp32 mode) against the golden vectors produced by the reference's own training_step."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import head_oracle
from tests import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(helpers.HEAD_CONFIGS) + list(helpers.TRAINED_CONFIGS))
def test_oracle_fp32_matches_reference_golden(name, golden_dir):
    """The first steps are compared at tolerances that a different sgemm code path or thread count exceeds, and MKL picks its kernels by
    CPU vendor and model. So the comparison runs in a child process on MKL's COMPATIBLE branch, which computes the same sgemm bits on every
    x86-64 host, and on a fixed number of threads (the split of the reductions); the fixtures were made on that branch
    (tests/golden/make_head_golden.py --compatible-sgemm)."""
    code = "import sys; sys.path.insert(0, %r); from tests.test_head_oracle import check_against_golden; check_against_golden(%r, %r)" % (
        ROOT, name, golden_dir)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MKL_CBWR="COMPATIBLE", OMP_NUM_THREADS="8", MKL_NUM_THREADS="8"), capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]


def check_against_golden(name, golden_dir):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    prob, flat0, cfg = helpers.problem_for(name)
    batches = helpers.golden_batches(prob, cfg["steps"])
    pose_flat = None
    if cfg["pose_refinement"] == "mlp":
        from acezero_amd.head import init_pose_network
        pose_flat = init_pose_network(helpers.SEED + 3)
    if cfg["pose_refinement"] == "naive":
        pose_flat = torch.from_numpy(prob["image_pose_inv"][:, :3].reshape(-1).copy())
    tr = head_oracle.TrainerOracle(flat0.clone(), prob["mean"], cfg, mode="fp32", pose_flat=pose_flat, image_pose_inv=prob["image_pose_inv"])
    losses, inl, lrs, maxit, focal = [], [], [], [], []
    snaps = {}
    for it, idx in enumerate(batches):
        b = helpers.torch_batch(prob, idx)
        if it == 0:
            X0 = tr.head.scene_coordinates(b["features"])[:64].numpy()
            np.testing.assert_allclose(X0, g["coords0"], rtol=1e-4, atol=1e-4)
        rec = tr.step(b["features"], b)
        maxit.append(tr.sched.max_iterations)
        focal.append(1.0 + tr.sched.calib_g)
        if rec is None:
            break
        losses.append(rec["loss"]); inl.append(rec["inliers"]); lrs.append(rec["lr"])
        if cfg["pose_refinement"] in ("mlp", "naive"):
            # refined poses and the pose parameters after this step vs the reference's PoseRefiner
            np.testing.assert_allclose(tr.current_poses().numpy(), g["poses"][it], atol=5e-5 if it < 4 else 5e-4)
            stride = 97 if tr.pose.flat.numel() > 1000 else 1
            np.testing.assert_allclose(tr.pose.flat.detach().numpy()[::stride], g["pose_params_sel"][it], atol=2e-6 if it < 3 else 3e-3)
        snaps[it] = tr.head.p.flat.clone().numpy()
    assert len(losses) == int(g["steps_run"])
    if name in helpers.TRAINED_CONFIGS:
        assert min(inl) > 0.8, "the trained-regime fixtures exist to exercise batch_inliers > 0.7"
    if name == "head_trained_1cyclepoly":
        # the cool-down trigger fired on real inlier counts (ace_schedule.py:86-101): max_iterations = 3 + 6, training stopped there
        assert maxit[-1] == 9 and len(losses) == 9 and int(g["max_iterations"][-1]) == 9
    np.testing.assert_allclose(lrs, g["lr"], rtol=1e-12)
    np.testing.assert_array_equal(maxit, g["max_iterations"])
    np.testing.assert_allclose(inl, g["inliers"], atol=1.5 / helpers.B)
    # the first steps pin the arithmetic; later ones only bound the drift (mask/sign flips amplify 1e-7 differences)
    # (trained regime: the first loss pins the arithmetic; from the second step on the tiny gradients of a converged problem make
    # AdamW's m / (sqrt(v) + eps) amplify last-bit differences -- 1e-4 relative on the loss, measured)
    np.testing.assert_allclose(losses[:1], g["loss"][:1], rtol=2e-5)
    np.testing.assert_allclose(losses[:5], g["loss"][:5], rtol=3e-4 if name in helpers.TRAINED_CONFIGS else 2e-5)
    np.testing.assert_allclose(losses, g["loss"], rtol=3e-2)
    sel = g["param_sel"]
    np.testing.assert_allclose(snaps[0][sel], g["params_after_first"], rtol=0, atol=2e-6)
    # after several AdamW steps sign flips of tiny gradients can move single weights by ~lr; compare robustly
    d = np.abs(snaps[int(g["last_it"])][sel] - g["params_after_last"])
    moved = np.abs(snaps[int(g["last_it"])][sel] - flat0.numpy()[sel]).mean()
    assert np.median(d) < 0.05 * moved and d.max() < 0.02, (np.median(d), moved, d.max())
    np.testing.assert_allclose(focal, g["focal_scale"], rtol=0, atol=2e-5)


def test_bf16_mode_close_to_fp32():
    prob, flat0 = helpers.golden_problem()
    idx = helpers.golden_batches(prob, 1)[0]
    b = helpers.torch_batch(prob, idx)
    h32 = head_oracle.HeadOracle(flat0.clone(), prob["mean"], mode="fp32")
    h16 = head_oracle.HeadOracle(flat0.clone(), prob["mean"], mode="bf16")
    X32, X16 = h32.scene_coordinates(b["features"]), h16.scene_coordinates(b["features"])
    rel = (X32 - X16).norm() / (X32 - torch.from_numpy(prob["mean"])).norm()
    assert rel < 0.05


@pytest.mark.parametrize("name", list(helpers.BIG_CONFIGS))
def test_oracle_fp32_matches_reference_golden_at_the_baseline_batch(name, golden_dir):
    """BASELINE's batch of 5120 rows: three steps of the reference's own training_step (tests/golden/make_head_golden.py); six for the
    step ace_zero.py runs in every non-seed round (pose MLP + focal refinement on 200 images), with the refined poses of every image."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    prob, flat0, cfg = helpers.problem_for(name)
    pose_flat = None
    if cfg["pose_refinement"] == "mlp":
        from acezero_amd.head import init_pose_network
        pose_flat = init_pose_network(helpers.SEED + 3)
    tr = head_oracle.TrainerOracle(flat0.clone(), prob["mean"], cfg, mode="fp32", pose_flat=pose_flat, image_pose_inv=prob["image_pose_inv"])
    losses, inl, lrs, focal = [], [], [], []
    for it, idx in enumerate(helpers.big_batches(prob, cfg["steps"])):
        assert len(idx) == helpers.BIG_B
        b = helpers.torch_batch(prob, idx)
        if it == 0:
            np.testing.assert_allclose(tr.head.scene_coordinates(b["features"])[:64].numpy(), g["coords0"], rtol=1e-4, atol=1e-4)
        rec = tr.step(b["features"], b)
        losses.append(rec["loss"]); inl.append(rec["inliers"]); lrs.append(rec["lr"]); focal.append(1.0 + tr.sched.calib_g)
        if it == 0:
            d = np.abs(tr.head.p.flat.numpy()[g["param_sel"]] - g["params_after_first"])
            # the first AdamW step moves a weight by lr * g / (|g| + 1e-8): a weight whose gradient is at the 1e-8 level follows the last bits of
            # the summation order (here: autograd's) -- one such weight among the 2110 sampled in the refinement configuration
            assert d.max() < (2.5e-5 if pose_flat is not None else 2e-6) and (d > 2e-6).mean() < 2e-3, (d.max(), (d > 2e-6).mean())
        if pose_flat is not None:
            # the refined poses of all 200 images and the pose network's parameters after this step, vs the reference's PoseRefiner
            assert g["poses"].shape[1] == prob["image_pose_inv"].shape[0] >= 200
            # (refined poses: exact until the first pose update; from then on a few sign-flipped +-lr weights move every pose by a few 1e-3
            # per update -- the reference's own trajectory is that sensitive to the last bits of its first pose gradients)
            upd = it - cfg["pose_refinement_wait"]
            np.testing.assert_allclose(tr.current_poses().numpy(), g["poses"][it], atol=5e-5 if upd <= 0 else 5e-3 * upd)
            # (the pose network's first AdamW steps move every weight by +-lr = 1e-3 with the sign of its gradient: a weight whose gradient is
            # at the rounding level may take the other sign -- a few of the 732 sampled weights, each off by 2 lr per such step)
            dp = np.abs(tr.pose.flat.detach().numpy()[::97] - g["pose_params_sel"][it])
            updates = it - cfg["pose_refinement_wait"]     # pose-network updates applied so far
            if updates <= 0:
                assert dp.max() < 2e-6, (it, dp.max())
            elif updates == 1:
                assert dp.max() < 3e-3 and (dp > 2e-6).mean() < 0.02, (it, dp.max(), (dp > 2e-6).mean())
            else:   # (the flipped weights have moved the poses, hence every later gradient: bounded drift)
                assert dp.max() < 5e-3 and np.median(dp) < 3e-4, (it, dp.max(), np.median(dp))
    np.testing.assert_allclose(lrs, g["lr"], rtol=1e-12)
    np.testing.assert_allclose(losses[:1], g["loss"][:1], rtol=2e-5)
    if pose_flat is None:
        np.testing.assert_allclose(inl, g["inliers"], atol=1.5 / helpers.BIG_B)
        np.testing.assert_allclose(losses, g["loss"], rtol=3e-4)
        np.testing.assert_allclose(focal, g["focal_scale"], atol=2e-6)
    else:
        # identical (1e-6) through the first pose update's forward; behind it the sign-flipped pose weights separate the two fp32 trajectories:
        # measured 0.45 % on the loss, 2 rows of 5120 on the inlier count, 2.6e-4 on the focal scale after four pose updates
        k = cfg["pose_refinement_wait"] + 2
        np.testing.assert_allclose(losses[:k], g["loss"][:k], rtol=2e-5)
        np.testing.assert_allclose(focal[:k], g["focal_scale"][:k], atol=2e-6)
        np.testing.assert_allclose(losses, g["loss"], rtol=1e-2)
        np.testing.assert_allclose(inl, g["inliers"], atol=3.5 / helpers.BIG_B)
        np.testing.assert_allclose(focal, g["focal_scale"], atol=5e-4)
