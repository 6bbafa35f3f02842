"""GPU: DSAC* RGB-D backward (acezero_amd/csrc/ransac_grad.hip) against the fp64 numpy restatement (tests/dsac_grad_restated.py) on
synthetic frames with noisy correspondences: the forward pass's hypotheses, probabilities, losses, inlier sets, expected loss and
gradient map; bitwise determinism, the += contract, single-call / batched / host agreement, and a short descent through
expected_pose_loss_rgbd."""
import numpy as np
import pytest
import torch

from acezero_amd import dsacstar
from tests import dsac_grad_restated as G
from tests.test_dsac_rgbd_gpu import make_frames

pytestmark = pytest.mark.gpu

THR, ALPHA, MAXD, SEED, WR, WT, CUT = 10.0, 100.0, 100.0, 1305, 1.0, 100.0, 100.0


def _cam_to_world(gt):
    return np.stack([np.linalg.inv(g) for g in gt]).astype(np.float32)


def _prm(hyps):
    return dict(hyps=hyps, thr=THR, alpha=ALPHA, max_reproj=MAXD, max_tries=16)


def _backward(sc, cc, gtc, hyps, ids, out=None):
    g, loss = dsacstar.register_batch_rgbd_backward(torch.from_numpy(sc).cuda(), torch.from_numpy(cc).cuda(), torch.from_numpy(gtc),
                                                    _prm(hyps), SEED, ids, WR, WT, CUT, out_grad=out)
    torch.cuda.synchronize()
    return g.cpu().numpy(), loss.cpu().numpy()


@pytest.mark.parametrize("shape,hyps", [((12, 16), 16), ((60, 80), 64)])
def test_backward_samples_the_forward_hypotheses(shape, hyps):
    sc, cc, gt = make_frames(11, n=2, h=shape[0], w=shape[1])
    ids = [5, 77]
    dsacstar.register_batch_rgbd(torch.from_numpy(sc).cuda(), torch.from_numpy(cc).cuda(), _prm(hyps), SEED, ids)
    fw = dsacstar.debug_fetch_rgbd(2, hyps)
    _backward(sc, cc, _cam_to_world(gt), hyps, ids)
    bw = dsacstar.debug_fetch_rgbd_backward(2, hyps, *shape)
    for k in ("samples", "hyp_poses", "scores"):
        assert np.array_equal(fw[k], bw[k]), k


# 96 x 128 cells: the valid lists do not fit the LDS and go to HBM (rgbd_grad_kernel<true>)
@pytest.mark.parametrize("shape,hyps,outliers", [((12, 16), 16, 0.3), ((60, 80), 64, 0.3), ((60, 80), 32, 0.6), ((96, 128), 16, 0.3)])
def test_against_the_restatement(shape, hyps, outliers):
    """E and the per-hypothesis losses to 1e-6 relative, probabilities to 1e-6 absolute, the inlier sets exactly, the gradient map to
    1e-4 of its norm (relative norm of the difference over the frame). The kernel rounds each distance to float inside the scores as
    the forward pass does; the restatement does not."""
    h, w = shape
    sc, cc, gt = make_frames(23 + h, n=2, h=h, w=w, outliers=outliers)
    gtc = _cam_to_world(gt)
    # perturb the scene coordinates so that the loss is not at its minimum: a 2 degree / 5 cm error of the whole map
    R = G.O.rodrigues(np.radians([1.2, -1.0, 0.8]))
    sc = (np.einsum("ij,njhw->nihw", R, sc) + np.array([0.05, -0.03, 0.02])[None, :, None, None]).astype(np.float32)
    ids = [9, 2 ** 33]
    g, loss = _backward(sc, cc, gtc, hyps, ids)
    dbg = dsacstar.debug_fetch_rgbd_backward(2, hyps, h, w)
    for f in range(2):
        ref = G.backward(sc[f], cc[f], gtc[f], hyps, THR, ALPHA, MAXD, SEED, ids[f], WR, WT, CUT)
        assert np.allclose(dbg["probs"][f], ref["probs"], rtol=0, atol=1e-6), f
        nv = len(ref["cells"])
        for hh in range(hyps):
            acc = ref["accs"][hh]
            assert np.array_equal(dbg["masks"][f, hh, :nv], acc if acc is not None else np.zeros(nv, bool)), (f, hh)
            assert not dbg["masks"][f, hh, nv:].any()
        assert np.allclose(dbg["losses"][f], ref["losses"], rtol=1e-6, atol=1e-9), f
        assert abs(loss[f] - ref["E"]) <= 1e-6 * max(1.0, abs(ref["E"])), (loss[f], ref["E"])
        ent = -sum(p * np.log2(p) for p in dbg["probs"][f] if p > 0)
        assert abs(dbg["entropy"][f] - ent) <= 1e-9 * max(1.0, ent)
        d = np.linalg.norm(g[f] - ref["grad_map"])
        assert np.linalg.norm(ref["grad_map"]) > 0
        assert d <= 1e-4 * np.linalg.norm(ref["grad_map"]), (f, d, np.linalg.norm(ref["grad_map"]))


def test_bitwise_deterministic_and_additive():
    sc, cc, gt = make_frames(5, n=3)
    gtc = _cam_to_world(gt)
    g1, l1 = _backward(sc, cc, gtc, 64, [1, 2, 3])
    g2, l2 = _backward(sc, cc, gtc, 64, [1, 2, 3])
    assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32)) and np.array_equal(l1, l2)
    assert np.abs(g1).max() > 0
    base = torch.full((3, 3, 60, 80), 0.25, device="cuda")
    g3, _ = _backward(sc, cc, gtc, 64, [1, 2, 3], out=base)
    assert np.array_equal(g3, (np.float32(0.25) + g1).astype(np.float32))


def test_single_call_batched_and_host_agree():
    sc, cc, gt = make_frames(8, n=2)
    gtc = _cam_to_world(gt)
    gb, lb = _backward(sc, cc, gtc, 64, [40, 41])
    for dev in ("cuda", "cpu"):
        dsacstar.reset_call_counter(40)
        for f in range(2):
            out = torch.zeros(1, 3, 60, 80, device=dev)
            e = dsacstar.backward_rgbd(torch.from_numpy(sc[f:f + 1]).to(dev), torch.from_numpy(cc[f:f + 1]).to(dev), out,
                                       torch.from_numpy(gtc[f]), 64, THR, WR, WT, CUT, ALPHA, MAXD, SEED)
            assert e == lb[f], (dev, f)
            assert np.array_equal(out[0].cpu().numpy(), gb[f]), (dev, f)


def _pose_error(est, gtc):
    dR = est[:3, :3] @ gtc[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))
    return ang + 100 * np.linalg.norm(est[:3, 3] - gtc[:3, 3])


def test_descent_through_expected_pose_loss_rgbd():
    """25 Adam steps (lr 4 mm) on scene coordinates carrying a 3 degree / 10 cm error of the whole map: the expected loss falls below
    half of its start and the pose register_batch_rgbd returns moves toward the ground truth (its error at least halves)."""
    sc, cc, gt = make_frames(31, n=2)
    gtc = _cam_to_world(gt)
    R = G.O.rodrigues(np.radians([2.0, -1.5, 1.2]))
    sc = (np.einsum("ij,njhw->nihw", R, sc) + np.array([0.1, 0.0, -0.05])[None, :, None, None]).astype(np.float32)
    coords = torch.from_numpy(sc).cuda().requires_grad_(True)
    camc = torch.from_numpy(cc).cuda()
    gtt = torch.from_numpy(gtc)

    def pose_err():
        p, _, _ = dsacstar.register_batch_rgbd(coords.detach(), camc, _prm(64), SEED, [0, 1], want_masks=False)
        return sum(_pose_error(p[f].cpu().numpy(), gtc[f]) for f in range(2))
    err0 = pose_err()
    opt = torch.optim.Adam([coords], lr=0.004)
    losses = []
    for step in range(25):
        opt.zero_grad()
        loss = dsacstar.expected_pose_loss_rgbd(coords, camc, gtt, 64, THR, WR, WT, CUT, ALPHA, MAXD, seed=SEED,
                                                frame_ids=[1000 * step, 1000 * step + 1]).sum()
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
    assert losses[-1] < losses[0] / 2, losses
    assert pose_err() < err0 / 2, (err0, pose_err())
