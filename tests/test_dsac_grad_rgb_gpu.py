"""GPU: DSAC* RGB backward (the GRAD instantiation of ransac_kernel in acezero_amd/csrc/ransac_api.hip) against the fp64 numpy
restatement (tests/dsac_grad_restated.rgb_backward) on synthetic room frames with noisy scene coordinates and outliers: the forward
pass's hypotheses, the probabilities, losses, expected loss and gradient map; the refined poses and inlier sets against the
forward refinement; bitwise determinism, +=, single-call / batched / host agreement, and a short descent through
expected_pose_loss_rgb."""
import numpy as np
import pytest
import torch

from acezero_amd import dsacstar, synth
from tests import dsac_grad_restated as G

pytestmark = pytest.mark.gpu

THR, ALPHA, MAXR, SUB, SEED, WR, WT, CUT = 10.0, 100.0, 100.0, 8, 1305, 1.0, 100.0, 100.0


def _frames(seed, n=2, h=60, w=80, shift=True):
    fr = synth.make_registration_frames(seed=seed, n_frames=n, h=h, w=w)
    sc = fr["scene_coords"]
    if shift:   # a 1.5 degree / 5 cm error of the whole map, so that the loss is not at its minimum
        R = G.O.rodrigues(np.radians([0.8, -1.0, 0.6]))
        sc = (np.einsum("ij,njhw->nihw", R, sc) + np.array([0.05, -0.02, 0.03])[None, :, None, None]).astype(np.float32)
    return sc, np.asarray(fr["poses"], np.float32), [(fr["focal"], fr["ppx"], fr["ppy"])] * n, fr


def _prm(hyps):
    return dict(hyps=hyps, thr=THR, alpha=ALPHA, max_reproj=MAXR, sub=SUB, max_tries=16)


def _backward(sc, gt, intr, hyps, ids, out=None):
    g, loss = dsacstar.register_batch_backward(torch.from_numpy(sc).cuda(), intr, torch.from_numpy(gt), _prm(hyps), SEED, ids, WR, WT,
                                               CUT, out_grad=out)
    torch.cuda.synchronize()
    return g.cpu().numpy(), loss.cpu().numpy()


@pytest.mark.parametrize("shape,hyps", [((12, 16), 16), ((60, 80), 64)])
def test_backward_samples_and_refines_as_forward(shape, hyps):
    """The sampled poses and scores are the forward pass's; the refined pose and inlier map of the forward's selected hypothesis are
    the forward's refinement, bit for bit."""
    sc, gt, intr, _ = _frames(11, h=shape[0], w=shape[1])
    ids = [5, 77]
    dsacstar.register_batch(torch.from_numpy(sc).cuda(), intr, _prm(hyps), SEED, ids)
    torch.cuda.synchronize()
    fw = dsacstar.debug_fetch(2, hyps)
    poses, inl, masks = dsacstar.register_batch(torch.from_numpy(sc).cuda(), intr, _prm(hyps), SEED, ids)
    masks = masks.cpu().numpy()
    _backward(sc, gt, intr, hyps, ids)
    bw = dsacstar.debug_fetch_rgb_backward(2, hyps, *shape)
    assert np.array_equal(fw["hyp_poses"], bw["hyp_poses"]) and np.array_equal(fw["scores"], bw["scores"])
    h, w = shape
    for f in range(2):
        b = int(fw["best"][f])
        if bw["probs"][f, b] >= G.PROB_THRESH:
            assert np.array_equal(bw["ref_poses"][f, b], fw["refined"][f]), f
            scan = masks[f].T.reshape(-1).astype(bool)   # [w][h] -> scan order x * h + y
            assert np.array_equal(bw["masks"][f, b], scan), f


@pytest.mark.parametrize("shape,hyps", [((12, 16), 16), ((60, 80), 64)])
def test_against_the_restatement(shape, hyps):
    """Probabilities to 1e-9, losses and E to 1e-9 relative, the gradient map to 1e-4 of its norm (relative norm of the difference)."""
    sc, gt, intr, fr = _frames(23, h=shape[0], w=shape[1])
    ids = [9, 2 ** 33]
    g, loss = _backward(sc, gt, intr, hyps, ids)
    dbg = dsacstar.debug_fetch_rgb_backward(2, hyps, *shape)
    for f in range(2):
        ref = G.rgb_backward(sc[f], dbg, f, fr["focal"], fr["ppx"], fr["ppy"], gt[f], THR, ALPHA, MAXR, SUB, WR, WT, CUT)
        assert np.allclose(dbg["probs"][f], ref["probs"], rtol=0, atol=1e-9)
        assert np.allclose(dbg["losses"][f], ref["losses"], rtol=1e-9, atol=1e-12)
        assert abs(loss[f] - ref["E"]) <= 1e-9 * max(1.0, abs(ref["E"]))
        n = np.linalg.norm(ref["grad_map"])
        assert n > 0
        assert np.linalg.norm(g[f] - ref["grad_map"]) <= 1e-4 * n, (f, np.linalg.norm(g[f] - ref["grad_map"]), n)


def test_bitwise_deterministic_additive_and_call_forms_agree():
    sc, gt, intr, fr = _frames(5)
    g1, l1 = _backward(sc, gt, intr, 64, [40, 41])
    g2, l2 = _backward(sc, gt, intr, 64, [40, 41])
    assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32)) and np.array_equal(l1, l2)
    assert np.abs(g1).max() > 0
    base = torch.full((2, 3, 60, 80), 0.25, device="cuda")
    g3, _ = _backward(sc, gt, intr, 64, [40, 41], out=base)
    assert np.array_equal(g3, (np.float32(0.25) + g1).astype(np.float32))
    for dev in ("cuda", "cpu"):
        dsacstar.reset_call_counter(40)
        for f in range(2):
            out = torch.zeros(1, 3, 60, 80, device=dev)
            e = dsacstar.backward_rgb(torch.from_numpy(sc[f:f + 1]).to(dev), out, torch.from_numpy(gt[f]), 64, THR, fr["focal"], fr["ppx"],
                                      fr["ppy"], WR, WT, CUT, ALPHA, MAXR, SUB, SEED)
            assert e == l1[f], (dev, f)
            assert np.array_equal(out[0].cpu().numpy(), g1[f]), (dev, f)


def _pose_error(est, gtc):
    dR = est[:3, :3] @ gtc[:3, :3].T
    return np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))) + 100 * np.linalg.norm(est[:3, 3] - gtc[:3, 3])


def test_descent_through_expected_pose_loss_rgb():
    """25 Adam steps (lr 4 mm) on scene coordinates carrying a 3 degree / 10 cm error of the whole map: the expected loss falls below
    half of its start and the pose register_batch returns moves toward the ground truth (its error at least halves)."""
    sc, gt, intr, _ = _frames(31, shift=False)
    R = G.O.rodrigues(np.radians([2.0, -1.5, 1.2]))
    sc = (np.einsum("ij,njhw->nihw", R, sc) + np.array([0.1, 0.0, -0.05])[None, :, None, None]).astype(np.float32)
    coords = torch.from_numpy(sc).cuda().requires_grad_(True)
    gtt = torch.from_numpy(gt)

    def pose_err():
        p, _, _ = dsacstar.register_batch(coords.detach(), intr, _prm(64), SEED, [0, 1], want_masks=False)
        return sum(_pose_error(p[f].cpu().numpy(), gt[f]) for f in range(2))
    err0 = pose_err()
    opt = torch.optim.Adam([coords], lr=0.004)
    losses = []
    for step in range(25):
        opt.zero_grad()
        loss = dsacstar.expected_pose_loss_rgb(coords, intr, gtt, 64, THR, WR, WT, CUT, ALPHA, MAXR, SUB, seed=SEED,
                                               frame_ids=[1000 * step, 1000 * step + 1]).sum()
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
    assert losses[-1] < losses[0] / 2, losses
    assert pose_err() < err0 / 2, (err0, pose_err())
