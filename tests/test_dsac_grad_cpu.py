"""CPU: the fp64 restatement of DSAC*'s RGB-D backward pass (tests/dsac_grad_restated.py) is the derivative of its own expected loss,
its Kabsch Jacobian agrees with dKabschFD's central differences, dLoss agrees with differences of loss, and without a GPU the
backward binding refuses instead of falling back."""
import numpy as np
import pytest
import torch

from tests import dsac_grad_restated as G
from tests import rgbd_restated as O


def _rot(rng, deg):
    ax = rng.normal(size=3)
    return O.rodrigues(ax / np.linalg.norm(ax) * np.radians(deg))


def _gt(rng):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _rot(rng, rng.uniform(10, 170)), rng.uniform(-2, 2, 3)
    return T


@pytest.mark.parametrize("w_rot,w_trans,cut", [(1.0, 1.0, 100.0), (1.0, 100.0, 5.0), (0.5, 10.0, 1e9)])
def test_dloss_matches_differences_of_loss(w_rot, w_trans, cut):
    """eps 1e-6 central differences of loss in each of the six pose coordinates; relative 1e-5 of the gradient's norm."""
    rng = np.random.default_rng(3)
    for _ in range(10):
        gt = _gt(rng)
        pose = np.concatenate([rng.normal(size=3) * 0.8, rng.uniform(-2, 2, 3)])
        g = G.dloss(pose, gt, w_rot, w_trans, cut)
        fd = np.zeros(6)
        for i in range(6):
            e = np.zeros(6)
            e[i] = 1e-6
            fd[i] = (G.loss(pose + e, gt, w_rot, w_trans, cut) - G.loss(pose - e, gt, w_rot, w_trans, cut)) / 2e-6
        assert np.linalg.norm(g - fd) <= 1e-5 * np.linalg.norm(fd), (g, fd)


@pytest.mark.parametrize("n", [3, 4, 40])
def test_kabsch_jacobian_matches_dkabschfd(n):
    """The analytic 6 x 3n Jacobian against dKabschFD (eps 0.001): the differences' O(eps^2) error bounds the agreement, 1e-4 of the
    largest entry."""
    rng = np.random.default_rng(n)
    for _ in range(5):
        X = rng.uniform(-2, 2, (n, 3))
        R, t = _rot(rng, rng.uniform(0, 170)), rng.uniform(-2, 2, 3)
        E = X @ R.T + t + rng.normal(0, 0.02, (n, 3))
        J = G.kabsch_jacobian(X, E)
        assert J is not None
        fd = G.kabsch_jacobian_fd(X, E)
        assert np.abs(J - fd).max() <= 1e-4 * np.abs(fd).max()


def _frame(seed, nv=40, hyps=8, outliers=0.2):
    rng = np.random.default_rng(seed)
    R, t = _rot(rng, 60), rng.uniform(-1, 1, 3)
    E = np.column_stack([rng.uniform(-1, 1, nv), rng.uniform(-1, 1, nv), rng.uniform(2, 4, nv)])
    S = (E - t) @ R + rng.normal(0, 0.01, (nv, 3))               # R^T (eye - t) with 1 cm noise
    bad = rng.random(nv) < outliers
    S[bad] = rng.uniform(-3, 3, (int(bad.sum()), 3))
    gt = np.eye(4)
    gt[:3, :3], gt[:3, 3] = R.T, -R.T @ t                          # cam->world
    good = np.flatnonzero(~bad)
    triples = [list(rng.choice(good, 3, replace=False)) for h in range(hyps)]
    return S, E, gt, triples


def test_gradient_matches_differences_of_the_expected_loss():
    """The restatement's analytic gradient against eps 1e-6 central differences of its own expected loss along 6 random directions,
    with the triples and the final inlier sets held fixed (so nothing flips under the step). alpha is small so that every hypothesis
    keeps p >= PROB_THRESH (the pass differentiates only those), the triples are drawn from the inliers so that every hypothesis has
    an accepted refinement step (as in the reference, a hypothesis without one gets no hypothesis-path term), and max_dist is large so
    that no error is clamped. Tolerance: 1e-5 of |grad| |v|."""
    H, W, thr, alpha, maxd = 5, 8, 10.0, 4.0, 1e6
    for seed in range(3):
        S, E, gt, triples = _frame(seed)
        base = G.backward_lists(S, E, H * W, H, W, triples, [None] * len(triples), gt, thr, alpha, maxd)
        accs = [O.refine(p, S.astype(np.float32), E.astype(np.float32), thr, 1e6)[1] for p in base["poses"]]
        out = G.backward_lists(S, E, H * W, H, W, triples, accs, gt, thr, alpha, maxd, 1.0, 10.0, 100.0)
        assert (out["probs"] >= G.PROB_THRESH).all()
        assert all(a is not None for a in accs)
        rng = np.random.default_rng(100 + seed)
        for _ in range(6):
            v = rng.normal(size=S.shape)
            f = [G.backward_lists(S + s * 1e-6 * v, E, H * W, H, W, triples, accs, gt, thr, alpha, maxd, 1.0, 10.0, 100.0)["E"]
                 for s in (1, -1)]
            fd = (f[0] - f[1]) / 2e-6
            an = float((out["grad"] * v).sum())
            assert abs(fd - an) <= 1e-5 * np.linalg.norm(out["grad"]) * np.linalg.norm(v), (seed, fd, an)


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_backward_rgbd_refuses_without_a_gpu():
    from acezero_amd import dsacstar
    z = torch.zeros(1, 3, 6, 8)
    with pytest.raises(RuntimeError):
        dsacstar.backward_rgbd(z, z, torch.zeros(1, 3, 6, 8), torch.eye(4), 8, 10.0, 1.0, 1.0, 100.0, 100.0, 100.0, 1)


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_backward_rgb_refuses_without_a_gpu():
    from acezero_amd import dsacstar
    z = torch.zeros(1, 3, 6, 8)
    with pytest.raises(RuntimeError):
        dsacstar.backward_rgb(z, torch.zeros(1, 3, 6, 8), torch.eye(4), 8, 10.0, 525.0, 32.0, 24.0, 1.0, 1.0, 100.0, 100.0, 100.0, 8, 1)
