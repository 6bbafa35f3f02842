"""fp64 numpy restatement of DSAC*'s RGB-D backward pass as acezero_amd/csrc/ransac_grad.hip states it (the reference's commented-out
dsacstar_rgbd_backward with dsacstar_loss.h's loss / dLoss and dsacstar_derivative.h's dSMScoreRGBD), for the CPU gradient checks
and the GPU parity tests. Sampling and refinement are tests/rgbd_restated.py's; everything after them is recomputed here on numpy's
SVD with the closed-form right Jacobian of the rotation vector, independently of the kernel's formulation:

    p = softmax(scores), E = sum_h p_h loss_h (refined poses for p_h >= PROB_THRESH, sampled poses otherwise)
    dE/dX = sum_{h: p_h >= PROB_THRESH} p_h dloss_h/dpose dpose_h/dX            (path I, Kabsch of the final inlier set)
                                      + p_h (loss_h - E) dscore_h/dX           (path II, own errors + the sampled triple)

Scores are the fp64 soft inlier counts (the kernel rounds each distance to float first; the difference is far below the tolerances
the tests use). Lists are the valid cells in scan order; gradients come back per list entry [nv,3]."""
import numpy as np

from tests import rgbd_restated as O

PROB_THRESH = 0.001
MAXLOSS = 10000000.0


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def right_jacobian(r):
    """Jr with rodrigues(r + dr) ~ rodrigues(r) [Jr dr]x."""
    th = np.linalg.norm(r)
    if th < 1e-8:
        return np.eye(3) - 0.5 * skew(r)
    K = skew(r)
    return np.eye(3) - (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K


def loss(pose6, gt, w_rot=1.0, w_trans=1.0, cut=100.0):
    """dsacstar::loss(pose2trans(pose6), gt): gt is the 4x4 cam->world ground truth."""
    R = O.rodrigues(pose6[:3])
    Rg = np.asarray(gt, np.float64)[:3, :3].T
    tr = np.clip(np.trace(R @ Rg.T), -1, 3)
    rot = 180 * np.arccos((tr - 1) / 2) / np.pi
    c = -R.T @ np.asarray(pose6[3:], np.float64)
    l = w_rot * rot + w_trans * np.linalg.norm(c - np.asarray(gt, np.float64)[:3, 3])
    if l > cut:
        l = np.sqrt(cut * l)
    return min(l, MAXLOSS)


def dloss(pose6, gt, w_rot=1.0, w_trans=1.0, cut=100.0):
    """d loss / d (rvec, tvec): rotation in the body frame (loss(R [w]x)), mapped to the rotation vector by Jr^T."""
    r, t = np.asarray(pose6[:3], np.float64), np.asarray(pose6[3:], np.float64)
    R = O.rodrigues(r)
    G = np.asarray(gt, np.float64)
    Rg = G[:3, :3].T
    tr = np.trace(R @ Rg.T)
    rot = 180 * np.arccos(np.clip((tr - 1) / 2, -1, 1)) / np.pi
    u = -R.T @ t - G[:3, 3]
    te = np.linalg.norm(u)
    l = w_rot * rot + w_trans * te
    L = np.sqrt(cut * l) if l > cut else l
    if L >= MAXLOSS or rot + te <= 0:
        return np.zeros(6)
    # d tr / dw = vee-gradient of trace(R [w]x Rg^T) = sum over the skew part of Rg^T R
    Mx = Rg.T @ R
    dtr_dw = np.array([Mx[1, 2] - Mx[2, 1], Mx[2, 0] - Mx[0, 2], Mx[0, 1] - Mx[1, 0]])
    drot = w_rot * (-180 / np.pi) / np.sqrt(3 - tr * tr + 2 * tr) if -1 < tr < 3 else 0.0
    un = u / te if te > 0 else np.zeros(3)
    # c = -R^T t; with R -> R [w]x: dc = -[w]x^T R^T t = [w]x R^T t = w x (R^T t) -> dte/dw = (R^T t) x un
    dte_dw = np.cross(R.T @ t, un)
    gw = drot * dtr_dw + w_trans * dte_dw
    g = np.concatenate([right_jacobian(r).T @ gw, -w_trans * (R @ un)])
    return g * (0.5 * np.sqrt(cut / l) if l > cut else 1.0)


def _proper_svd(C):
    U, S, Vt = np.linalg.svd(C)
    V = Vt.T.copy()
    S = S.copy()
    if np.linalg.det(U) < 0:
        U[:, 2] *= -1
        S[2] *= -1
    if np.linalg.det(V) < 0:
        V[:, 2] *= -1
        S[2] *= -1
    return U, S, V


def kabsch_jacobian(X, E):
    """6 x 3n Jacobian of O.kabsch(X, E) with respect to X (row-major per point), or None if it is degenerate (s1 + s2 <= 1e-6 s0)."""
    X, E = np.asarray(X, np.float64), np.asarray(E, np.float64)
    n = len(X)
    k = O.kabsch(X, E)
    mX, mE = X.mean(0), E.mean(0)
    C = (X - mX).T @ (E - mE)
    U, S, V = _proper_svd(C)
    if k is None or not (S[1] + S[2] > 1e-6 * S[0]):
        return None
    R = V @ U.T
    Jri = np.linalg.inv(right_jacobian(k[0]))
    out = np.zeros((6, 3 * n))
    for i in range(n):
        ec = E[i] - mE
        for c in range(3):
            dC = np.zeros((3, 3))
            dC[c] = ec
            G = V.T @ dC.T @ U                     # U_M^T dM V_M with M = C^T = V S U^T
            Om = np.zeros((3, 3))
            for a in range(3):
                for b in range(3):
                    if a != b:
                        Om[a, b] = (G[a, b] - G[b, a]) / (S[a] + S[b])
            dR = V @ Om @ U.T
            w = R.T @ dR
            w = np.array([w[2, 1], w[0, 2], w[1, 0]])
            ex = np.zeros(3)
            ex[c] = 1.0 / n
            out[:3, 3 * i + c] = Jri @ w
            out[3:, 3 * i + c] = -dR @ mX - R @ ex
    return out


def kabsch_jacobian_fd(X, E, eps=0.001):
    """dKabschFD: central differences of O.kabsch (eps 0.001); a column that fails or is not finite stays zero."""
    X = np.asarray(X, np.float64).copy()
    out = np.zeros((6, 3 * len(X)))
    for i in range(len(X)):
        for c in range(3):
            X[i, c] += eps
            f = O.kabsch(X, E)
            X[i, c] -= 2 * eps
            b = O.kabsch(X, E)
            X[i, c] += eps
            if f is None or b is None:
                continue
            col = (np.concatenate(f) - np.concatenate(b)) / (2 * eps)
            if np.isfinite(col).all():
                out[:, 3 * i + c] = col
    return out


def kabsch_vjp(X, E, g6):
    J = kabsch_jacobian(X, E)
    if J is None:
        J = kabsch_jacobian_fd(X, E)
    return (g6 @ J).reshape(-1, 3)


def _errs(pose6, S, E):
    R, t = O.rodrigues(pose6[:3]), np.asarray(pose6[3:], np.float64)
    d = E.astype(np.float64) - (S.astype(np.float64) @ R.T + t)
    return d, np.sqrt((d * d).sum(1))


def score(pose6, S, E, n_cells, H, W, thr, alpha, max_dist):
    """fp64 soft inlier count (invalid cells carry max_dist)."""
    _, err = _errs(pose6, S, E)
    e = np.minimum(err * 100, max_dist)
    beta = 5.0 / thr

    def term(v):
        return 1 - 1 / (1 + np.exp(-beta * (v - thr)))
    return (term(e).sum() + (n_cells - len(S)) * term(max_dist)) * float(np.float32(alpha) / np.float32(W) / np.float32(H))


def score_grad(pose6, S, E, H, W, thr, alpha, max_dist):
    """(d score / d X [nv,3] with the pose fixed, d score / d pose6)."""
    r = np.asarray(pose6[:3], np.float64)
    R = O.rodrigues(r)
    d, err = _errs(pose6, S, E)
    beta = 5.0 / thr
    ok = (err * 100 <= max_dist) & (err > 0)
    s = 1 / (1 + np.exp(-beta * (err * 100 - thr)))
    dD = np.where(ok, -s * (1 - s) * beta, 0.0) * float(np.float32(alpha) / np.float32(W) / np.float32(H))
    gp = (dD / np.where(ok, err, 1.0))[:, None] * (-100.0 * d)   # d score / d (R X + t)
    gX = gp @ R
    RtG = gp @ R                                                  # R^T gp per row
    gw = np.cross(S.astype(np.float64), RtG).sum(0)
    return gX, np.concatenate([right_jacobian(r).T @ gw, gp.sum(0)])


def softmax(scores):
    e = np.exp(np.asarray(scores) - np.max(scores))
    return e / e.sum()


def backward_lists(S, E, n_cells, H, W, triples, accs, gt, thr, alpha, max_dist, w_rot=1.0, w_trans=1.0, cut=100.0):
    """The backward pass on the valid lists S, E [nv,3] with FIXED triples (list indices [hyps][3], or None for a zero pose) and
    final inlier sets (bool [nv] or None; refinement is not re-run). -> dict(E, probs, losses, poses, refined, grad [nv,3])."""
    S, E = np.asarray(S, np.float64), np.asarray(E, np.float64)
    hyps = len(triples)
    poses = []
    for tri in triples:
        k = None if tri is None else O.kabsch(S[list(tri)], E[list(tri)])
        poses.append(np.zeros(6) if k is None else np.concatenate(k))
    scores = np.array([score(p, S, E, n_cells, H, W, thr, alpha, max_dist) for p in poses])
    probs = softmax(scores)
    refined = []
    for h in range(hyps):
        a = accs[h]
        if probs[h] >= PROB_THRESH and a is not None:
            refined.append(np.concatenate(O.kabsch(S[a], E[a])))
        else:
            refined.append(poses[h])
    losses = np.array([loss(refined[h], gt, w_rot, w_trans, cut) for h in range(hyps)])
    Eexp = float(probs @ losses)
    grad = np.zeros_like(S)
    for h in range(hyps):
        if probs[h] < PROB_THRESH:
            continue
        a = accs[h]
        if a is not None:      # path I
            idx = np.flatnonzero(a)
            grad[idx] += kabsch_vjp(S[idx], E[idx], probs[h] * dloss(refined[h], gt, w_rot, w_trans, cut))
        sg = probs[h] * (losses[h] - Eexp)   # path II
        gX, g6 = score_grad(poses[h], S, E, H, W, thr, alpha, max_dist)
        grad += sg * gX
        tri = triples[h]
        if tri is None or O.kabsch(S[list(tri)], E[list(tri)]) is None:
            continue
        J = kabsch_jacobian(S[list(tri)], E[list(tri)])
        if J is None:
            J = kabsch_jacobian_fd(S[list(tri)], E[list(tri)])
        if np.abs(J).max() > 10:
            continue
        grad[list(tri)] += (sg * g6 @ J).reshape(3, 3)
    return dict(E=Eexp, probs=probs, losses=losses, poses=poses, refined=refined, grad=grad)


def backward(sc, cc, gt, hyps, thr, alpha, max_dist, seed, frame_id, w_rot=1.0, w_trans=1.0, cut=100.0, max_tries=16):
    """The whole pass on one frame (sc, cc [3,H,W]): rgbd_restated's sampling, the probabilities, rgbd_restated's refinement of every
    hypothesis with p >= PROB_THRESH, then backward_lists. The gradient comes back as a [3,H,W] map; 'accs' holds the inlier sets."""
    H, W = cc.shape[1:]
    cells = O.valid_cells(cc)
    S, E = sc.reshape(3, -1).T[cells].astype(np.float64), cc.reshape(3, -1).T[cells].astype(np.float64)
    S32, E32 = sc.reshape(3, -1).T[cells], cc.reshape(3, -1).T[cells]
    where = {int(m): i for i, m in enumerate(cells)}
    smp = O.sample(sc, cc, hyps, max_tries, thr, seed, frame_id)
    triples = [None if pose is None else [where[int(m)] for m in trip] for trip, pose, _ in smp]
    poses = [np.zeros(6) if pose is None else pose for _, pose, _ in smp]
    probs = softmax([score(p, S, E, H * W, H, W, thr, alpha, max_dist) for p in poses])
    accs = [O.refine(poses[h], S32, E32, thr, max_dist)[1] if probs[h] >= PROB_THRESH else None for h in range(hyps)]
    out = backward_lists(S, E, H * W, H, W, triples, accs, gt, thr, alpha, max_dist, w_rot, w_trans, cut)
    g = np.zeros((3, H * W))
    g[:, cells] = out["grad"].T
    out.update(grad_map=g.reshape(3, H, W), accs=accs, cells=cells, triples=triples)
    return out


# ---------------------------------------------------------------------------------------------------- RGB (backward_rgb)
def rgb_backward(sc, dbg, f, focal, ppx, ppy, gt, thr, alpha, max_reproj, sub, w_rot=1.0, w_trans=1.0, cut=100.0):
    """The RGB pass (dsacstar_rgb_backward) on frame f of sc [3,H,W], from the sampled hypotheses, their minimal sets, scores, refined
    poses and final inlier masks that the kernel's debug fetch returns (tests/test_dsac_gpu.py pins sampling, scoring and refinement
    against the CPU oracle). Recomputed here: probabilities, losses, E, path I (-(J^T J)^+ J^T dN/dObj with numpy's pseudo-inverse and
    the oracle's projection Jacobian, zeroed above 10) and path II (every pixel's error, and central differences of the oracle's P3P
    in the first three points of the minimal set). -> dict(E, probs, losses, grad_map [3,H,W])."""
    from oracle import dsac_oracle as DO
    H, W = sc.shape[1:]
    half = sub // 2
    # scan order p = x * H + y
    xs, ys = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    xs, ys = xs.ravel(), ys.ravel()
    X = np.stack([sc[c][ys, xs] for c in range(3)], 1).astype(np.float32)
    img = np.stack([xs * sub + half, ys * sub + half], 1).astype(np.float32).astype(np.float64)
    hyps = dbg["scores"].shape[1]
    probs = softmax(dbg["scores"][f])
    refined = dbg["ref_poses"][f]
    losses = np.array([loss(refined[h], gt, w_rot, w_trans, cut) for h in range(hyps)])
    E = float(probs @ losses)
    grad = np.zeros((H * W, 3))
    beta = np.float32(5) / np.float32(thr)
    scale = float(np.float32(alpha) / np.float32(W) / np.float32(H))

    def rows_and_dobj(pose, idx):
        uv, J = DO.project(pose, focal, ppx, ppy, X[idx], jac=True)
        d = uv - img[idx]
        err = np.maximum(np.sqrt((d * d).sum(1)), 1e-8)
        ok = err <= max_reproj
        rows = np.einsum("nk,nkq->nq", d / err[:, None], J) * ok[:, None]
        R, t = O.rodrigues(pose[:3]), pose[3:]
        c = X[idx].astype(np.float64) @ R.T + t
        z = c[:, 2:3]
        px = np.stack([focal * c[:, 0] / c[:, 2] + ppx, focal * c[:, 1] / c[:, 2] + ppy], 1)
        e2 = px - img[idx]
        err2 = np.sqrt((e2 * e2).sum(1))
        dpx = focal * (R[0][None, :] / z - c[:, 0:1] / z ** 2 * R[2][None, :])
        dpy = focal * (R[1][None, :] / z - c[:, 1:2] / z ** 2 * R[2][None, :])
        g = (e2[:, 0:1] * dpx + e2[:, 1:2] * dpy) / (err2[:, None] + 1e-8)
        g *= ((err2 <= max_reproj) & (np.abs(c[:, 2]) >= 1e-8))[:, None]
        return rows, g, ok

    for h in range(hyps):
        p = probs[h]
        if p < PROB_THRESH:
            continue
        m = dbg["masks"][f, h]
        idx = np.flatnonzero(m)
        if len(idx):          # path I
            rows, g, _ = rows_and_dobj(refined[h], idx)
            JR = -np.linalg.pinv(rows.T @ rows) @ rows.T      # 6 x n
            if np.abs(JR).max() <= 10:
                a = p * dloss(refined[h], gt, w_rot, w_trans, cut) @ JR
                grad[idx] += a[:, None] * g
        sg = p * (losses[h] - E)   # path II
        pose = dbg["hyp_poses"][f, h]
        uv = DO.project(pose, focal, ppx, ppy, X)
        pf = uv.astype(np.float32)
        dd = (img.astype(np.float32) - pf).astype(np.float64)
        e = np.sqrt((dd * dd).sum(1)).astype(np.float32)
        e = np.where(e < np.float32(max_reproj), e, np.float32(max_reproj))
        be = beta * (e - np.float32(thr))
        st = 1 / (1 + np.exp(-be.astype(np.float64)))
        dD = np.where(be > 40, 0.0, -st * (1 - st) * float(beta) * sg * scale)
        allidx = np.arange(H * W)
        rows, g, ok = rows_and_dobj(pose, allidx)
        dD = dD * ok
        grad += dD[:, None] * g
        s6 = dD @ rows
        smp = dbg["samples"][f, h]
        obj = X[smp].copy()
        im = img[smp].astype(np.float32)
        cols = np.zeros((9, 6))
        good = True
        for i in range(3):
            for c in range(3):
                o = obj.copy()
                o[i, c] = np.float32(obj[i, c] + np.float32(0.001))
                okf, fw = DO.p3p(o, im, focal, ppx, ppy)
                o[i, c] = np.float32(o[i, c] - np.float32(2) * np.float32(0.001))
                okb, bw = DO.p3p(o, im, focal, ppx, ppy)
                if not (okf and okb):
                    good = False
                    break
                cols[3 * i + c] = (fw - bw) / float(np.float32(2) * np.float32(0.001))
            if not good:
                break
        if good and np.isfinite(cols).all() and np.abs(cols).max() <= 10:
            grad[smp[:3]] += (cols @ s6).reshape(3, 3)
    gm = np.zeros((3, H, W))
    gm[:, ys, xs] = grad.T
    return dict(E=E, probs=probs, losses=losses, grad_map=gm)
