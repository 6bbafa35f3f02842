"""numpy restatement of the device's pose evaluation (acezero_amd/csrc/align_api.hip), for the CPU tests and tools/eval_timing.py.

Same algorithm as estimate_alignment of the reference (eval_poses_util.py:70-180), vectorised over hypotheses instead of a Python
loop: Kabsch through np.linalg.svd, the translation test for all (hypothesis, frame) pairs, and the rotation angle (orthogonal polar
factor by SVD, Markley's quaternion, 2 atan2(|v|, |w|)) only where the translation test passes.  A non-finite transform or a
rotation block with det <= 0 is "not an inlier" (the device's rule; scipy raises there)."""
import math

import numpy as np


def kabsch_batch(p1, p2, estimate_scale):
    """p1, p2: [B, k, 3] (k points per problem, all valid).  Returns T [B, 4, 4], scale [B]."""
    m1, m2 = p1.mean(axis=1), p2.mean(axis=1)
    c1, c2 = p1 - m1[:, None], p2 - m2[:, None]
    cov = np.matmul(c1.transpose(0, 2, 1), c2) / p1.shape[1]
    U, S, VT = np.linalg.svd(cov)
    V = VT.transpose(0, 2, 1)
    d = np.sign(np.linalg.det(np.matmul(V, U.transpose(0, 2, 1))))
    corr = np.tile(np.eye(3), (len(p1), 1, 1))
    corr[:, 2, 2] = d
    if estimate_scale:
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.mean(np.sum(c2 * c2, axis=2), axis=1) / (S[:, 0] + S[:, 1] + d * S[:, 2])
    else:
        scale = np.ones(len(p1))
    with np.errstate(invalid="ignore"):
        R = scale[:, None, None] * np.matmul(np.matmul(V, corr), U.transpose(0, 2, 1))
    T = np.tile(np.eye(4), (len(p1), 1, 1))
    T[:, :3, :3] = R
    T[:, :3, 3] = m2 - np.einsum("bij,bj->bi", R, m1)
    return T, scale


def rotation_angle(M):
    """[K, 3, 3] -> [K] radians: angle of the orthogonal polar factor (NaN where not finite or det <= 0)."""
    out = np.full(len(M), np.nan)
    ok = np.all(np.isfinite(M), axis=(1, 2))
    ok[ok] = np.linalg.det(M[ok]) > 0
    if not ok.any():
        return out
    U, _, VT = np.linalg.svd(M[ok])
    Q = np.matmul(U, VT)
    tr = Q[:, 0, 0] + Q[:, 1, 1] + Q[:, 2, 2]
    dec = np.stack([Q[:, 0, 0], Q[:, 1, 1], Q[:, 2, 2], tr], 1)
    ch = np.argmax(dec, axis=1)
    q = np.zeros((len(Q), 4))
    for i in range(3):
        s = ch == i
        j, k = (i + 1) % 3, (i + 2) % 3
        q[s, i] = 1 - tr[s] + 2 * Q[s, i, i]
        q[s, j] = Q[s, j, i] + Q[s, i, j]
        q[s, k] = Q[s, k, i] + Q[s, i, k]
        q[s, 3] = Q[s, k, j] - Q[s, j, k]
    s = ch == 3
    q[s, 0] = Q[s, 2, 1] - Q[s, 1, 2]
    q[s, 1] = Q[s, 0, 2] - Q[s, 2, 0]
    q[s, 2] = Q[s, 1, 0] - Q[s, 0, 1]
    q[s, 3] = 1 + tr[s]
    q /= np.linalg.norm(q, axis=1)[:, None]
    out[ok] = 2 * np.arctan2(np.linalg.norm(q[:, :3], axis=1), np.abs(q[:, 3]))
    return out


def inliers_batch(T, gt, est, thr_t, thr_r_deg):
    """T [B, 4, 4] against all frames -> bool [B, N] (get_inliers, eval_poses_util.py:55-67)."""
    finite = np.all(np.isfinite(T), axis=(1, 2))
    Tf = np.where(finite[:, None, None], T, 0.0)
    G = np.einsum("bij,njk->bnik", Tf, gt)
    with np.errstate(invalid="ignore"):
        dt = np.linalg.norm(G[:, :, :3, 3] - est[None, :, :3, 3], axis=2)
    cand = (dt < thr_t) & finite[:, None]
    out = np.zeros(cand.shape, bool)
    b, f = np.nonzero(cand)
    if len(b):
        M = np.matmul(G[b, f, :3, :3], est[f, :3, :3].transpose(0, 2, 1))
        with np.errstate(invalid="ignore"):
            out[b, f] = rotation_angle(M) < thr_r_deg / 180 * math.pi
    return out


def stable_order(scores, candidates):
    """Indices of the candidate hypotheses in sorted(..., key=score, reverse=True) order (ties: ascending index)."""
    idx = np.nonzero(candidates)[0]
    return idx[np.argsort(-np.asarray(scores)[idx], kind="stable")]


def estimate_alignment(gt, est, conf, triples, *, confidence_threshold=500, min_confident=10, thr_t=0.05, thr_r=5,
                       refinement_max_hyp=12, refinement_max_it=8, estimate_scale=False, chunk=500):
    """Returns dict(T (None if failed), scale, scores [H], valid [H])."""
    finite = np.all(np.isfinite(gt), axis=(1, 2))
    keep = finite & (np.asarray(conf) > confidence_threshold)
    g, e = gt[keep], est[keep]
    nc = len(g)
    H = len(triples)
    if nc < min_confident:
        return dict(T=None, scale=1, scores=np.zeros(H, int), valid=np.zeros(H, bool))
    tri = np.asarray(triples, np.int64)
    Ts, scales, masks = np.zeros((H, 4, 4)), np.zeros(H), np.zeros((H, nc), bool)
    for h0 in range(0, H, chunk):
        t = tri[h0:h0 + chunk]
        T, s = kabsch_batch(g[t][:, :, :3, 3], e[t][:, :, :3, 3], estimate_scale)
        Ts[h0:h0 + chunk], scales[h0:h0 + chunk] = T, s
        masks[h0:h0 + chunk] = inliers_batch(T, g, e, thr_t, thr_r)
    scores = masks.sum(1)
    valid = masks[np.arange(H)[:, None], tri].sum(1) >= 3
    order = stable_order(scores, valid)[:refinement_max_hyp]
    if len(order) == 0:
        return dict(T=None, scale=1, scores=scores, valid=valid)
    short = []
    for h in order:
        T, s, m, sc = Ts[h], scales[h], masks[h], scores[h]
        for _ in range(refinement_max_it):
            T2, s2 = kabsch_batch(g[m][None, :, :3, 3], e[m][None, :, :3, 3], estimate_scale)
            m2 = inliers_batch(T2, g, e, thr_t, thr_r)[0]
            if m2.sum() > sc:
                T, s, m, sc = T2[0], s2[0], m2, m2.sum()
            else:
                break
        short.append((sc, T, s))
    best = sorted(short, key=lambda x: x[0], reverse=True)[0]
    return dict(T=best[1], scale=float(best[2]), scores=scores, valid=valid)
