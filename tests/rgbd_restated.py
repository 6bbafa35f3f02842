"""fp64 numpy restatement of DSAC*'s RGB-D estimator as acezero_amd/csrc/ransac_rgbd.hip states it (the reference's commented-out
dsacstar_rgbd_forward: sampleHypothesesRGBD, get3DDistErrs, getHypScores, refineHypRGBD), for the GPU parity tests and
tools/rgbd_timing.py. Kabsch runs on numpy's SVD here, not on the device's Jacobi SVD."""
import numpy as np

M64 = (1 << 64) - 1


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def try_key(seed, frame, hyp, tr):
    return mix64(mix64(mix64(seed) ^ frame) ^ ((hyp << 32) | tr))


def irand(key, draw, n):
    r = mix64((key + draw * 0xD1B54A32D192ED03) & M64)
    return ((r >> 32) * n) >> 32


def rodrigues(rv):
    rv = np.asarray(rv, np.float64)
    th = np.linalg.norm(rv)
    if th < 2.220446049250313e-16:
        return np.eye(3)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * K


def rodrigues_inv(R):
    r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.sqrt((r @ r) * 0.25)
    c = np.clip((np.trace(R) - 1) * 0.5, -1, 1)
    th = np.arccos(c)
    if s < 1e-5:
        if c > 0:
            return np.zeros(3)
        v = np.sqrt(np.maximum((np.diag(R) + 1) * 0.5, 0))
        v[1] *= -1 if R[0, 1] < 0 else 1
        v[2] *= -1 if R[0, 2] < 0 else 1
        if abs(v[0]) < abs(v[1]) and abs(v[0]) < abs(v[2]) and (R[1, 2] > 0) != (v[1] * v[2] > 0):
            v[2] = -v[2]
        return v * th / np.linalg.norm(v)
    return r / (2 * s) * th


def kabsch(X, E):
    """(rvec, tvec) with E ~ R X + t, or None if the centred covariance has rank < 2. X, E: [k,3]."""
    X, E = np.asarray(X, np.float64), np.asarray(E, np.float64)
    mX, mE = X.mean(0), E.mean(0)
    C = (X - mX).T @ (E - mE)
    U, S, Vt = np.linalg.svd(C)
    if not (S[0] > 0) or not (S[1] >= 1e-12 * S[0]):
        return None
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1, 1, d]) @ U.T
    return rodrigues_inv(R), mE - R @ mX


def valid_cells(cc):
    """Map indices y*W+x of the valid cells of camera coordinates [3,H,W], in the reference's x-outer / y-inner scan order."""
    H, W = cc.shape[1:]
    ok = (cc[2] != 0) & np.isfinite(cc).all(0)
    y, x = np.nonzero(ok)
    order = np.lexsort((y, x))
    return (y[order] * W + x[order]).astype(np.int64)


def dist_errs(pose6, S, E, max_dist):
    """get3DDistErrs on lists S, E [k,3] float32: (float) |E - (float)(R S + t)| * 100, clamped."""
    R, t = rodrigues(pose6[:3]), np.asarray(pose6[3:], np.float64)
    P = (S.astype(np.float64) @ R.T + t).astype(np.float32)
    d = (E.astype(np.float32) - P).astype(np.float64)
    l = np.sqrt((d * d).sum(1)).astype(np.float32) * np.float32(100)
    return np.where(l < np.float32(max_dist), l, np.float32(max_dist)).astype(np.float32)


def score(errs, n_cells, thr, alpha, max_dist, H, W):
    beta = np.float32(5) / np.float32(thr)

    def term(e):
        be = beta * (np.asarray(e, np.float32) - np.float32(thr))
        return np.where(be > 40, 0.0, 1 - 1 / (1 + np.exp(-be.astype(np.float64))))
    s = term(errs).sum() + (n_cells - len(errs)) * float(term(np.float32(max_dist)))
    return s * float(np.float32(alpha) / np.float32(W) / np.float32(H))


def refine(pose6, S, E, thr, max_dist, max_steps=100):
    """refineHypRGBD: (pose6, inlier flags over the list of the last accepted step or None, count)."""
    pose = np.asarray(pose6, np.float64).copy()
    flags = dist_errs(pose, S, E, max_dist) < np.float32(thr)
    best, acc = 3, None
    for _ in range(max_steps):
        cnt = int(flags.sum())
        if cnt <= best:
            break
        k = kabsch(S[flags], E[flags])
        if k is None:
            break
        best, acc = cnt, flags
        pose = np.concatenate(k)
        flags = dist_errs(pose, S, E, max_dist) < np.float32(thr)
    return pose, acc, (best if acc is not None else 0)


def pose2trans(pose6):
    T = np.eye(4)
    T[:3, :3] = rodrigues(pose6[:3])
    T[:3, 3] = pose6[3:]
    return np.linalg.inv(T)


def sample(sc, cc, hyps, max_tries, thr, seed, frame_id):
    """sampleHypothesesRGBD on the counter-based stream: per hypothesis (map indices of the kept triple, pose6 or None if rank < 2,
    accepted)."""
    cells = valid_cells(cc)
    S, E = sc.reshape(3, -1).T[cells], cc.reshape(3, -1).T[cells]
    out = []
    for h in range(hyps):
        for t in range(max_tries):
            key = try_key(seed, frame_id, h, t)
            j = [irand(key, d, len(cells)) for d in range(3)]
            k = kabsch(S[j], E[j])
            ok = k is not None and bool((dist_errs(np.concatenate(k), S[j], E[j], np.inf).astype(np.float64) < thr).all())
            if ok or t == max_tries - 1:
                out.append((cells[j], None if k is None else np.concatenate(k), ok))
                break
    return out
