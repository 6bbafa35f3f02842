"""Semi-global aggregation of the plane costs (include/acez.h section M) restated in numpy: the definition that the HIP kernels
acez_mvs_volume, acez_mvs_aggregate and acez_mvs_select are compared with bit for bit (tests/test_sgm_gpu.py), checked on its own
without a GPU (tests/test_sgm_cpu.py). Written from the header's text. The costs C and the in-view counts come from
tests/mvs_restated.cost_volume as [D,h,w]; the device's layout [h,w,D] with V in bit 15 is `pack`'s. Integers throughout; the one
float expression (the depth) is section L's, one float32 rounding per operation."""
import numpy as np

from tests import mvs_restated as R

F32 = np.float32
DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))     # (dy, dx), the header's order
BIG = np.int64(1) << 40                                                                  # an absent term


def pack(C, n_in, keep):
    """The device's volume: uint16 [h,w,D], C in bits 0 .. 14 and V = (n_in >= keep) in bit 15."""
    assert C.min() >= 0 and C.max() <= 32767
    return np.ascontiguousarray((C.astype(np.uint16) | ((n_in >= keep).astype(np.uint16) << 15)).transpose(1, 2, 0))


def _step(C_p, L_q, p1, p2):
    """L_r of pixels with a predecessor inside the frame: C_p, L_q int64 [..., D] -> [..., D]."""
    m = L_q.min(-1, keepdims=True)
    down = np.concatenate([np.full_like(L_q[..., :1], BIG), L_q[..., :-1]], -1)           # L_r(q, k - 1); absent at k = 0
    up = np.concatenate([L_q[..., 1:], np.full_like(L_q[..., :1], BIG)], -1)              # L_r(q, k + 1); absent at k = D - 1
    return C_p + np.minimum(np.minimum(L_q, down + p1), np.minimum(up + p1, m + p2)) - m


def path(C, direction, p1, p2):
    """L_r int64 [D,h,w] of direction r = 1 .. 8 over the costs C [D,h,w]. Rows (dy != 0) or columns (dy = 0) are visited in the
    direction of travel; a row's pixels whose predecessor column is outside the frame keep C."""
    dy, dx = DIRECTIONS[direction - 1]
    c = np.asarray(C).astype(np.int64).transpose(1, 2, 0)                                 # [h,w,D]
    h, w, _ = c.shape
    L = c.copy()
    if dy == 0:
        xs = range(1, w) if dx > 0 else range(w - 2, -1, -1)
        for x in xs:
            L[:, x] = _step(c[:, x], L[:, x - dx], p1, p2)
    else:
        ys = range(1, h) if dy > 0 else range(h - 2, -1, -1)
        for y in ys:
            lo, hi = max(0, dx), w + min(0, dx)                                           # the x whose predecessor x - dx is inside
            if hi > lo:
                L[y, lo:hi] = _step(c[y, lo:hi], L[y - dy, lo - dx:hi - dx], p1, p2)
    return L.transpose(2, 0, 1)


def aggregate(C, paths, p1, p2):
    """S int64 [D,h,w]: the sum of L_r over the first `paths` directions."""
    assert paths in (4, 8) and 1 <= p1 <= p2 <= 32767
    return sum(path(C, r, p1, p2) for r in range(1, paths + 1))


def select(X, in_view, z_near, z_far, uniqueness=5):
    """SELECT: (depth float32 [h,w], X(k*) int32, k* int32) from the costs X [D,h,w] and V bool [D,h,w]; section L's rule."""
    X = np.asarray(X).astype(np.int64)
    D = X.shape[0]
    inv_far, step = R.plane_steps(z_near, z_far, D)
    ks = X.argmin(0).astype(np.int32)                                                    # the first minimum
    pick = lambda vol, k: np.take_along_axis(vol, np.clip(k, 0, D - 1)[None].astype(np.int64), 0)[0]
    best = pick(X, ks)
    outside = np.abs(np.arange(D, dtype=np.int32)[:, None, None] - ks[None]) > 1
    C2 = np.where(outside, X, np.iinfo(np.int64).max).min(0)
    unique = ~outside.any(0) | ((C2 > 0) & (100 * best <= (100 - int(uniqueness)) * C2))
    interior = (ks > 0) & (ks < D - 1)
    before, after = pick(X, ks - 1), pick(X, ks + 1)
    den = before - 2 * best + after
    with np.errstate(all="ignore"):
        refine = interior & (den > 0)
        delta = np.where(refine, (before - after).astype(np.float32) / (2 * den).astype(np.float32), F32(0.0)).astype(np.float32)
        depth = F32(1.0) / (inv_far + (ks.astype(np.float32) + delta) * step)
    assert depth.dtype == np.float32
    reject = ~pick(np.asarray(in_view, bool), ks) | ~unique
    if D > 2:
        reject |= (ks == 0) | (ks == D - 1)
    return np.where(reject, F32(0.0), depth), best.astype(np.int32), ks


def sweep(g, rows, ref, sources, z_near, z_far, planes, radius=2, truncation=40, keep=None, uniqueness=5, paths=4, p1=80, p2=640):
    """VOLUME -> AGGREGATE -> SELECT of reference frame `ref`: (depth float32, S(k*) int32, k* int32)."""
    keep = len(sources) if keep is None else int(keep)
    C, n_in = R.cost_volume(g, rows, ref, sources, z_near, z_far, planes, radius, truncation, keep)
    return select(aggregate(C, paths, p1, p2), n_in >= keep, z_near, z_far, uniqueness)


def estimate(images, rows, sources, ranges, planes, radius=2, truncation=40, keep=None, uniqueness=5, tolerance=0.01, min_consistent=2,
             depth_unit=0.001, paths=4, p1=None, p2=None):
    """mvs_restated.estimate with the aggregation between the costs and the choice of the plane, as
    acezero_amd.mvs.estimate_depth_maps(aggregation="sgm") runs it; p1, p2 None: acezero_amd.mvs.sgm_penalties of each frame.
    Returns (uint16 maps, float32 maps)."""
    from acezero_amd.mvs import sgm_penalties
    g = [R.prefilter(im) for im in images]
    live = [bool(sources[i]) and ranges[i] is not None for i in range(len(rows))]
    depths = []
    for i, r in enumerate(rows):
        if not live[i]:
            depths.append(np.zeros((r.h, r.w), np.float32))
            continue
        k = -(-len(sources[i]) // 2) if keep is None else min(int(keep), len(sources[i]))
        q1, q2 = sgm_penalties(k, radius, p1, p2)
        depths.append(sweep(g, rows, i, sources[i], ranges[i][0], ranges[i][1], planes, radius, truncation, k, uniqueness, paths, q1, q2)[0])
    out = [R.check(depths, rows, i, sources[i], tolerance, min_consistent, depth_unit) if live[i] else np.zeros((r.h, r.w), np.uint16)
           for i, r in enumerate(rows)]
    return out, depths
