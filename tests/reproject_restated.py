"""The reprojection score of include/acez.h section J restated in numpy: the definition the HIP passes of
acezero_amd/csrc/reproject_api.hip are compared with bit for bit (tests/test_benchmark_gpu.py), checked on its own without a GPU
(tests/test_benchmark_cpu.py). Every float operation is a numpy float32 operation in the kernel's order (one rounding each, no
fused multiply-add); everything after the projection is integer arithmetic."""
import numpy as np

ZMIN = np.float32(0.1)
F32 = np.float32


def cell_means(frames_nhw3):
    """uint8 [n,H,W,3] -> uint8 [n,ceil(H/8),ceil(W/8),3]: per channel (sum + count // 2) // count over the pixels a cell has."""
    fr = np.asarray(frames_nhw3, np.uint8)
    n, H, W, _ = fr.shape
    oh, ow = (H + 7) // 8, (W + 7) // 8
    out = np.zeros((n, oh, ow, 3), np.uint8)
    for cy in range(oh):
        for cx in range(ow):
            blk = fr[:, cy * 8:min(cy * 8 + 8, H), cx * 8:min(cx * 8 + 8, W)].astype(np.int64)
            cnt = blk.shape[1] * blk.shape[2]
            out[:, cy, cx] = (blk.sum(axis=(1, 2)) + cnt // 2) // cnt
    return out


def make_views(w2c, focal_px, ppx_px, ppy_px, sub=8):
    """[T,15] float32 view records: 3 x 4 world -> camera rows, then focal, cx, cy in cell units (pixels / sub; divided in float64,
    rounded to float32 once)."""
    w2c = np.asarray(w2c, np.float64)
    w2c = w2c.reshape(-1, w2c.shape[-2], 4)[:, :3]                      # [T,3,4] or [T,4,4]
    T = w2c.shape[0]
    out = np.zeros((T, 15), np.float32)
    out[:, :12] = w2c.reshape(T, 12).astype(np.float32)
    out[:, 12] = (np.broadcast_to(np.asarray(focal_px, np.float64), (T,)) / sub).astype(np.float32)
    out[:, 13] = (np.broadcast_to(np.asarray(ppx_px, np.float64), (T,)) / sub).astype(np.float32)
    out[:, 14] = (np.broadcast_to(np.asarray(ppy_px, np.float64), (T,)) / sub).astype(np.float32)
    return out


def project(points, view, oh, ow):
    """(valid [M] bool, cell [M] int64 (0 where not valid), depth [M] float32) of float32 points [M,3] in one view record [15]."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    m = np.asarray(view, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        xc = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]
        yc = ((m[4] * x + m[5] * y) + m[6] * z) + m[7]
        zc = ((m[8] * x + m[9] * y) + m[10] * z) + m[11]
        front = zc >= ZMIN
        iz = F32(1.0) / zc
        u = m[13] + (m[12] * xc) * iz
        v = m[14] + (m[12] * yc) * iz
        valid = front & (u >= F32(0.0)) & (u < F32(ow)) & (v >= F32(0.0)) & (v < F32(oh))
        cu = np.where(valid, np.floor(u), 0).astype(np.int64)
        cv = np.where(valid, np.floor(v), 0).astype(np.int64)
    assert xc.dtype == np.float32 and u.dtype == np.float32
    return valid, cv * ow + cu, zc


def score_views(points, colours, views, targets, depth_band):
    """The four passes. points float32 [M,3], colours uint8 [M,3], views float32 [T,15], targets uint8 [T,oh,ow,3].
    Returns (sse int64 [T], covered int64 [T], image uint8 [T,oh,ow,3], mask uint8 [T,oh,ow])."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    clr = np.asarray(colours, np.uint8).reshape(-1, 3).astype(np.int64)
    views = np.asarray(views, np.float32).reshape(-1, 15)
    tg = np.asarray(targets, np.uint8)
    T, oh, ow, _ = tg.shape
    hw = oh * ow
    one_plus_band = F32(np.float64(1.0) + np.float64(F32(depth_band)))
    sse, covered = np.zeros(T, np.int64), np.zeros(T, np.int64)
    image, mask = np.zeros((T, oh, ow, 3), np.uint8), np.zeros((T, oh, ow), np.uint8)
    idx = np.arange(len(pts), dtype=np.uint64)
    for t in range(T):
        valid, cell, zc = project(pts, views[t], oh, ow)
        at = np.flatnonzero(valid)
        keys = np.full(hw, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)                        # clear
        key = (zc[at].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[at]
        np.minimum.at(keys, cell[at], key)                                                   # nearest
        zmin = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
        with np.errstate(all="ignore"):
            lim = zmin * one_plus_band                                                       # one float32 product
        take = at[zc[at] <= lim[cell[at]]]
        sums = np.zeros((hw, 4), np.int64)                                                   # accumulate
        np.add.at(sums[:, 0], cell[take], clr[take, 0])
        np.add.at(sums[:, 1], cell[take], clr[take, 1])
        np.add.at(sums[:, 2], cell[take], clr[take, 2])
        np.add.at(sums[:, 3], cell[take], 1)
        assert sums.max(initial=0) < 2 ** 32                                                 # the device's sums are 32 bits wide
        cnt = sums[:, 3]
        cov = cnt > 0                                                                        # score
        col = np.zeros((hw, 3), np.int64)
        col[cov] = (sums[cov, :3] + (cnt[cov] // 2)[:, None]) // cnt[cov][:, None]
        diff = col[cov] - tg[t].reshape(hw, 3).astype(np.int64)[cov]
        sse[t] = int((diff * diff).sum())
        covered[t] = int(cov.sum())
        image[t] = col.reshape(oh, ow, 3).astype(np.uint8)
        mask[t] = cov.reshape(oh, ow).astype(np.uint8)
    return sse, covered, image, mask


def psnr(sse, covered):
    """Per view 10 log10(255^2 * 3 * covered / sse) in float64: inf for sse 0, None for a view without a covered cell."""
    out = []
    for s, c in zip(np.asarray(sse).tolist(), np.asarray(covered).tolist()):
        if c == 0:
            out.append(None)
        elif s == 0:
            out.append(float("inf"))
        else:
            out.append(float(10.0 * np.log10(np.float64(255.0 ** 2 * 3.0 * c) / np.float64(s))))
    return out
