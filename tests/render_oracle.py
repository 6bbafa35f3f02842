"""CPU restatement of the rasteriser (acezero_amd/csrc/render_api.hip, acez_render_frame), operation for operation in float32 /
float64 / int64 so that frames compare bit for bit. Slow and plain: points are vectorised, triangles go one by one."""
import numpy as np

F = np.float32
SUB = 256
GUARD = F(2097152.0)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def camera(cam_to_world, znear, zfar, width, height):
    """(w2c float32 [3,4], focal float32): the rigid inverse [R^T | -R^T t] in double, rounded once; f = (H/2) sqrt(3)."""
    T = np.asarray(cam_to_world, np.float64).reshape(4, 4)
    if not (width >= 1 and height >= 1 and width <= 16384 and height <= 16384):
        raise ValueError("frame size")
    if not (F(znear) > 0 and F(zfar) > F(znear) and np.isfinite(F(zfar))):
        raise ValueError("planes")
    m = np.zeros((3, 4), np.float32)
    for i in range(3):
        for j in range(3):
            m[i, j] = F(T[j, i])
        m[i, 3] = F(-((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3]))
    return m, F(0.5 * float(height) * 1.7320508075688772)


def _to_camera(m, x, y, z):
    return tuple(((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3))


def point_keys(xyz, m, f, znear, zfar, W, H):
    """Per-pixel winning key of the point layer: uint64 [H*W]."""
    keys = np.full(W * H, EMPTY, np.uint64)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    if len(xyz) == 0:
        return keys
    with np.errstate(all="ignore"):
        xc, yc, zc = _to_camera(m, xyz[:, 0], xyz[:, 1], xyz[:, 2])
        d = -zc
        ok = (d >= F(znear)) & (d <= F(zfar))
        cx, cy = F(0.5) * F(W), F(0.5) * F(H)
        u = cx + (f * xc) / d
        v = cy - (f * yc) / d
        ok &= (u > F(-2)) & (u < F(W) + F(2)) & (v > F(-2)) & (v < F(H) + F(2))
    idx = np.flatnonzero(ok)
    x0 = np.floor(u[idx] - F(0.5)).astype(np.int64)
    y0 = np.floor(v[idx] - F(0.5)).astype(np.int64)
    key = (d[idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            s = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            np.minimum.at(keys, y[s] * W + x[s], key[s])
    return keys


def _edge(ax, ay, bx, by, px, py):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def _owns(ax, ay, bx, by):
    return (by - ay) > 0 or ((by - ay) == 0 and (bx - ax) < 0)


def _raster(keys, p, tid, f, zfar, W, H):
    cx, cy = F(0.5) * F(W), F(0.5) * F(H)
    u, v, iz = [], [], []
    for (x, y, d) in p:
        u.append(cx + (f * x) / d)
        v.append(cy - (f * y) / d)
        iz.append(F(1) / d)
        if not (abs(u[-1]) < GUARD and abs(v[-1]) < GUARD):
            return
    X = [int(np.rint(F(a * F(SUB)))) for a in u]
    Y = [int(np.rint(F(a * F(SUB)))) for a in v]
    area = _edge(X[0], Y[0], X[1], Y[1], X[2], Y[2])
    if area == 0:
        return
    if area < 0:
        X[1], X[2] = X[2], X[1]
        Y[1], Y[2] = Y[2], Y[1]
        iz[1], iz[2] = iz[2], iz[1]
        area = -area
    x0 = max(0, (min(X) - SUB // 2 + SUB - 1) >> 8)
    x1 = min(W - 1, (max(X) - SUB // 2) >> 8)
    y0 = max(0, (min(Y) - SUB // 2 + SUB - 1) >> 8)
    y1 = min(H - 1, (max(Y) - SUB // 2) >> 8)
    if x1 < x0 or y1 < y0:
        return
    t0, t1, t2 = _owns(X[1], Y[1], X[2], Y[2]), _owns(X[2], Y[2], X[0], Y[0]), _owns(X[0], Y[0], X[1], Y[1])
    sx = np.arange(x0, x1 + 1, dtype=np.int64)[None, :] * SUB + SUB // 2
    sy = np.arange(y0, y1 + 1, dtype=np.int64)[:, None] * SUB + SUB // 2
    w0 = _edge(X[1], Y[1], X[2], Y[2], sx, sy)
    w1 = _edge(X[2], Y[2], X[0], Y[0], sx, sy)
    w2 = _edge(X[0], Y[0], X[1], Y[1], sx, sy)
    inside = (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
    inside &= ~((w0 == 0) & (not t0)) & ~((w1 == 0) & (not t1)) & ~((w2 == 0) & (not t2))
    with np.errstate(all="ignore"):
        invd = (w0.astype(np.float32) * iz[0] + w1.astype(np.float32) * iz[1] + w2.astype(np.float32) * iz[2]) / F(area)
        d = F(1) / invd
    inside &= d <= F(zfar)
    yy, xx = np.nonzero(inside)
    if len(yy) == 0:
        return
    key = (d[yy, xx].astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(tid)
    np.minimum.at(keys, (yy + y0) * W + (xx + x0), key)


def _clip(a, b, znear):
    t = (znear - a[2]) / (b[2] - a[2])
    return (a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), znear)


def triangle_keys(tri, m, f, znear, zfar, W, H):
    """Per-pixel winning key of the triangle layer: uint64 [H*W]. Near-plane crossings are clipped (Sutherland-Hodgman, fan)."""
    keys = np.full(W * H, EMPTY, np.uint64)
    tri = np.asarray(tri, np.float32).reshape(-1, 3, 3)
    znear = F(znear)
    with np.errstate(all="ignore"):
        for t in range(len(tri)):
            v, ok = [], True
            for k in range(3):
                xc, yc, zc = _to_camera(m, tri[t, k, 0], tri[t, k, 1], tri[t, k, 2])
                if not (np.isfinite(xc) and np.isfinite(yc) and np.isfinite(zc)):
                    ok = False
                    break
                v.append((xc, yc, -zc))
            if not ok:
                continue
            ins = [p[2] >= znear for p in v]
            if not any(ins):
                continue
            if all(ins):
                _raster(keys, v, t, f, zfar, W, H)
                continue
            poly = []
            for k in range(3):
                k1 = (k + 1) % 3
                if ins[k]:
                    poly.append(v[k])
                if ins[k] != ins[k1]:
                    poly.append(_clip(v[k], v[k1], znear) if ins[k] else _clip(v[k1], v[k], znear))
            _raster(keys, poly[:3], t, f, zfar, W, H)
            if len(poly) == 4:
                _raster(keys, [poly[0], poly[2], poly[3]], t, f, zfar, W, H)
    return keys


def blend(bg_rgb, fg_rgba):
    """ace_visualizer._blend_images: float64, then truncation to uint8."""
    mask = fg_rgba[..., 3].astype(float) / 255
    mask = mask[..., None]
    return (fg_rgba[..., :3].astype(float) * mask + bg_rgb.astype(float) * (1 - mask)).astype("uint8")


def render(xyz, rgb, tri, tri_rgba, cam_to_world, znear, zfar, width, height, flipped_portrait=False):
    """The frame acez_render_frame writes: uint8 [height][width][3], or [width][height][3] rotated -90 degrees when flipped."""
    m, f = camera(cam_to_world, znear, zfar, width, height)
    pk = point_keys(xyz, m, f, znear, zfar, width, height)
    tk = triangle_keys(tri, m, f, znear, zfar, width, height)
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    tri_rgba = np.asarray(tri_rgba, np.uint8).reshape(-1, 4)
    bg = np.zeros((width * height, 3), np.uint8)
    hit = pk != EMPTY
    bg[hit] = rgb[(pk[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    fg = np.zeros((width * height, 4), np.uint8)
    hit = tk != EMPTY
    fg[hit] = tri_rgba[(tk[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    out = blend(bg, fg).reshape(height, width, 3)
    return np.ascontiguousarray(np.rot90(out, -1)) if flipped_portrait else out
