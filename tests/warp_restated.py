"""numpy restatement of the three view-warp kernels of acezero_amd/csrc/buffer_api.hip (warp_mean_kernel, warp_views_kernel,
warp_mask_kernel) -- TEST INFRASTRUCTURE ONLY. Written from the formulas in that file's header and in session.warp_views, without torch:
affine_grid's align_corners=False base grid, the affine map, grid_sample's unnormalisation, reflection about -0.5 / size - 0.5, the
clip, four bilinear taps with bounds checks, torchvision's ColorJitter brightness / contrast on the de-normalised grey value.

Every function takes `dt`: np.float64 is the reference the GPU tests compare with (tests/test_warp_restated_cpu.py pins it against
torch's float64 affine_grid / grid_sample to 1e-12); np.float32 evaluates the same expressions in the kernels' operation order and
number format, which is how the tests' error bounds are measured (tests/warp_cases.py)."""
import numpy as np

from tests.ordered_sums import wave_sums

EPS32 = float(np.finfo(np.float32).eps)


def source_coords(theta, H, W, hs, ws, dt=np.float64, ys=None, xs=None):
    """theta [B,6] (row-major 2 x 3). The unreflected source coordinate (ix, iy), each [B,hs,ws], of every output pixel -- or of the
    pixels (ys [h'], xs [w']) only."""
    th = np.asarray(theta).astype(dt).reshape(-1, 6, 1, 1)
    x = (np.arange(ws) if xs is None else np.asarray(xs)).astype(dt)[None, None, :]
    y = (np.arange(hs) if ys is None else np.asarray(ys)).astype(dt)[None, :, None]
    one, two, half = dt(1), dt(2), dt(0.5)
    xn = (two * x + one) / dt(ws) - one
    yn = (two * y + one) / dt(hs) - one
    gx = xn * th[:, 0] + yn * th[:, 1] + th[:, 2]
    gy = xn * th[:, 3] + yn * th[:, 4] + th[:, 5]
    return ((gx + one) * dt(W) - one) * half, ((gy + one) * dt(H) - one) * half


def reflect_flips(x, size):
    """How many times reflect_clip folds x back: floor(|x + 0.5| / size)."""
    return np.floor(np.abs(np.asarray(x, np.float64) + 0.5) / size).astype(np.int64)


def reflect_clip(x, size, dt=np.float64):
    """Reflection about -0.5 and size - 0.5, any number of flips, then the clip to [0, size - 1]."""
    x = np.asarray(x).astype(dt)
    mn, span = dt(-0.5), dt(size)
    a = np.abs(x - mn)
    extra = np.fmod(a, span)
    flips = np.floor(a / span).astype(np.int64)
    r = np.where(flips & 1, span - extra + mn, extra + mn).astype(dt)
    return np.minimum(dt(size - 1), np.maximum(r, dt(0)))


def jitter(values, br, ct, mean, dt=np.float64):
    """ColorJitter on the de-normalised grey value (warp_jitter); br, ct, mean broadcast against values."""
    v = np.asarray(values).astype(dt)
    br, ct, m = (np.asarray(a).astype(dt) for a in (br, ct, mean))
    g = np.minimum(np.maximum((v * dt(0.25) + dt(0.4)) * br, dt(0)), dt(1))
    g = np.minimum(np.maximum((g - m) * ct + m, dt(0)), dt(1))
    return (g - dt(0.4)) / dt(0.25)


def jitter_mean(image, br, dt=np.float64):
    """Mean over the frame of clamp((v * 0.25 + 0.4) * br, 0, 1) (warp_mean_kernel). In float64 a plain mean; in float32 the kernel's
    summation order: 1024 strided partial sums, a 64-lane butterfly per wave, the 16 wave sums one after the other."""
    g = np.asarray(image).astype(dt).reshape(-1)
    g = np.minimum(np.maximum((g * dt(0.25) + dt(0.4)) * dt(br), dt(0)), dt(1))
    if dt is np.float64:
        return float(g.sum() / g.size)
    hw = g.size
    rows = np.zeros(((hw + 1023) // 1024) * 1024, dt)
    rows[:hw] = g
    acc = np.zeros(1024, dt)
    for r in rows.reshape(-1, 1024):
        acc = acc + r
    acc = wave_sums(acc.reshape(16, 64, 1))
    s = dt(0)
    for i in range(16):
        s = s + acc[i, 0]
    return dt(s / dt(hw))


def warp(images, index, theta, jit, means, hs, ws, dt=np.float64, tau=None):
    """images [n,H,W], index [B], theta [B,6], jit [B,2] = (brightness, contrast) or None, means [B] (read only with jit).
    Returns (values [B,hs,ws], L [B,hs,ws], tapmax [B,1,1]): L is the largest absolute difference between horizontally adjacent and
    between vertically adjacent taps of the four read (after jitter; a tap outside the frame reads 0, as in the kernel) -- the
    bilinear surface's slope per pixel of source coordinate -- and tapmax the largest absolute tap the view can read, the maximum of
    its source frame after jitter.
    The bilinear surface is continuous but its slope changes from cell to cell, and a coordinate within rounding of a whole number
    (the identity map, a half turn) is read from either cell. With tau [B] (pixels), L is therefore the largest such difference over
    the four taps of every cell the coordinate reaches within +-tau: one cell almost everywhere, two or four next to a cell border."""
    images = np.asarray(images)
    n, H, W = images.shape
    B = len(index)
    ix, iy = source_coords(theta, H, W, hs, ws, dt)
    ix, iy = reflect_clip(ix, W, dt), reflect_clip(iy, H, dt)
    fx, fy = np.floor(ix), np.floor(iy)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    wx1, wy1 = ix - fx, iy - fy
    wx0, wy0 = (fx + dt(1)) - ix, (fy + dt(1)) - iy
    src = images[np.asarray(index, np.int64)].astype(dt)                 # [B,H,W]
    if jit is not None:
        j = np.asarray(jit).astype(dt)
        src = jitter(src, j[:, 0].reshape(B, 1, 1), j[:, 1].reshape(B, 1, 1), np.asarray(means).astype(dt).reshape(B, 1, 1), dt)
    b = np.arange(B)[:, None, None]

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        return np.where(inside, src[b, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], dt(0))

    def cell(yy, xx):
        t00, t01, t10, t11 = tap(yy, xx), tap(yy, xx + 1), tap(yy + 1, xx), tap(yy + 1, xx + 1)
        slope = np.maximum(np.maximum(np.abs(t01 - t00), np.abs(t11 - t10)), np.maximum(np.abs(t10 - t00), np.abs(t11 - t01)))
        return (t00, t01, t10, t11), slope

    (t00, t01, t10, t11), L = cell(y0, x0)
    val = t00 * (wx0 * wy0) + t01 * (wx1 * wy0) + t10 * (wx0 * wy1) + t11 * (wx1 * wy1)
    if tau is not None:
        t = np.asarray(tau, np.float64).reshape(B, 1, 1)
        xa, xb = (np.floor(np.clip(ix + d, 0, W - 1)).astype(np.int64) for d in (-t, t))
        ya, yb = (np.floor(np.clip(iy + d, 0, H - 1)).astype(np.int64) for d in (-t, t))
        for yy, xx in ((ya, xa), (ya, xb), (yb, xa), (yb, xb)):
            L = np.maximum(L, cell(yy, xx)[1])
    tapmax = np.abs(src).max(axis=(1, 2), keepdims=True)
    return val, L, tapmax


def mask_pixels(hs, ws, mh, mw):
    """The view pixel (y [mh], x [mw]) each feature-map cell reads: floor(my * hs / mh), floor(mx * ws / mw), in exact integers."""
    return np.minimum(np.arange(mh) * hs // mh, hs - 1), np.minimum(np.arange(mw) * ws // mw, ws - 1)


def mask_pixels_f32(hs, ws, mh, mw):
    """The same pick in the kernel's float32 expressions, min((int)floorf(my * ((float)hs / (float)mh)), hs - 1)."""
    sy, sx = np.float32(hs) / np.float32(mh), np.float32(ws) / np.float32(mw)
    y = np.floor(np.arange(mh).astype(np.float32) * sy).astype(np.int64)
    x = np.floor(np.arange(mw).astype(np.float32) * sx).astype(np.int64)
    return np.minimum(y, hs - 1), np.minimum(x, ws - 1)


def mask(theta, H, W, hs, ws, mh, mw, dt=np.float64):
    """(mask [B,mh,mw] bool, dist [B,mh,mw]): the cell's source coordinate lies in the open box (-1, W) x (-1, H), and its distance to
    the nearest of the four limits -1, W, -1, H."""
    ys, xs = mask_pixels(hs, ws, mh, mw)
    ix, iy = source_coords(theta, H, W, hs, ws, dt, ys=ys, xs=xs)
    m = (ix > dt(-1)) & (ix < dt(W)) & (iy > dt(-1)) & (iy < dt(H))
    dist = np.minimum(np.minimum(np.abs(ix + 1), np.abs(ix - W)), np.minimum(np.abs(iy + 1), np.abs(iy - H)))
    return m, dist
