"""numpy restatement of Pillow's 8-bit resize(BILINEAR) and convert("L") (include/acez.h section I states the arithmetic), written for
the ingest tests: tests/test_ingest_cpu.py pins it to the installed Pillow and the library's tables to it, tests/test_ingest_gpu.py
compares the kernels with Pillow and cli.load_frames directly."""
import math

import numpy as np

BITS = 22

# (H, W, short side of the result)
CASES = [
    (37, 53, 16),        # downscale
    (53, 37, 16),        # downscale, portrait
    (120, 67, 16),       # downscale
    (16, 16, 16),        # identity
    (64, 96, 64),        # identity on the short side
    (33, 200, 32),       # scale just above 1
    (9, 11, 24),         # upscale, support 1
    (17, 17, 40),        # upscale, support 1
    (301, 17, 8),        # extreme aspect
    (480, 640, 16),      # scale 30, 61 taps
    (1080, 1920, 480),   # production size
]
CONTENTS = ["noise", "zeros", "full"]


def resized_size(h, w, res):
    """cli.load_frames' arithmetic: (nh, nw) of an h x w frame whose short side becomes res."""
    sc = res / min(w, h)
    nw, nh = (res, int(h * sc)) if w <= h else (int(w * sc), res)
    return nh, nw


def frames(h, w, content, n=1, seed=0):
    """uint8 [n, h, w, 3]: seeded uniform noise (n different frames), all 0 or all 255."""
    if content == "noise":
        return np.random.default_rng([seed, h, w]).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    return np.full((n, h, w, 3), 0 if content == "zeros" else 255, np.uint8)


def coeffs(n_in, n_out):
    """(ksize, int32 [n_out, 2] (first source index, tap count), int32 [n_out, ksize] taps with 22 fraction bits) of one axis."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    taps = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        k = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs)) for x in range(xmax - xmin)]
        ww = 0.0
        for w in k:                                                      # summed in order, in double
            ww += w
        bounds[xx] = (xmin, xmax - xmin)
        taps[xx, :len(k)] = [int(0.5 + (w / ww) * (1 << BITS)) for w in k]
    return ksize, bounds, taps


def _pass(img, n_out, axis):
    """One pass along `axis` of a uint8 array: (2^21 + sum pixel * tap) >> 22, clipped, stored as uint8."""
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    _, bounds, taps = coeffs(img.shape[0], n_out)
    out = np.empty((n_out,) + img.shape[1:], np.int64)
    for xx in range(n_out):
        x0, cnt = bounds[xx]
        k = taps[xx, :cnt].astype(np.int64).reshape((cnt,) + (1,) * (img.ndim - 1))
        out[xx] = ((1 << (BITS - 1)) + (img[x0:x0 + cnt] * k).sum(0)) >> BITS
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize_bilinear(rgb, nh, nw):
    """uint8 [h, w, 3] -> uint8 [nh, nw, 3]: the horizontal pass first, its uint8 result into the vertical pass."""
    return _pass(_pass(rgb, nw, 1), nh, 0)


def to_grey(rgb):
    v = rgb.astype(np.int64)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def pillow_resize(rgb, nh, nw):
    """(uint8 [nh, nw, 3], uint8 grey [nh, nw]) as cli.load_frames gets them from Pillow."""
    from PIL import Image
    small = Image.fromarray(rgb).convert("RGB").resize((nw, nh), Image.BILINEAR)
    return np.asarray(small, np.uint8), np.asarray(small.convert("L"), np.uint8)


def host_normalise(grey):
    """cli.load_frames' float32 frame of a uint8 grey image."""
    return (np.asarray(grey, np.float32) / 255.0 - 0.4) / 0.25
