"""The view-warp cases shared by tests/test_warp_restated_cpu.py (which pins the restatement on them and measures the error bounds) and
tests/test_buffer_warp_gpu.py (which runs acez_buffer_warp_views on them), and the bounds themselves.

A case is one frame size, one canvas size, a table of four frames (three of synth.make_gray_images and a three-level pattern of period
3 px, (x + 2 y) mod 3, in which horizontally and vertically adjacent pixels always differ, so a wrong tap weight shows everywhere) and
a list of affine maps. It runs once without jitter (one view per map) and once with it (every map under every (brightness, contrast)
pair of JITTER)."""
import functools
import math

import numpy as np

from acezero_amd import synth
from tests import warp_restated as R

JITTER = [(1.0, 1.0), (0.8, 1.2), (3.0, 1.0), (1.0, 0.0), (1.2, 2.0)]   # (3, 1): brightness saturates the clamp; (1, 0): every pixel is the mean

# Bounds. r is the largest ratio, over every pixel (view) of every case, of |restatement in float32 - restatement in float64| to
#   pixels: L * eps32 * max(H, W) * g + eps32 * max|tap|      mean: eps32 * (H W / 1024 + 22)
# measured by tests/test_warp_restated_cpu.py::test_float32_restatement_stays_inside_the_recorded_ratio, which fails if a change to the
# cases makes it larger than recorded here (or less than half of it). k = 4 * max(1, r): the factor 4 is for what float32 numpy does
# not model -- contracted multiply-adds, the device's fmodf and division, its 1024-way summation order.
# Two readings the measurement forced (warp_restated.warp), both from the arithmetic and not from any device:
#   max|tap| is the largest absolute value of the view's source frame after jitter, not of the four taps: the jitter ends in
#     (g - 0.4) / 0.25, whose rounding error is eps32 * O(1) however small the result (four taps near grey 0.4 gave r = 100);
#   L covers every cell within tau of the coordinate: a coordinate within rounding of a whole number (identity, half turn) is read
#     from either cell, and a flat cell (clamped by the jitter) next to a steep one gave r = 70 with the cell's own L alone.
R_PIXEL = 2.01      # measured 2.000 (brightness 3 saturates the clamp: (1 - 0.4f) / 0.25f is two float32 roundings from 2.4)
R_MEAN = 0.04       # measured 0.038
K_PIXEL = 4.0 * max(1.0, R_PIXEL)
K_MEAN = 4.0 * max(1.0, R_MEAN)
MASK_NEAR_LIMIT = 0.005       # at most this share of a case's mask cells may lie within tau of a limit (a condition on the inputs)


def map_size(hs, ws):
    """The encoder's feature-map size of an hs x ws view: three stride-2, pad-1, 3x3 convolutions."""
    for _ in range(3):
        hs, ws = (hs - 1) // 2 + 1, (ws - 1) // 2 + 1
    return hs, ws


def _rot(deg, H, W, zoom=1.0):
    """Rotation by `deg` about the centre in pixel coordinates, source offsets scaled by `zoom` (session.warp_theta's layout)."""
    c, s = math.cos(math.radians(deg)) * zoom, math.sin(math.radians(deg)) * zoom
    return [c, -s * H / W, 0.0, s * W / H, c, 0.0]


def special_thetas(H, W):
    """name -> map. Identity; quarter and half turns in normalised coordinates (exact: source coordinates fall on pixel centres);
    45 degrees; a zoom-out by 5.37 with a translation, whose source coordinates run from two frame widths left of the frame to three
    right of it (0, 1, 2 and 3 flips of the reflection; 3.37 reaches only 2); a zoom-in by 0.31 that stays inside the frame."""
    return {"identity": [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], "rot90": [0.0, -1.0, 0.0, 1.0, 0.0, 0.0], "rot180": [-1.0, 0.0, 0.0, 0.0, -1.0, 0.0],
            "rot45": _rot(45.0, H, W), "zoom_out": [5.37, 0.0, 0.41, 0.0, 5.37, -0.83], "zoom_in": [0.31, 0.0, 0.0, 0.0, 0.31, 0.0]}


def _pattern(H, W):
    lv = np.array([0.1, 0.5, 0.9])[(np.arange(W)[None, :] + 2 * np.arange(H)[:, None]) % 3]
    return ((lv - 0.4) / 0.25).astype(np.float32)


@functools.lru_cache(maxsize=None)
def images(H, W):
    return np.ascontiguousarray(np.concatenate([synth.make_gray_images(seed=3, n=3, h=H, w=W)[:, 0], _pattern(H, W)[None]]))


def _session_thetas(H, W, scale, seed):
    from acezero_amd import session
    ang = np.radians(np.random.default_rng(seed).uniform(-15, 15, size=7))
    th, hs, ws = session.warp_theta(H, W, scale, ang)
    return th.reshape(7, 6).numpy(), hs, ws


@functools.lru_cache(maxsize=None)
def geometry():
    """name -> (H, W, hs, ws, theta float32 [T,6], index int32 [T], names [T])."""
    out = {}
    for name, scale, seed in (("scale094", 0.94, 11), ("scale106", 1.06, 12)):                  # the production shape, session.warp_theta
        th, hs, ws = _session_thetas(120, 168, scale, seed)
        out[name] = (120, 168, hs, ws, th, [3, 0, 2, 2, 1, 3, 0], [f"rot{i}" for i in range(7)])
    # special maps on the production frame; then odd sizes with hs * ws no multiple of 256; then a frame of fewer than 1024 pixels
    for name, (H, W, hs, ws) in (("special", (120, 168, 120, 168)), ("odd", (37, 53, 35, 50)), ("small", (24, 40, 24, 40))):
        sp = special_thetas(H, W)
        sp["tilt_zoom"] = _rot(-11.0, H, W, zoom=0.97)
        sp["tilt_pattern"] = _rot(7.0, H, W, zoom=1.04)
        index = [0, 3, 1, 3, 3, 2, 3, 3]                                                       # repeated and non-monotone
        out[name] = (H, W, hs, ws, np.asarray(list(sp.values()), np.float32), index, list(sp.keys()))
    return {k: (H, W, hs, ws, np.ascontiguousarray(th, np.float32), np.asarray(ix, np.int32), nm) for k, (H, W, hs, ws, th, ix, nm) in out.items()}


GEOMETRIES = ["scale094", "scale106", "special", "odd", "small"]


def case(name, with_jitter):
    """dict(H, W, hs, ws, images [4,H,W], index [B], theta [B,6], jitter [B,2] or None, names [B], g [B])."""
    H, W, hs, ws, th, ix, nm = geometry()[name]
    jt = None
    if with_jitter:
        T = len(ix)
        jt = np.repeat(np.asarray(JITTER, np.float32), T, axis=0)
        th, ix, nm = np.tile(th, (len(JITTER), 1)), np.tile(ix, len(JITTER)), [f"{n}/{b},{c}" for b, c in JITTER for n in nm]
    g = np.maximum(1.0, np.abs(th.astype(np.float64)[:, [0, 1, 3, 4]]).max(axis=1))
    return dict(name=name, H=H, W=W, hs=hs, ws=ws, images=images(H, W), index=ix, theta=np.ascontiguousarray(th), jitter=jt, names=nm, g=g)


def pixel_bracket(c, L, tapmax):
    """[B,hs,ws]: L * eps32 * max(H, W) * g + eps32 * max|tap| (multiply by K_PIXEL for the bound)."""
    return L * (R.EPS32 * max(c["H"], c["W"]) * c["g"])[:, None, None] + R.EPS32 * tapmax


def mean_bracket(c):
    return R.EPS32 * (c["H"] * c["W"] / 1024.0 + 22.0)


def mask_tau(c):
    """[B]: K_PIXEL * eps32 * max(H, W) * g, the distance to a limit below which a mask cell may fall either way."""
    return K_PIXEL * R.EPS32 * max(c["H"], c["W"]) * c["g"]


def mask_sizes(c):
    """The mask at feature resolution (what production asks for) and at full view resolution (every pixel's coordinate)."""
    return [map_size(c["hs"], c["ws"]), (c["hs"], c["ws"])]
