"""CPU: the image quad inside the registration frustums (render.image_box, CameraTrajectory.add_camera_frustum(image=...)) against
numbers worked out by hand from ace_vis_util.get_image_box, the mip chain and level-of-detail map of tests/render_texture_oracle.py,
and the texture size query of libacez.so."""
import ctypes as C

import numpy as np
import pytest

import render_texture_oracle as T
from acezero_amd import render


def _corners(xyz, uv):
    """{(u, v): vertex} of the two triangles (each corner once)."""
    out = {}
    for tri, tuv in zip(xyz, uv):
        for p, q in zip(tri, tuv):
            out[(float(q[0]), float(q[1]))] = np.asarray(p)
    return out


# get_image_box with cam_marker_size s and the image's w / h = a: height 0.75 s, width 0.75 a s (negated with flip), the plane at
# z = -s; corners (w/2, h/2), (w/2, -h/2), (-w/2, -h/2), (-w/2, h/2) with the reference's uvs (1,0), (1,1), (0,1), (0,0) of the
# top/bottom-flipped image (mirrored left/right with flip), counted from its bottom left. In the image as stored (row 0 on top):
#   flip=True : (-|w|/2,  h/2) -> (0, 0)  top left      (|w|/2, h/2) -> (1, 0)  top right
#               (-|w|/2, -h/2) -> (0, 1)  bottom left   (|w|/2, -h/2) -> (1, 1) bottom right
#   flip=False: the same four pairs (the negated width and the mirror cancel).
@pytest.mark.parametrize("aspect,size,half_w,half_h", [(4 / 3, 0.3, 0.15, 0.1125), (0.75, 0.2, 0.05625, 0.075), (640 / 480, 1.0, 0.5, 0.375)])
@pytest.mark.parametrize("flip", [True, False])
def test_image_box_corners_by_hand(aspect, size, half_w, half_h, flip):
    xyz, uv = render.image_box(np.eye(4), aspect, size, flip=flip)
    assert xyz.shape == (2, 3, 3) and uv.shape == (2, 3, 2)
    got = _corners(xyz, uv)
    want = {(0.0, 0.0): [-half_w, half_h, -size], (1.0, 0.0): [half_w, half_h, -size], (0.0, 1.0): [-half_w, -half_h, -size],
            (1.0, 1.0): [half_w, -half_h, -size]}
    assert set(got) == set(want)
    for k in want:
        assert np.allclose(got[k], want[k], atol=1e-15), (k, got[k], want[k])
    # faces (0, 1, 2), (2, 3, 0) of the corners listed in the reference's order
    first = [-half_w, half_h, -size] if flip else [half_w, half_h, -size]
    assert np.allclose(xyz[0, 0], first) and np.allclose(xyz[1, 2], first) and np.allclose(xyz[0, 2], xyz[1, 0])
    ref = T.image_box(np.eye(4), aspect, size, flip)
    assert np.array_equal(ref[0], xyz) and np.array_equal(ref[1], uv)


def test_image_box_follows_the_pose():
    P = np.eye(4)
    P[:3, :3] = np.diag([-1.0, -1.0, 1.0])                      # 180 degrees about z
    P[:3, 3] = [1.0, 2.0, 3.0]
    xyz, uv = render.image_box(P, 4 / 3, 0.3)
    c = _corners(xyz, uv)
    assert np.allclose(c[(0.0, 0.0)], [1.15, 1.8875, 2.7]) and np.allclose(c[(1.0, 1.0)], [0.85, 2.1125, 2.7])


def test_frustum_image_sets_the_aspect_ratio_for_later_frustums():
    tr = render.CameraTrajectory(frustum_skip=0, frustum_scale=0.3)
    assert tr.aspect_ratio == 4 / 3
    plain = render.frustum_outline(np.eye(4), size=0.3).verts
    portrait = np.zeros((640, 480, 3), np.uint8)
    tr.add_camera_frustum(np.eye(4), sparse=False, image=portrait)
    assert tr.aspect_ratio == 0.75 and len(tr.frustums) == 1 and len(tr.frustum_images) == 1
    xyz, uv, img = tr.frustum_images[0]
    assert img is portrait and np.array_equal(xyz, render.image_box(np.eye(4), 0.75, 0.3)[0])
    tall = render.frustum_outline(np.eye(4), size=0.3, aspect_ratio=0.75).verts
    assert np.array_equal(tr.frustums[0].verts, tall) and not np.array_equal(tall, plain)
    tr.clear_frustums()
    assert tr.frustums == [] and tr.frustum_images == []
    tr.add_camera_frustum(np.eye(4), sparse=False)                # no image: the last image's aspect ratio persists
    assert tr.aspect_ratio == 0.75 and np.array_equal(tr.frustums[0].verts, tall) and tr.frustum_images == []
    tr.add_camera_frustum(np.eye(4), sparse=False, image=np.zeros((480, 640, 3), np.uint8))
    assert tr.aspect_ratio == 640 / 480 and len(tr.frustum_images) == 1
    # a sparse frustum that is skipped adds no image either
    tr2 = render.CameraTrajectory(frustum_skip=1.0)
    tr2.add_camera_frustum(np.eye(4), image=portrait)
    tr2.add_camera_frustum(np.eye(4), image=np.zeros((10, 40, 3), np.uint8))
    assert len(tr2.frustums) == 1 and len(tr2.frustum_images) == 1 and tr2.aspect_ratio == 0.75


def _mip_by_definition(level):
    h, w = level.shape[:2]
    dh, dw = max(1, h // 2), max(1, w // 2)
    out = np.zeros((dh, dw, 3), np.uint8)
    for y in range(dh):
        for x in range(dw):
            ys, xs = (2 * y, min(2 * y + 1, h - 1)), (2 * x, min(2 * x + 1, w - 1))
            for c in range(3):
                s = sum(int(level[yy, xx, c]) for yy in ys for xx in xs)
                out[y, x, c] = (s + 2) // 4
    return out


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (5, 3), (1, 7), (481, 641)])
def test_mip_chain_on_odd_sizes(h, w):
    from acezero_amd import _native as N
    rng = np.random.default_rng(h * 1000 + w)
    img = rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    lv = T.mip_chain(img)
    shapes = [(h, w)]
    while shapes[-1] != (1, 1):
        shapes.append((max(1, shapes[-1][0] // 2), max(1, shapes[-1][1] // 2)))
    assert [x.shape[:2] for x in lv] == shapes
    assert np.array_equal(lv[0], img)
    small = [k for k in range(1, len(lv)) if lv[k - 1].size <= 5000]
    for k in small:
        assert np.array_equal(lv[k], _mip_by_definition(lv[k - 1])), k
    if (h, w) == (3, 5):                                           # level 1 is 1 x 2: blocks rows 0-1 x columns 0-1 and 2-3
        a = img[:2, :4].astype(int)
        assert np.array_equal(lv[1][0, 0], (a[:, :2].sum(axis=(0, 1)) + 2) // 4)
        assert np.array_equal(lv[1][0, 1], (a[:, 2:].sum(axis=(0, 1)) + 2) // 4)
        l1 = lv[1].astype(int)                                     # 1 high: the block's second row clamps to row 0
        assert np.array_equal(lv[2][0, 0], (l1[0, 0] * 2 + l1[0, 1] * 2 + 2) // 4)
    levels, nbytes = C.c_int(), C.c_int64()
    assert N.lib().acez_render_texture_size(w, h, C.byref(levels), C.byref(nbytes)) == 0
    assert levels.value == len(lv) and nbytes.value == len(T.chain_bytes(lv))


def test_texture_size_query_refuses_bad_sizes():
    from acezero_amd import _native as N
    levels, nbytes = C.c_int(), C.c_int64()
    lib = N.lib()
    assert lib.acez_render_texture_size(0, 4, C.byref(levels), C.byref(nbytes)) == -1
    assert lib.acez_render_texture_size(4, 16385, C.byref(levels), C.byref(nbytes)) == -1
    assert lib.acez_render_texture_size(4, 4, None, C.byref(nbytes)) == -1
    assert lib.acez_render_texture_size(640, 480, C.byref(levels), C.byref(nbytes)) == 0 and levels.value == 10


def test_lod_map_is_monotone_and_continuous_at_level_boundaries():
    # every float32 rho^2 in [2^-4, 2^24] at a stride, plus each power of two and its neighbours
    lo, hi = np.float32(2.0 ** -4).view(np.uint32), np.float32(2.0 ** 24).view(np.uint32)
    grid = np.arange(lo, hi, 997, dtype=np.uint32).view(np.float32)
    lam = T.lambda_of(grid)
    assert np.all(np.diff(lam) >= 0)
    for e in range(-3, 24):
        p = np.float32(2.0 ** e)
        below, at = np.nextafter(p, np.float32(0)), p
        assert T.lambda_of(at) == e / 2 and 0 <= T.lambda_of(at) - T.lambda_of(below) < 1e-6
    assert np.max(np.abs(lam - np.log2(grid.astype(np.float64)) / 2)) < 0.05      # (m - 1) stays within 0.09 of log2 m
    # the two levels and the fraction: continuous through each integer lambda (rho^2 = 4^k)
    last = 12
    for k in range(1, last):
        p = np.float32(4.0 ** k)
        a0, a1, fa = T.lod(np.array([np.nextafter(p, np.float32(0))], np.float32), last)
        b0, b1, fb = T.lod(np.array([p], np.float32), last)
        assert (a0[0], a1[0]) == (k - 1, k) and fa[0] > 1 - 1e-6
        assert (b0[0], b1[0]) == (k, k + 1) and fb[0] == 0
    m0, m1, fm = T.lod(np.array([0.0, 0.5, 1.0, np.nextafter(np.float32(1), np.float32(2)), np.inf, np.nan], np.float32), last)
    assert list(m0) == [0, 0, 0, 0, last, last] and list(m1) == [-1, -1, -1, 1, -1, -1] and fm[3] < 1e-6
    t0, t1, _ = T.lod(np.array([np.float32(4.0 ** last), np.float32(4.0 ** (last + 3))], np.float32), last)
    assert list(t0) == [last, last] and list(t1) == [-1, -1]


def _look_at(eye, target):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross([0, 1.0, 0], z)
    x /= np.linalg.norm(x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, np.cross(z, x), z, eye
    return P


def test_oracle_draws_the_image_upright_in_front_of_the_camera():
    """Looking along a query camera from behind it, the image's top-left quadrant (red) is drawn at the top left of the quad."""
    img = np.zeros((60, 80, 3), np.uint8)
    img[:30, :40] = (255, 0, 0)
    img[30:, 40:] = (0, 0, 255)
    quad, uv = render.image_box(np.eye(4), 80 / 60, 1.0)
    tex = [(quad[k], uv[k], 0) for k in range(2)]
    view = np.eye(4)
    view[2, 3] = 1.0                                               # one metre behind the query camera, looking the same way
    W, H = 160, 90
    frame = T.render(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3, 3), np.float32), np.zeros((0, 4), np.uint8),
                     tex, [img], view, 0.05, 100.0, W, H)
    # the quad spans x in [-0.5, 0.5], y in [-0.375, 0.375] at distance 2: f = 45 sqrt(3) px, so +-19.5 px across, +-14.6 px up/down
    f = 0.5 * H * np.sqrt(3)
    hx, hy = 0.5 / 2 * f, 0.375 / 2 * f
    cx, cy = W / 2, H / 2
    tl = frame[int(cy - hy / 2), int(cx - hx / 2)]
    br = frame[int(cy + hy / 2), int(cx + hx / 2)]
    tr_, bl = frame[int(cy - hy / 2), int(cx + hx / 2)], frame[int(cy + hy / 2), int(cx - hx / 2)]
    assert tuple(tl) == (255, 0, 0) and tuple(br) == (0, 0, 255) and tuple(tr_) == (0, 0, 0) and tuple(bl) == (0, 0, 0)
    assert not frame[:int(cy - hy) - 1].any() and not frame[:, :int(cx - hx) - 1].any()
