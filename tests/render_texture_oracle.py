"""CPU restatement of the textured path of the rasteriser (acezero_amd/csrc/render_api.hip: acez_render_texture_build,
acez_render_frame_tex) and of the image quad geometry (ace_vis_util.get_image_box), operation for operation in float32 / int so that
frames compare bit for bit. It is the definition of the textured output: no claim of parity with OpenGL is made.

  mip chain   level k + 1 is max(1, w // 2) x max(1, h // 2); texel = (a + b + c + d + 2) >> 2 over the 2 x 2 block at (2x, 2y) of
              level k, the block's second column / row clamped to level k's last one.
  raster      textured triangle t is triangle n_flat + t of the one triangle key plane (render_oracle.triangle_keys on the joined list).
  uv          the pixel's ray r = (x + 1/2 - cx, cy - y - 1/2, -f) in camera space; e_k = r . (P_{k+1} x P_{k+2}); uv = sum e_k uv_k / sum e_k.
  lod         rho^2 = max over x, y of |d(u w, v h)|^2 from the analytic derivatives; log2(rho^2) ~ e + (m - 1) for rho^2 = m 2^e,
              m in [1, 2); lambda = half of that.
  filter      bilinear about texel centres with clamp to edge; levels floor(lambda), floor(lambda) + 1 mixed by the fraction of lambda.
"""
import numpy as np

import render_oracle as R

F = np.float32
U32 = np.uint32


# ------------------------------------------------------------------------------------------------------------------- geometry
def image_box(pose_gl, aspect_ratio, size, flip=True):
    """(xyz float64 [2,3,3], uv float64 [2,3,2]) in the acez_tex_triangle uv convention (u from the left, v from the top of the image
    as stored). get_image_box: height 0.75, width height * aspect, both times size, width negated with flip; corners (w/2, h/2),
    (w/2, -h/2), (-w/2, -h/2), (-w/2, h/2) at z = -size with uvs (1, 0), (1, 1), (0, 1), (0, 0) of the top/bottom-flipped (and, with
    flip, mirrored) image counted from its bottom left; faces (0, 1, 2), (2, 3, 0)."""
    h = 0.75
    w = h * aspect_ratio * size
    h = h * size
    if flip:
        w = -w
    q = np.array([[w / 2, h / 2, -size, 1], [w / 2, -h / 2, -size, 1], [-w / 2, -h / 2, -size, 1], [-w / 2, h / 2, -size, 1]])
    ref_uv = np.array([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.0, 0.0]])
    # the reference's image is flipud(I) (then mirrored with flip); its uv origin is the bottom left. Row (1 - v) h of flipud(I) from
    # the top is row v h of I from the top; column u of the mirror is column 1 - u of I.
    uv = np.stack([1.0 - ref_uv[:, 0] if flip else ref_uv[:, 0], ref_uv[:, 1]], 1)
    X = (np.asarray(pose_gl, np.float64) @ q.T).T
    X = X[:, :3] / X[:, 3:]
    f = [[0, 1, 2], [2, 3, 0]]
    return X[f], uv[f]


# ------------------------------------------------------------------------------------------------------------------ mip chain
def mip_chain(image):
    """The levels of a uint8 [h][w][3] image: a list of uint8 arrays, level 0 first, down to 1 x 1."""
    lv = [np.ascontiguousarray(image, np.uint8)]
    while lv[-1].shape[0] > 1 or lv[-1].shape[1] > 1:
        s = lv[-1].astype(np.int32)
        sh, sw = s.shape[:2]
        dh, dw = max(1, sh // 2), max(1, sw // 2)
        y0, x0 = 2 * np.arange(dh), 2 * np.arange(dw)
        y1, x1 = np.minimum(y0 + 1, sh - 1), np.minimum(x0 + 1, sw - 1)
        a, b = s[y0][:, x0], s[y0][:, x1]
        c, d = s[y1][:, x0], s[y1][:, x1]
        lv.append(((a + b + c + d + 2) >> 2).astype(np.uint8))
    return lv


def chain_bytes(image_or_levels):
    lv = image_or_levels if isinstance(image_or_levels, list) else mip_chain(image_or_levels)
    return np.concatenate([x.reshape(-1) for x in lv])


# ------------------------------------------------------------------------------------------------------------------------ lod
def lod(rho2, last):
    """(level a, level b or -1, fraction) of rho^2 (float32 array), levels 0 .. last."""
    rho2 = np.asarray(rho2, F)
    n = rho2.shape
    l0, l1, frac = np.zeros(n, np.int64), np.full(n, -1, np.int64), np.zeros(n, F)
    with np.errstate(invalid="ignore"):
        mag = rho2 <= F(1)
        bad = ~mag & ~(rho2 < F(np.inf))
    mid = ~mag & ~bad
    l0[bad] = last
    bits = rho2[mid].view(U32)
    ex = (bits >> U32(23)).astype(np.int64) - 127
    mf = ((bits & U32(0x7FFFFF)) | U32(0x3F800000)).view(F) - F(1)
    L = ex >> 1
    fr = ((ex & 1).astype(F) + mf) * F(0.5)
    top = L >= last
    a, b = np.where(top, last, L), np.where(top, -1, L + 1)
    l0[mid], l1[mid], frac[mid] = a, b, fr
    return l0, l1, frac


def lambda_of(rho2):
    """The level of detail the map above stands for: (e + (m - 1)) / 2, in float64 (for the CPU tests' monotonicity checks)."""
    rho2 = np.asarray(rho2, F)
    bits = rho2.view(U32)
    ex = (bits >> U32(23)).astype(np.int64) - 127
    mf = ((bits & U32(0x7FFFFF)) | U32(0x3F800000)).view(F).astype(np.float64) - 1.0
    return (ex + mf) / 2


# ------------------------------------------------------------------------------------------------------------------- sampling
def bilinear(level, u, v):
    """Float32 RGB [k,3] of one level at uv arrays u, v [k]."""
    h, w = level.shape[:2]
    s = u * F(w) - F(0.5)
    t = v * F(h) - F(0.5)
    with np.errstate(invalid="ignore"):
        s = np.where(s >= F(-1), s, F(-1)).astype(F)
        s = np.where(s > F(w), F(w), s).astype(F)
        t = np.where(t >= F(-1), t, F(-1)).astype(F)
        t = np.where(t > F(h), F(h), t).astype(F)
    fs, ft = np.floor(s), np.floor(t)
    a, b = s - fs, t - ft
    i, j = fs.astype(np.int64), ft.astype(np.int64)
    i0, i1 = np.clip(i, 0, w - 1), np.clip(i + 1, 0, w - 1)
    j0, j1 = np.clip(j, 0, h - 1), np.clip(j + 1, 0, h - 1)
    w00, w10, w01, w11 = (F(1) - a) * (F(1) - b), a * (F(1) - b), (F(1) - a) * b, a * b
    T = level.astype(F)
    t00, t10, t01, t11 = T[j0, i0], T[j0, i1], T[j1, i0], T[j1, i1]
    return ((w00[:, None] * t00 + w10[:, None] * t10) + w01[:, None] * t01) + w11[:, None] * t11


def shade(levels, m, f, W, H, xyz, uv, px, py):
    """uint8 [k,3] colours of one textured triangle (float32 world xyz [3,3], uv [3,2]) at render pixels (px, py) [k]."""
    P = [np.array(R._to_camera(m, xyz[k, 0], xyz[k, 1], xyz[k, 2]), F) for k in range(3)]
    C = []
    for k in range(3):
        a, b = P[(k + 1) % 3], P[(k + 2) % 3]
        C.append(np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F))
    cx, cy = F(0.5) * F(W), F(0.5) * F(H)
    rx = (px.astype(F) + F(0.5)) - cx
    ry = cy - (py.astype(F) + F(0.5))
    rz = -f
    uv = np.asarray(uv, F)
    with np.errstate(all="ignore"):
        e = [(rx * C[k][0] + ry * C[k][1]) + rz * C[k][2] for k in range(3)]
        D = (e[0] + e[1]) + e[2]
        U = ((e[0] * uv[0, 0] + e[1] * uv[1, 0]) + e[2] * uv[2, 0]) / D
        V = ((e[0] * uv[0, 1] + e[1] * uv[1, 1]) + e[2] * uv[2, 1]) / D
        Dx = (C[0][0] + C[1][0]) + C[2][0]
        Dy = (C[0][1] + C[1][1]) + C[2][1]
        Nux = (C[0][0] * uv[0, 0] + C[1][0] * uv[1, 0]) + C[2][0] * uv[2, 0]
        Nvx = (C[0][0] * uv[0, 1] + C[1][0] * uv[1, 1]) + C[2][0] * uv[2, 1]
        Nuy = (C[0][1] * uv[0, 0] + C[1][1] * uv[1, 0]) + C[2][1] * uv[2, 0]
        Nvy = (C[0][1] * uv[0, 1] + C[1][1] * uv[1, 1]) + C[2][1] * uv[2, 1]
        h0, w0 = levels[0].shape[:2]
        sx = ((Nux - U * Dx) / D) * F(w0)
        tx = ((Nvx - V * Dx) / D) * F(h0)
        sy = ((Nuy - U * Dy) / D) * F(w0)
        ty = ((Nvy - V * Dy) / D) * F(h0)
        r2x = sx * sx + tx * tx
        r2y = sy * sy + ty * ty
        rho2 = np.where(r2y > r2x, r2y, r2x).astype(F)
    l0, l1, frac = lod(rho2, len(levels) - 1)
    out = np.zeros((len(px), 3), F)
    for lv in np.unique(l0):
        s = l0 == lv
        out[s] = bilinear(levels[lv], U[s], V[s])
    for lv in np.unique(l1[l1 >= 0]):
        s = l1 == lv
        c1 = bilinear(levels[lv], U[s], V[s])
        fr = frac[s][:, None]
        out[s] = (F(1) - fr) * out[s] + fr * c1
    return np.clip((out + F(0.5)).astype(np.int32), 0, 255).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------------- frame
def render(xyz, rgb, tri, tri_rgba, tex_tris, images, cam_to_world, znear, zfar, width, height, flipped_portrait=False):
    """The frame acez_render_frame_tex writes. tex_tris: a list of (xyz [3,3], uv [3,2], image index) textured triangles, images: the
    uint8 [h,w,3] textures."""
    m, f = R.camera(cam_to_world, znear, zfar, width, height)
    tri = np.asarray(tri, np.float32).reshape(-1, 3, 3)
    n_flat = len(tri)
    txyz = np.array([np.asarray(t[0], np.float32) for t in tex_tris], np.float32).reshape(-1, 3, 3)
    pk = R.point_keys(xyz, m, f, znear, zfar, width, height)
    tk = R.triangle_keys(np.concatenate([tri, txyz]), m, f, znear, zfar, width, height)
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    tri_rgba = np.asarray(tri_rgba, np.uint8).reshape(-1, 4)
    bg = np.zeros((width * height, 3), np.uint8)
    hit = pk != R.EMPTY
    bg[hit] = rgb[(pk[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    tid = np.where(tk != R.EMPTY, (tk & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    fg = np.zeros((width * height, 4), np.uint8)
    flat = (tid >= 0) & (tid < n_flat)
    fg[flat] = tri_rgba[tid[flat]]
    out = R.blend(bg, fg)
    chains = [mip_chain(im) for im in images]
    for t, (_, uv, ti) in enumerate(tex_tris):
        at = np.flatnonzero(tid == n_flat + t)
        if len(at):
            out[at] = shade(chains[ti], m, f, width, height, txyz[t], uv, at % width, at // width)
    out = out.reshape(height, width, 3)
    return np.ascontiguousarray(np.rot90(out, -1)) if flipped_portrait else out
