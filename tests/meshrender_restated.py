"""numpy restatement of include/acez.h section R (acezero_amd/csrc/meshrender_api.hip): a triangle mesh rasterised into the frames of
a table, in float32 with one rounding per operation in the header's order, int64 edge functions, and the per-pixel minimum of the
packed key. A helper module, not a test file. The per-vertex and per-sample arithmetic is written once over arrays (numpy's float32
element-wise operations are the IEEE ones the device performs, so an array expression is the loop over frames and triangles with the
same bits); only the near-plane clipping, which few triangles need, is a Python loop."""
import numpy as np

F32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SUB = 256
GUARD = F32(2097152.0)
CHUNK = 1 << 22                      # samples evaluated at a time


class Row:
    """A frame of the table: m float32 [12] (world -> camera rows), focal, ppx, ppy float32, h, w."""

    def __init__(self, m, focal, ppx, ppy, h, w):
        self.m = np.asarray(m, np.float32).reshape(12)
        self.focal, self.ppx, self.ppy, self.h, self.w = F32(focal), F32(ppx), F32(ppy), int(h), int(w)


def rows(sizes, cam_to_world=None, world_to_cam=None, focals=None, ppx=None, ppy=None):
    """The rows acezero_amd.frames builds for these frames: poses through frames._w2c34, the principal point at (w / 2, h / 2) by default."""
    from acezero_amd.frames import _per_frame, _w2c34
    n = len(sizes)
    w2c, focals = _w2c34(world_to_cam, cam_to_world, n), _per_frame(focals, n)
    ppx, ppy = (None if p is None else _per_frame(p, n) for p in (ppx, ppy))
    return [Row(w2c[f], focals[f], w / 2.0 if ppx is None else ppx[f], h / 2.0 if ppy is None else ppy[f], h, w) for f, (h, w) in enumerate(sizes)]


def to_camera(row, p):
    """Step 1 for points float32 [n,3]: float32 [n,3]."""
    m, x, y, z = row.m, p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((m[0] * x + m[1] * y) + m[2] * z) + m[3], ((m[4] * x + m[5] * y) + m[6] * z) + m[7],
                     ((m[8] * x + m[9] * y) + m[10] * z) + m[11]], 1)


def _clip_point(a, b, znear):                      # a inside, b outside; float32 scalars throughout
    t = (znear - a[2]) / (b[2] - a[2])
    return np.array([a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), znear], np.float32)


def clip_near(c, znear):
    """Step 2 for one triangle c float32 [3,3] that crosses the plane: its 3 or 4 points."""
    inn = c[:, 2] >= znear
    poly = []
    for k in range(3):
        k1 = (k + 1) % 3
        if inn[k]:
            poly.append(c[k])
        if inn[k] != inn[k1]:
            poly.append(_clip_point(c[k], c[k1], znear) if inn[k] else _clip_point(c[k1], c[k], znear))
    return poly


def _edge(ax, ay, bx, by, px, py):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def _owns(ax, ay, bx, by):
    return ((by - ay) > 0) | (((by - ay) == 0) & ((bx - ax) < 0))


def camera_triangles(vertices, faces, row, min_depth):
    """Steps 1-2: (q float32 [n,3,3] camera-space triangles in front of the near plane, ids int64 [n], clipped bool [n])."""
    v, f = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    ids = np.nonzero(ok)[0]
    with np.errstate(all="ignore"):
        c = np.stack([to_camera(row, v[f[ids, k]]) for k in range(3)], 1) if len(ids) else np.zeros((0, 3, 3), np.float32)
    finite = np.isfinite(c).all((1, 2))
    c, ids = c[finite], ids[finite]
    n_in = (c[:, :, 2] >= F32(min_depth)).sum(1)
    whole = n_in == 3
    q, qi, qc = [c[whole]], [ids[whole]], [np.zeros(int(whole.sum()), bool)]
    for k in np.nonzero((n_in > 0) & ~whole)[0]:
        poly = clip_near(c[k], F32(min_depth))
        fan = [np.stack([poly[0], poly[1], poly[2]])] + ([np.stack([poly[0], poly[2], poly[3]])] if len(poly) == 4 else [])
        q.append(np.stack(fan))
        qi.append(np.full(len(fan), ids[k]))
        qc.append(np.ones(len(fan), bool))
    return np.concatenate(q), np.concatenate(qi), np.concatenate(qc)


def setup(q, row):
    """Steps 3-5 for triangles q [n,3,3]: dict of X, Y int64 [n,3], iz float32 [n,3], area int64 [n], x0, y0, bw, count int64 [n]
    (count 0: nothing to draw) and guard bool [n]."""
    with np.errstate(all="ignore"):
        a = (row.focal * q[:, :, 0]) / q[:, :, 2]
        b = (row.focal * q[:, :, 1]) / q[:, :, 2]
        guard = ~((np.abs(a) < GUARD) & (np.abs(b) < GUARD)).all(1)
        u, v, iz = a + row.ppx, b + row.ppy, F32(1.0) / q[:, :, 2]
        X = np.where(guard[:, None], 0, np.rint(u * F32(SUB))).astype(np.int64)
        Y = np.where(guard[:, None], 0, np.rint(v * F32(SUB))).astype(np.int64)
    area = _edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    flip = area < 0
    order = np.where(flip[:, None], [0, 2, 1], [0, 1, 2])
    X, Y, iz = (np.take_along_axis(t, order, 1) for t in (X, Y, iz))
    area = np.abs(area)
    x0 = np.maximum(0, -((-X.min(1)) // SUB))
    x1 = np.minimum(row.w - 1, X.max(1) // SUB)
    y0 = np.maximum(0, -((-Y.min(1)) // SUB))
    y1 = np.minimum(row.h - 1, Y.max(1) // SUB)
    drawn = ~guard & (area != 0) & (x1 >= x0) & (y1 >= y0)
    bw = np.where(drawn, x1 - x0 + 1, 1)
    count = np.where(drawn, bw * (y1 - y0 + 1), 0)
    return dict(X=X, Y=Y, iz=iz, area=area, x0=x0, y0=y0, bw=bw, count=count, guard=guard)


def _walk(s, ids, row, max_depth, keys, pick):
    """Steps 6-8 for the triangles `pick` (indices into the set-up)."""
    count = s["count"][pick]
    rep = np.repeat(pick, count)
    j = np.arange(int(count.sum()), dtype=np.int64) - np.repeat(np.cumsum(count) - count, count)
    px, py = s["x0"][rep] + j % s["bw"][rep], s["y0"][rep] + j // s["bw"][rep]
    X, Y, iz = s["X"][rep], s["Y"][rep], s["iz"][rep]
    sx, sy = px * SUB, py * SUB
    w0 = _edge(X[:, 1], Y[:, 1], X[:, 2], Y[:, 2], sx, sy)
    w1 = _edge(X[:, 2], Y[:, 2], X[:, 0], Y[:, 0], sx, sy)
    w2 = _edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], sx, sy)
    t0, t1, t2 = _owns(X[:, 1], Y[:, 1], X[:, 2], Y[:, 2]), _owns(X[:, 2], Y[:, 2], X[:, 0], Y[:, 0]), _owns(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1])
    cover = (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & ~(((w0 == 0) & ~t0) | ((w1 == 0) & ~t1) | ((w2 == 0) & ~t2))
    with np.errstate(all="ignore"):
        invd = ((w0.astype(F32) * iz[:, 0] + w1.astype(F32) * iz[:, 1]) + w2.astype(F32) * iz[:, 2]) / s["area"][rep].astype(F32)
        d = F32(1.0) / invd
        cover &= d <= F32(max_depth)
    key = (d[cover].view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[rep[cover]].astype(np.uint64)
    np.minimum.at(keys, (py * row.w + px)[cover], key)


def frame_keys(vertices, faces, row, min_depth, max_depth):
    """(keys uint64 [h*w], EMPTY where nothing landed; 1 per triangle-frame the guard dropped, summed)."""
    q, ids, _ = camera_triangles(vertices, faces, row, min_depth)
    s = setup(q, row)
    keys = np.full(row.h * row.w, EMPTY, np.uint64)
    todo = np.nonzero(s["count"] > 0)[0]
    at = 0
    while at < len(todo):                                            # chunks of about CHUNK samples
        csum = np.cumsum(s["count"][todo[at:]])
        upto = at + max(1, int(np.searchsorted(csum, CHUNK, side="right")))
        _walk(s, ids, row, max_depth, keys, todo[at:upto])
        at = upto
    return keys, len(np.unique(ids[s["guard"]]))


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def planes(vertices, colours, faces, row, keys, depth_unit, outputs):
    """The outputs of section R from a frame's keys: dict of depth float32 [h,w], face int32 [h,w], depth_u16 uint16 [h,w], normal and
    colour uint8 [h,w,3], as requested."""
    h, w = row.h, row.w
    hit = keys != EMPTY
    d = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), F32(0.0)).astype(np.float32)
    face = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    out = {}
    if "depth" in outputs:
        out["depth"] = d.reshape(h, w)
    if "face" in outputs:
        out["face"] = face.astype(np.int32).reshape(h, w)
    if "depth_u16" in outputs:
        with np.errstate(all="ignore"):
            q = np.rint(d / F32(depth_unit))
        out["depth_u16"] = np.where(hit & (q <= F32(65535.0)), q, 0).astype(np.uint16).reshape(h, w)
    if "normal" not in outputs and "colour" not in outputs:
        return out
    pix = np.nonzero(hit)[0]
    v, f = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    idx = f[face[pix]]
    with np.errstate(all="ignore"):
        p = [to_camera(row, v[idx[:, k]]) for k in range(3)]
        r = np.stack([(pix % w).astype(F32) - row.ppx, (pix // w).astype(F32) - row.ppy, np.full(len(pix), row.focal, np.float32)], 1)
        if "normal" in outputs:
            n = _cross(p[1] - p[0], p[2] - p[0])
            along = (n[:, 0] * r[:, 0] + n[:, 1] * r[:, 1]) + n[:, 2] * r[:, 2]
            n = np.where((along > 0)[:, None], -n, n)
            length = np.sqrt(((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(np.float64)).astype(np.float32)
            good = (length > 0) & np.isfinite(length)
            byte = np.clip(np.rint((n / length[:, None]) * F32(127.0)) + F32(128.0), F32(1.0), F32(255.0))
            nrm = np.zeros((h * w, 3), np.uint8)
            nrm[pix] = np.where(good[:, None], byte, 128).astype(np.uint8)
            out["normal"] = nrm.reshape(h, w, 3)
        if "colour" in outputs:
            col = np.asarray(colours, np.uint8).reshape(-1, 3)
            e = [(r[:, 0] * c[:, 0] + r[:, 1] * c[:, 1]) + r[:, 2] * c[:, 2] for c in (_cross(p[1], p[2]), _cross(p[2], p[0]), _cross(p[0], p[1]))]
            D = (e[0] + e[1]) + e[2]
            m = ((e[0][:, None] * col[idx[:, 0]].astype(F32) + e[1][:, None] * col[idx[:, 1]].astype(F32)) + e[2][:, None] * col[idx[:, 2]].astype(F32)) / D[:, None]
            q = np.floor(m + F32(0.5))
            rgb = np.zeros((h * w, 3), np.uint8)
            rgb[pix] = np.where(q >= 0, np.minimum(q, F32(255.0)), 0).astype(np.uint8)
            out["colour"] = rgb.reshape(h, w, 3)
    return out


def render(vertices, faces, table, colours=None, min_depth=0.05, max_depth=10.0, depth_unit=0.001, outputs=("depth_u16",)):
    """(one dict of planes per row of the table, the status count)."""
    frames, status = [], 0
    for row in table:
        keys, guard = frame_keys(vertices, faces, row, min_depth, max_depth)
        status += guard
        frames.append(planes(vertices, colours, faces, row, keys, depth_unit, outputs))
    return frames, status


def depth_agreement(model, measured, tolerance):
    """acezero_amd.meshrender.depth_agreement on host arrays: (both, model_only, measured_only, sum |delta|, within)."""
    a, b = np.asarray(model).astype(np.int64), np.asarray(measured).astype(np.int64)
    both = (a > 0) & (b > 0)
    delta = np.abs(a - b)[both]
    return int(both.sum()), int(((a > 0) & (b == 0)).sum()), int(((a == 0) & (b > 0)).sum()), int(delta.sum()), int((delta <= tolerance).sum())
