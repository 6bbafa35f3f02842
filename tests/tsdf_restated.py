"""TSDF integration and surface-net extraction of include/acez.h section K restated in numpy: the definition the HIP kernels of
acezero_amd/csrc/fusion_api.hip are compared with bit for bit (tests/test_fusion_gpu.py), checked on its own without a GPU
(tests/test_fusion_cpu.py). Written from the header's text: every float operation is a numpy float32 operation in the header's
order, one rounding each, no fused multiply-add. There is no frustum skip here: every voxel meets every frame."""
import numpy as np

F32 = np.float32
# corner numbers dx + 2 dy + 4 dz of a cell's 12 edges, lower end first, in the header's order (x edges, y edges, z edges)
EDGES = [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)]


class Volume:
    """tsdf, weight [nz,ny,nx] float32 and colour [3,nz,ny,nx] float32, cleared the way acezero_amd.fusion.TSDFVolume clears them."""

    def __init__(self, origin, dims, voxel_size, truncation, max_weight=64.0):
        self.origin = np.asarray(origin, np.float32)
        self.nx, self.ny, self.nz = (int(d) for d in dims)
        self.v, self.tau, self.max_weight = F32(voxel_size), F32(truncation), F32(max_weight)
        self.tsdf = np.ones((self.nz, self.ny, self.nx), np.float32)
        self.weight = np.zeros((self.nz, self.ny, self.nx), np.float32)
        self.colour = np.zeros((3, self.nz, self.ny, self.nx), np.float32)

    def centres(self):
        """Step 1: px [nx], py [ny], pz [nz]."""
        o, v = self.origin, self.v
        return (o[0] + np.arange(self.nx, dtype=np.float32) * v, o[1] + np.arange(self.ny, dtype=np.float32) * v,
                o[2] + np.arange(self.nz, dtype=np.float32) * v)


def integrate(vol, depths, w2c, focals, ppx, ppy, rgbs=None, depth_unit=0.001, max_depth=4.0):
    """Steps 1-9 for the frames in order. depths: list of uint16 [h,w]; w2c [n,3,4] (or [n,4,4]); rgbs: list of uint8 [h,w,3] or None."""
    x, y, z = vol.centres()
    px, py, pz = x[None, None, :], y[None, :, None], z[:, None, None]
    tau, du, md, mw = vol.tau, F32(depth_unit), F32(max_depth), vol.max_weight
    for f, raw_img in enumerate(depths):
        raw_img = np.asarray(raw_img, np.uint16)
        h, w = raw_img.shape
        m = np.asarray(w2c[f], np.float32)[:3].reshape(12)
        fo, cx, cy = F32(focals[f]), F32(ppx[f]), F32(ppy[f])
        with np.errstate(all="ignore"):
            xc = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3]
            yc = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7]
            zc = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11]
            ok = zc > F32(0.0)
            u = (fo * xc) / zc + cx
            w_ = (fo * yc) / zc + cy
            ok &= (u >= F32(-0.5)) & (u < F32(w) - F32(0.5)) & (w_ >= F32(-0.5)) & (w_ < F32(h) - F32(0.5))
            ix = np.minimum(np.where(ok, np.floor(u + F32(0.5)), 0).astype(np.int64), w - 1)
            iy = np.minimum(np.where(ok, np.floor(w_ + F32(0.5)), 0).astype(np.int64), h - 1)
            raw = raw_img[iy, ix]
            ok &= raw != 0
            d = raw.astype(np.float32) * du
            ok &= ~(d > md)
            sdf = d - zc
            ok &= ~(sdf < -tau)
            t = np.minimum(F32(1.0), sdf / tau)
            assert xc.dtype == u.dtype == d.dtype == t.dtype == np.float32
            wt = vol.weight
            w1 = wt + F32(1.0)
            vol.tsdf = np.where(ok, (vol.tsdf * wt + t) / w1, vol.tsdf)
            if rgbs is not None:
                c = np.asarray(rgbs[f], np.uint8)[iy, ix].astype(np.float32)          # [nz,ny,nx,3]
                for ch in range(3):
                    vol.colour[ch] = np.where(ok, (vol.colour[ch] * wt + c[..., ch]) / w1, vol.colour[ch])
            vol.weight = np.where(ok, np.minimum(w1, mw), wt)
    return vol


def extract(tsdf, weight, colour, origin, voxel_size, min_weight):
    """(vertices float32 [V,3], colours uint8 [V,3], faces int32 [F,3]) of a volume; colour may be None (colours are then zeros)."""
    tsdf, weight = np.asarray(tsdf, np.float32), np.asarray(weight, np.float32)
    nz, ny, nx = tsdf.shape
    o, v = np.asarray(origin, np.float32), F32(voxel_size)
    known = weight >= F32(min_weight)
    inside = tsdf < F32(0.0)
    active = np.zeros((nz, ny, nx), bool)
    if min(nx, ny, nz) >= 2:
        def corner(a, c):
            dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
            return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
        all_known = np.ones((nz - 1, ny - 1, nx - 1), bool)
        n_in = np.zeros((nz - 1, ny - 1, nx - 1), np.int32)
        for c in range(8):
            all_known &= corner(known, c)
            n_in += corner(inside, c)
        active[:nz - 1, :ny - 1, :nx - 1] = all_known & (n_in != 0) & (n_in != 8)
    rank = np.cumsum(active.reshape(-1)).astype(np.int64)                              # inclusive; vertex id = rank - 1
    cells = np.flatnonzero(active.reshape(-1))
    k, j, i = np.unravel_index(cells, (nz, ny, nx))
    V = len(cells)
    ssum, csum, count = np.zeros((V, 3), np.float32), np.zeros((V, 3), np.float32), np.zeros(V, np.int32)
    with np.errstate(all="ignore"):
        for a, b in EDGES:
            oa, ob = ((a & 1, (a >> 1) & 1, a >> 2), (b & 1, (b >> 1) & 1, b >> 2))
            da, db = tsdf[k + oa[2], j + oa[1], i + oa[0]], tsdf[k + ob[2], j + ob[1], i + ob[0]]
            cross = (da < F32(0.0)) != (db < F32(0.0))
            s = da / (da - db)
            for ax in range(3):
                pa, pb = F32(oa[ax]), F32(ob[ax])
                ssum[:, ax] = np.where(cross, ssum[:, ax] + (pa + s * (pb - pa)), ssum[:, ax])
            if colour is not None:
                for ch in range(3):
                    ca, cb = colour[ch][k + oa[2], j + oa[1], i + oa[0]], colour[ch][k + ob[2], j + ob[1], i + ob[0]]
                    csum[:, ch] = np.where(cross, csum[:, ch] + (ca + s * (cb - ca)), csum[:, ch])
            count += cross
        n = count.astype(np.float32)
        idx = np.stack([i, j, k], 1).astype(np.float32)
        vertices = o[None, :] + (idx + ssum / n[:, None]) * v
        colours = np.minimum(np.maximum(np.floor(csum / n[:, None] + F32(0.5)), F32(0.0)), F32(255.0)).astype(np.uint8)
    assert vertices.dtype == np.float32
    if colour is None:
        colours = np.zeros((V, 3), np.uint8)
    faces = []
    dims, stride = (nx, ny, nz), (1, nx, nx * ny)
    act = active.reshape(-1)
    kn, ins = known.reshape(-1), inside.reshape(-1)
    p = np.stack(np.unravel_index(np.arange(nx * ny * nz), (nz, ny, nx))[::-1], 0)       # p[0] = i, p[1] = j, p[2] = k
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        ok = (p[a] < dims[a] - 1) & (p[b] >= 1) & (p[b] < dims[b] - 1) & (p[c] >= 1) & (p[c] < dims[c] - 1)
        at = np.flatnonzero(ok)
        hi = at + stride[a]
        cell = [at - stride[b] - stride[c], at - stride[c], at, at - stride[b]]
        quad = kn[at] & kn[hi] & (ins[at] != ins[hi]) & act[cell[0]] & act[cell[1]] & act[cell[2]] & act[cell[3]]
        at = at[quad]
        v0, v1, v2, v3 = (rank[cl[quad]] - 1 for cl in cell)
        low = ins[at]
        tri = np.empty((len(at), 2, 3), np.int64)
        tri[:, 0, 0], tri[:, 0, 1], tri[:, 0, 2] = v0, np.where(low, v1, v2), np.where(low, v2, v1)
        tri[:, 1, 0], tri[:, 1, 1], tri[:, 1, 2] = v0, np.where(low, v2, v3), np.where(low, v3, v2)
        faces.append(tri.reshape(-1, 3))
    return vertices, colours, np.concatenate(faces, 0).astype(np.int32)
