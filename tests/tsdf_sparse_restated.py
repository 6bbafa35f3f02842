"""The block-sparse volume of include/acez.h section K2 restated in numpy on top of tests/tsdf_restated.py: the MARK rule in float64 in
the header's order (the flags the kernel sets are compared with it byte for byte), the sparse chain as the dense restatement with the
voxels of unmarked blocks unknown, the layout of the block storage, and the rule by which two meshes whose rows are ordered
differently are the same mesh. A helper module, not a test file."""
import numpy as np

from tests import tsdf_restated as R

F32, F64 = np.float32, np.float64
BLOCK = 8
SLACK = F64(1e-5)


def block_grid(dims):
    return tuple((int(d) + BLOCK - 1) // BLOCK for d in dims)


def mark(origin, dims, voxel_size, truncation, depths, w2c, focals, ppx, ppy, depth_unit=0.001, max_depth=4.0, flags=None):
    """uint8 [bz,by,bx]: section K2's MARK for the frames (depths: list of uint16 [h,w]; w2c [n,3,4] or [n,4,4]). `flags` continues an
    earlier call's array."""
    o = np.asarray(origin, np.float32).astype(F64)
    n3 = [int(d) for d in dims]
    v, tau = F64(F32(voxel_size)), F64(F32(truncation))
    bx, by, bz = block_grid(dims)
    if flags is None:
        flags = np.zeros((bz, by, bx), np.uint8)
    A = [np.maximum(np.abs(o[c]), np.abs(o[c] + F64(n3[c] - 1) * v)) for c in range(3)]
    for f, raw_img in enumerate(depths):
        raw_img = np.asarray(raw_img, np.uint16)
        h, w = raw_img.shape
        m = np.asarray(w2c[f], np.float32)[:3].reshape(12).astype(F64)
        r = [[m[0], m[1], m[2]], [m[4], m[5], m[6]], [m[8], m[9], m[10]]]
        t = [m[3], m[7], m[11]]
        fo, cx, cy = F64(F32(focals[f])), F64(F32(ppx[f])), F64(F32(ppy[f]))
        c = [[r[1][1] * r[2][2] - r[1][2] * r[2][1], r[0][2] * r[2][1] - r[0][1] * r[2][2], r[0][1] * r[1][2] - r[0][2] * r[1][1]],
             [r[1][2] * r[2][0] - r[1][0] * r[2][2], r[0][0] * r[2][2] - r[0][2] * r[2][0], r[0][2] * r[1][0] - r[0][0] * r[1][2]],
             [r[1][0] * r[2][1] - r[1][1] * r[2][0], r[0][1] * r[2][0] - r[0][0] * r[2][1], r[0][0] * r[1][1] - r[0][1] * r[1][0]]]
        det = (r[0][0] * c[0][0] + r[0][1] * c[1][0]) + r[0][2] * c[2][0]
        inv = [[c[a][k] / det for k in range(3)] for a in range(3)]
        e = [SLACK * (((np.abs(r[k][0]) * A[0] + np.abs(r[k][1]) * A[1]) + np.abs(r[k][2]) * A[2]) + np.abs(t[k])) for k in range(3)]
        s = [(np.abs(inv[a][0]) * e[0] + np.abs(inv[a][1]) * e[1]) + np.abs(inv[a][2]) * e[2] for a in range(3)]
        su = SLACK * ((np.abs(cx) + F64(w)) + F64(1.0))
        sv = SLACK * ((np.abs(cy) + F64(h)) + F64(1.0))
        d32 = raw_img.astype(np.float32) * F32(depth_unit)
        iy, ix = np.nonzero((raw_img != 0) & ~(d32 > F32(max_depth)))
        if len(ix) == 0:
            continue
        d = d32[iy, ix].astype(F64)
        sd = SLACK * (d + tau)
        zs = [np.maximum(d - sd, F64(0.0)), (d + tau) + sd]
        us = [(ix.astype(F64) - F64(0.5)) - su, (ix.astype(F64) + F64(0.5)) + su]
        ws = [(iy.astype(F64) - F64(0.5)) - sv, (iy.astype(F64) + F64(0.5)) + sv]
        lo = [np.full(len(ix), np.inf) for _ in range(3)]
        hi = [np.full(len(ix), -np.inf) for _ in range(3)]
        for corner in range(8):
            z = zs[corner >> 2]
            x = ((us[corner & 1] - cx) / fo) * z
            y = ((ws[(corner >> 1) & 1] - cy) / fo) * z
            q = [x - t[0], y - t[1], z - t[2]]
            for a in range(3):
                wa = (inv[a][0] * q[0] + inv[a][1] * q[1]) + inv[a][2] * q[2]
                lo[a], hi[a] = np.minimum(lo[a], wa), np.maximum(hi[a], wa)
        first = [np.maximum(np.floor(((lo[a] - s[a]) - o[a]) / v) - F64(1.0), F64(0.0)) for a in range(3)]
        last = [np.minimum(np.ceil(((hi[a] + s[a]) - o[a]) / v) + F64(1.0), F64(n3[a] - 1)) for a in range(3)]
        ok = (first[0] <= last[0]) & (first[1] <= last[1]) & (first[2] <= last[2])
        b0 = [first[a][ok].astype(np.int64) >> 3 for a in range(3)]
        b1 = [last[a][ok].astype(np.int64) >> 3 for a in range(3)]
        for box in np.unique(np.stack(b0 + b1, 1), axis=0):
            flags[box[2]:box[5] + 1, box[1]:box[4] + 1, box[0]:box[3] + 1] = 1
    return flags


def voxel_mask(flags, dims):
    """bool [nz,ny,nx]: the voxels of the marked blocks."""
    nx, ny, nz = dims
    return np.repeat(np.repeat(np.repeat(flags.astype(bool), BLOCK, 0), BLOCK, 1), BLOCK, 2)[:nz, :ny, :nx]


def sparse_chain(vol, flags, min_weight):
    """The sparse volume's mesh from a dense restated volume: what the block kernels hold is the dense volume's voxels inside the
    marked blocks, and every other voxel is unknown (weight 0, tsdf 1, the cleared state)."""
    mask = voxel_mask(flags, (vol.nx, vol.ny, vol.nz))
    tsdf = np.where(mask, vol.tsdf, F32(1.0))
    weight = np.where(mask, vol.weight, F32(0.0))
    colour = np.where(mask[None], vol.colour, F32(0.0))
    return R.extract(tsdf, weight, colour, vol.origin, vol.v, min_weight)


def to_blocks(dense, flags, fill):
    """[n_blocks,8,8,8] of a dense [nz,ny,nx] array: the marked blocks in ascending block index, `fill` beyond the grid."""
    bz, by, bx = flags.shape
    nz, ny, nx = dense.shape
    full = np.full((bz * BLOCK, by * BLOCK, bx * BLOCK), fill, dense.dtype)
    full[:nz, :ny, :nx] = dense
    rows = full.reshape(bz, BLOCK, by, BLOCK, bx, BLOCK).transpose(0, 2, 4, 1, 3, 5).reshape(-1, BLOCK, BLOCK, BLOCK)
    return np.ascontiguousarray(rows[flags.reshape(-1) != 0])


def inside_grid(flags, dims):
    """bool [n_blocks,8,8,8]: which voxels of the marked blocks lie inside the grid."""
    nx, ny, nz = dims
    return to_blocks(np.ones((nz, ny, nx), bool), flags, False)


def _rows(vertices, colours):
    v = np.ascontiguousarray(np.asarray(vertices, np.float32)).view(np.uint32).astype(np.int64)
    return np.concatenate([v, np.asarray(colours, np.uint8).astype(np.int64)], 1)


def assert_same_mesh(got, want):
    """The same mesh, whatever the order of its rows: the vertex rows with their colours are equal as sets of bit patterns (and no row
    occurs twice), and with the vertex ids renamed through those rows the face rows, ordered triples, are equal as sets."""
    gv, gc, gf = (np.asarray(a) for a in got)
    wv, wc, wf = (np.asarray(a) for a in want)
    assert gv.shape == wv.shape and gf.shape == wf.shape, (gv.shape, wv.shape, gf.shape, wf.shape)
    g_rows, w_rows = _rows(gv, gc), _rows(wv, wc)
    both, inverse = np.unique(np.concatenate([g_rows, w_rows], 0), axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    g_id, w_id = inverse[:len(g_rows)], inverse[len(g_rows):]
    assert len(np.unique(w_id)) == len(w_rows), "two vertices of the reference mesh are the same row: ids cannot be renamed through rows"
    assert len(both) == len(w_rows) and len(np.unique(g_id)) == len(g_rows), \
        f"{len(both) - len(w_rows)} vertex rows occur in one mesh only"
    g_faces = np.unique(g_id[np.asarray(gf, np.int64)].reshape(-1, 3), axis=0)
    w_faces = np.unique(w_id[np.asarray(wf, np.int64)].reshape(-1, 3), axis=0)
    assert len(g_faces) == len(gf) and len(w_faces) == len(wf), "a face occurs twice"
    assert np.array_equal(g_faces, w_faces), "the face rows differ"
