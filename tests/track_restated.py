"""Frame-to-model tracking of include/acez.h section K3 restated in numpy float64: ACCUMULATE with the header's operation order and
summation order, UPDATE operation by operation as acezero_amd/csrc/track_solve.h has it (Python floats are IEEE doubles and nothing
here is fused), the loop per frame and the fuse / track rounds on tests/tsdf_restated.py's integration. The sparse form goes through
to_dense(): a voxel of a block without a slot reads tsdf 1, weight 0. A helper module, not a test file. Nothing here imports
acezero_amd.fusion."""
import math

import numpy as np

from tests import tsdf_restated as TR
from tests.ordered_sums import block_sums, totals  # noqa: F401  (the header's summation order; the tests call T.block_sums, T.totals)

F = np.float32
TERMS, STATE, RECORD = 29, 45, 16
RUNNING, CONVERGED, DEGENERATE = 0, 1, 2
STATUS = {RUNNING: "max_iterations", CONVERGED: "converged", DEGENERATE: "degenerate"}
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]          # the upper triangle, row-major


# ------------------------------------------------------------------------------------------------------------------ ACCUMULATE
def terms(tsdf, weight, origin, voxel_size, truncation, depth, pose, focal, ppx, ppy, depth_unit=0.001, max_depth=4.0, min_weight=1.0):
    """float64 [h * w, 29] of one frame: tsdf, weight float32 [nz,ny,nx]; depth uint16 [h,w]; pose: camera -> world, 12 doubles or
    [3,4] / [4,4]; focal, ppx, ppy, origin, voxel_size, truncation are rounded to float32 first, as the entry point receives them."""
    tsdf, weight = np.asarray(tsdf, F), np.asarray(weight, F)
    nz, ny, nx = tsdf.shape
    raw = np.asarray(depth, np.uint16)
    h, w = raw.shape
    raw = raw.reshape(-1)
    T = np.asarray(pose, np.float64).reshape(-1)[:12].reshape(3, 4)
    o, vs, tau = np.asarray(origin, F).astype(np.float64), float(F(voxel_size)), float(F(truncation))
    fo, cx, cy = float(F(focal)), float(F(ppx)), float(F(ppy))
    i = np.arange(h * w)
    ix, iy = (i % w).astype(np.float64), (i // w).astype(np.float64)
    out = np.zeros((h * w, TERMS))
    with np.errstate(all="ignore"):
        d32 = raw.astype(F) * F(depth_unit)
        ok = (raw != 0) & ~(d32 > F(max_depth))
        z = d32.astype(np.float64)
        x = ((ix - cx) * z) / fo
        y = ((iy - cy) * z) / fo
        pw = [((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)]
        g = [(pw[a] - o[a]) / vs for a in range(3)]
        fl = [np.floor(ga) for ga in g]
        for a, n in enumerate((nx, ny, nz)):
            ok &= np.isfinite(g[a]) & (fl[a] >= 0) & (fl[a] <= n - 2)
        i0, j0, k0 = (np.where(ok, fa, 0).astype(np.int64) for fa in fl)
        c, known, cut = [], ok.copy(), np.zeros(h * w, bool)
        for e in range(8):
            at = (k0 + (e >> 2), j0 + ((e >> 1) & 1), i0 + (e & 1))
            known &= weight[at] >= F(min_weight)
            cut |= ~(tsdf[at] >= F(1.0))
            c.append(tsdf[at].astype(np.float64))
        ok = known & cut
        fx, fy, fz = (g[a] - fl[a] for a in range(3))
        dx00, dx10, dx01, dx11 = c[1] - c[0], c[3] - c[2], c[5] - c[4], c[7] - c[6]
        c00, c10, c01, c11 = c[0] + fx * dx00, c[2] + fx * dx10, c[4] + fx * dx01, c[6] + fx * dx11
        dy0, dy1 = c10 - c00, c11 - c01
        c0, c1 = c00 + fy * dy0, c01 + fy * dy1
        dz = c1 - c0
        value = c0 + fz * dz
        gx0, gx1 = dx00 + fy * (dx10 - dx00), dx01 + fy * (dx11 - dx01)
        gx = gx0 + fz * (gx1 - gx0)
        gy = dy0 + fz * (dy1 - dy0)
        scale = tau / vs
        r = tau * value
        n = [scale * gx, scale * gy, scale * dz]
        a = [pw[k] - T[k, 3] for k in range(3)]
        J = n + [a[1] * n[2] - a[2] * n[1], a[2] * n[0] - a[0] * n[2], a[0] * n[1] - a[1] * n[0]]
        out[:, 0] = 1.0
        for k, (p, q) in enumerate(PAIRS):
            out[:, 1 + k] = J[p] * J[q]
        for k in range(6):
            out[:, 22 + k] = J[k] * r
        out[:, 28] = r * r
    return np.where(ok[:, None], out, 0.0)


def to_dense(tsdf_blocks, weight_blocks, block_table, dims):
    """(tsdf, weight [nz,ny,nx]) of a block-sparse volume ([n_blocks,8,8,8] storage, table int32 [bz,by,bx]): voxels of blocks without
    a slot (an entry outside 0 .. n_blocks - 1) read tsdf 1, weight 0, which is what the sparse ACCUMULATE takes them for."""
    nx, ny, nz = dims
    table = np.asarray(block_table)
    bz, by, bx = table.shape
    n_blocks = 0 if tsdf_blocks is None else len(tsdf_blocks)
    out = []
    for storage, fill in ((tsdf_blocks, 1.0), (weight_blocks, 0.0)):
        full = np.full((bz, by, bx, 8, 8, 8), fill, F)
        good = (table >= 0) & (table < n_blocks)
        if n_blocks:
            full[good] = np.asarray(storage, F)[table[good]]
        out.append(np.ascontiguousarray(full.transpose(0, 3, 1, 4, 2, 5).reshape(bz * 8, by * 8, bx * 8)[:nz, :ny, :nx]))
    return out


# ---------------------------------------------------------------------------------------------------------------------- UPDATE
def solve(s, damping, pose):
    """track_solve of acezero_amd/csrc/track_solve.h on Python floats: the new pose (12 floats), or None."""
    s = [float(v) for v in s]
    L = [[0.0] * 6 for _ in range(6)]
    for k, (i, j) in enumerate(PAIRS):
        L[i][j] = L[j][i] = s[1 + k]
    trace = ((((L[0][0] + L[1][1]) + L[2][2]) + L[3][3]) + L[4][4]) + L[5][5]
    lam = damping * (trace / 6.0)
    largest = 0.0
    for i in range(6):
        L[i][i] = L[i][i] + lam
        largest = L[i][i] if L[i][i] > largest else largest
    for j in range(6):
        d = L[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not d > 1e-12 * largest:
            return None
        root = math.sqrt(d)
        L[j][j] = root
        for i in range(j + 1, 6):
            v = L[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / root
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        v = s[22 + i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v / L[i][i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v / L[i][i]
    u = [-x[0], -x[1], -x[2]]
    hx, hy, hz = -x[3] / 2.0, -x[4] / 2.0, -x[5] / 2.0
    norm = math.sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz)
    qw, qx, qy, qz = 1.0 / norm, hx / norm, hy / norm, hz / norm
    D = [1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
         2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
         2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)]
    pose = [float(v) for v in pose]
    out = [0.0] * 12
    for r in range(3):
        for c in range(3):
            out[4 * r + c] = (D[3 * r] * pose[c] + D[3 * r + 1] * pose[4 + c]) + D[3 * r + 2] * pose[8 + c]
        out[4 * r + 3] = pose[4 * r + 3] + u[r]
    if not all(math.isfinite(v) for v in out):
        return None
    return out


def update(state, tot, rel_rms, damping, min_count, history):
    """One UPDATE on the state (float64 [45], in place) and the frame's history (float64 [max_iterations,16], in place); as
    track_update of acezero_amd/csrc/track_solve.h. The caller has checked status and record count."""
    tot = [float(v) for v in tot]
    it = int(state[13])
    count, sum_r2 = tot[0], tot[28]
    rms = math.sqrt(sum_r2 / count) if count > 0.0 else 0.0
    rec = history[it]
    rec[:12] = state[:12]
    rec[12], rec[13], rec[14] = count, sum_r2, rms
    prev_rms = float(state[15])
    state[13], state[14], state[15] = float(it + 1), count, rms
    state[16:45] = tot
    status = RUNNING
    if it >= 1 and abs(rms - prev_rms) < rel_rms:
        status = CONVERGED
    elif not all(math.isfinite(v) for v in tot) or count < min_count:
        status = DEGENERATE
    else:
        pose = solve(tot, damping, state[:12])
        if pose is None:
            status = DEGENERATE
        else:
            state[:12] = pose
    state[12] = rec[15] = float(status)


# ------------------------------------------------------------------------------------------------------------------- the loops
def new_state(cam_to_world):
    s = np.zeros(STATE)
    s[:12] = np.asarray(cam_to_world, np.float64).reshape(-1)[:12]
    return s


def track(tsdf, weight, origin, voxel_size, truncation, depths, cam_to_world, focals, ppx=None, ppy=None, depth_unit=0.001, max_depth=4.0,
          min_weight=1.0, max_iterations=10, rel_rms=1e-6, damping=1e-4, min_count=64):
    """acezero_amd.fusion's _Volume.track restated: (poses float64 [n,4,4], states [n,45], histories [n,max_iterations,16]). The
    principal point defaults to the image centre."""
    n = len(depths)
    c2w = np.asarray(cam_to_world, np.float64).reshape(n, -1, 4)
    focals = np.broadcast_to(np.asarray(focals, np.float64), (n,))
    states, histories = np.zeros((n, STATE)), np.zeros((n, max_iterations, RECORD))
    for f in range(n):
        h, w = np.asarray(depths[f]).shape
        cx = w / 2.0 if ppx is None else np.broadcast_to(ppx, (n,))[f]
        cy = h / 2.0 if ppy is None else np.broadcast_to(ppy, (n,))[f]
        state = new_state(c2w[f, :3])
        for _ in range(max_iterations):
            if state[12] != RUNNING:
                break
            t = terms(tsdf, weight, origin, voxel_size, truncation, depths[f], state[:12], focals[f], cx, cy, depth_unit, max_depth, min_weight)
            update(state, totals(block_sums(t)), rel_rms, damping, min_count, histories[f])
        states[f] = state
    poses = np.tile(np.eye(4), (n, 1, 1))
    poses[:, :3] = states[:, :12].reshape(n, 3, 4)
    return poses, states, histories


def fuse(volume, depths, cam_to_world, focals, depth_unit=0.001, max_depth=4.0):
    """tests/tsdf_restated.py's integration of the frames into a fresh Volume(**volume), the table rows made as
    acezero_amd.frames makes them: the pose inverted in float64 and rounded once, the principal point the image centre."""
    vol = TR.Volume(**volume)
    w2c = np.linalg.inv(np.asarray(cam_to_world, np.float64)).astype(F)
    n = len(depths)
    return TR.integrate(vol, depths, w2c, np.broadcast_to(np.asarray(focals, np.float64), (n,)), [d.shape[1] / 2.0 for d in depths],
                        [d.shape[0] / 2.0 for d in depths], None, depth_unit, max_depth)


def refine_poses(volume, depths, cam_to_world, focals, rounds, **track_args):
    """acezero_amd.fusion.refine_poses restated without the last fusion: (poses, per round (poses, states, histories))."""
    poses = np.array(np.asarray(cam_to_world, np.float64))
    out = []
    for _ in range(rounds):
        vol = fuse(volume, depths, poses, focals)
        tracked, states, histories = track(vol.tsdf, vol.weight, vol.origin, vol.v, vol.tau, depths, poses, focals, **track_args)
        good = states[:, 12] != DEGENERATE
        poses[good] = tracked[good]
        out.append((poses.copy(), states, histories))
    return poses, out


# ----------------------------------------------------------------------------------------------------------------- the measures
def pose_errors(poses, truth):
    """(translation error in metres [n], rotation error in degrees [n]) of camera -> world poses against the truth."""
    poses, truth = np.asarray(poses, np.float64), np.asarray(truth, np.float64)
    dt = np.linalg.norm(poses[:, :3, 3] - truth[:, :3, 3], axis=1)
    rel = np.einsum("nij,nkj->nik", poses[:, :3, :3], truth[:, :3, :3])
    return dt, np.rad2deg(np.arccos(np.clip((np.trace(rel, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)))


def relative_pose_error(poses, truth):
    """Metres [n]: the translation of (truth_k^-1 truth_k+1)^-1 (pose_k^-1 pose_k+1) over consecutive frames, cyclically."""
    poses, truth = np.asarray(poses, np.float64), np.asarray(truth, np.float64)
    rel = lambda T: np.linalg.inv(T) @ np.roll(T, -1, axis=0)
    return np.linalg.norm((np.linalg.inv(rel(truth)) @ rel(poses))[:, :3, 3], axis=1)
