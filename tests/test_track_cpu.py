"""CPU: frame-to-model tracking of include/acez.h section K3 on its numpy restatement (tests/track_restated.py): the host
instantiation of the device-side update (acezero_amd/csrc/track_solve.h, through tests/track_probe.hip) against the restated update bit
for bit; the restated loop on the wide-lens room of tests/track_cases.py, whose figures are the bounds the kernels are held to in
tests/test_track_gpu.py; the entry points' argument checks and fuse_depth.py's new flags, none of which needs a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import track_cases as TC
from tests import track_restated as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def probe():
    so = os.path.join(HERE, "_build", "libtrack_probe.so")
    src = os.path.join(HERE, "track_probe.hip")
    deps = [src] + [os.path.join(ROOT, "acezero_amd", "csrc", f) for f in ("track_solve.h", "device_loop.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                        "-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.probe_track_solve.restype = C.c_int
    lib.probe_track_solve.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    lib.probe_track_update.restype = None
    lib.probe_track_update.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    """Equal bit for bit, except that a NaN equals a NaN: IEEE 754 leaves a NaN's sign and payload to the implementation."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | both_nan).all())


@pytest.fixture(scope="module")
def truth_volume():
    depths, truth, _, focal = TC.room()
    return T.fuse(TC.ROOM_VOLUME, depths, truth, focal)


def room_totals(vol, frame):
    depths, _, perturbed, focal = TC.room()
    t = T.terms(vol.tsdf, vol.weight, vol.origin, vol.v, vol.tau, depths[frame], perturbed[frame, :3], focal, TC.ROOM_W / 2.0, TC.ROOM_H / 2.0)
    return T.totals(T.block_sums(t)), perturbed[frame]


def plane_totals(n=400, offset=0.005, seed=0):
    """Totals of n points on one plane z = const seen from the origin: normals (0, 0, 1), residual `offset` plus 1 mm of noise. The
    system has rank 3: sliding along x and y and turning about z are not observed."""
    g = np.random.default_rng(seed)
    a = np.c_[g.uniform(-1, 1, n), g.uniform(-1, 1, n), np.full(n, 1.5)]
    r = offset + g.normal(scale=0.001, size=n)
    nrm = np.tile([0.0, 0.0, 1.0], (n, 1))
    J = np.c_[nrm, np.cross(a, nrm)]
    t = np.zeros((n, T.TERMS))
    t[:, 0] = 1.0
    for k, (i, j) in enumerate(T.PAIRS):
        t[:, 1 + k] = J[:, i] * J[:, j]
    t[:, 22:28] = J * r[:, None]
    t[:, 28] = r * r
    return T.totals(T.block_sums(t))


def both_updates(probe, pose, tot, records=0, prev_rms=0.0, rel_rms=1e-6, damping=1e-4, min_count=64):
    """(state, history) after one UPDATE, restated and through the probe."""
    out = []
    for native in (False, True):
        state = T.new_state(pose)
        state[13], state[15] = records, prev_rms
        history = np.zeros((4, T.RECORD))
        tot = np.ascontiguousarray(tot, np.float64)
        if native:
            probe.probe_track_update(_p(state), _p(tot), rel_rms, damping, float(min_count), _p(history))
        else:
            T.update(state, tot, rel_rms, damping, min_count, history)
        out.append((state, history))
    return out


def test_summation_order():
    rng = np.random.default_rng(0)
    for n in (1, 64, 65, 255, 256, 257, 2745):
        t = rng.normal(size=(n, T.TERMS)) * 10.0 ** rng.integers(-6, 6, (n, 1))
        part = T.block_sums(t)
        assert part.shape == ((n + 255) // 256, T.TERMS)
        blk = len(part) - 1                                            # the last, partial tile, lane by lane
        waves = []
        for w in range(4):
            v = np.zeros((64, T.TERMS))
            rows = t[blk * 256 + w * 64: blk * 256 + (w + 1) * 64]
            v[:len(rows)] = rows
            for s in (32, 16, 8, 4, 2, 1):
                v = np.stack([v[lane] + v[lane ^ s] for lane in range(64)])
            waves.append(v[0])
        assert same_bits(part[blk], ((waves[0] + waves[1]) + waves[2]) + waves[3])
        assert np.allclose(T.totals(part), t.sum(0), rtol=1e-12, atol=1e-9 * np.abs(t).max())
    assert (T.totals(np.ones((700, T.TERMS))) == 700).all()           # more partial rows than UPDATE has threads


def test_update_well_conditioned(probe, truth_volume):
    for frame in (0, 7, 13):
        tot, pose = room_totals(truth_volume, frame)
        (s_r, h_r), (s_n, h_n) = both_updates(probe, pose, tot)
        assert same_bits(s_r, s_n) and same_bits(h_r, h_n)
        assert s_r[12] == T.RUNNING and s_r[13] == 1 and h_r[0, 15] == T.RUNNING
        assert same_bits(h_r[0, :12], pose[:3].reshape(12)) and not same_bits(s_r[:12], pose[:3].reshape(12))
        assert np.linalg.norm(s_r[[3, 7, 11]] - pose[:3, 3]) < 0.05 and same_bits(s_r[16:45], tot)
        # the second record under rule (a): an rms within rel_rms of the previous one converges and leaves the pose alone
        rms = h_r[0, 14]
        (s_r, h_r), (s_n, h_n) = both_updates(probe, pose, tot, records=1, prev_rms=rms + 5e-7)
        assert same_bits(s_r, s_n) and same_bits(h_r, h_n)
        assert s_r[12] == T.CONVERGED and s_r[13] == 2 and h_r[1, 15] == T.CONVERGED and same_bits(s_r[:12], pose[:3].reshape(12))


def test_update_rank_deficient(probe):
    tot = plane_totals()
    pose = TC.perturb(np.eye(4)[None], 1)[0]
    (s_r, h_r), (s_n, h_n) = both_updates(probe, pose, tot, damping=0.0)
    assert same_bits(s_r, s_n) and same_bits(h_r, h_n)
    assert s_r[12] == T.DEGENERATE and same_bits(s_r[:12], pose[:3].reshape(12)), "without damping a single plane determines no step"
    (s_r, h_r), (s_n, h_n) = both_updates(probe, pose, tot)
    assert same_bits(s_r, s_n) and same_bits(h_r, h_n)
    assert s_r[12] == T.RUNNING
    step = s_r[[3, 7, 11]] - pose[:3, 3]
    assert step[0] == 0.0 and step[1] == 0.0 and 0.004 < -step[2] < 0.006, "damped: along the normal only, nothing in the plane"
    turn = s_r[:12].reshape(3, 4)[:, :3] @ pose[:3, :3].T
    assert abs(turn[1, 0] - turn[0, 1]) < 1e-15, "and no turn about the normal (4 qw qz of the step's quaternion)"


def test_update_refuses(probe, truth_volume):
    tot, pose = room_totals(truth_volume, 3)
    assert tot[0] > 4000
    for case in ("few", "nan", "inf"):
        bad = tot.copy()
        min_count = 64
        if case == "few":
            min_count = int(tot[0]) + 1
        else:
            bad[5] = np.nan if case == "nan" else np.inf
        (s_r, h_r), (s_n, h_n) = both_updates(probe, pose, bad, min_count=min_count)
        assert same_bits(s_r, s_n) and same_bits(h_r, h_n), case
        assert s_r[12] == T.DEGENERATE and h_r[0, 15] == T.DEGENERATE and same_bits(s_r[:12], pose[:3].reshape(12)), case
    empty = np.zeros(T.TERMS)
    (s_r, h_r), (s_n, h_n) = both_updates(probe, pose, empty)
    assert same_bits(s_r, s_n) and same_bits(h_r, h_n) and s_r[12] == T.DEGENERATE and h_r[0, 14] == 0.0, "no sample: rms 0, not 0 / 0"


def test_retraction_is_a_rotation(probe):
    rng = np.random.default_rng(2)
    for scale in (1e-6, 1e-3, 0.1, 3.0):
        tot = np.zeros(T.TERMS)
        A = rng.normal(size=(12, 6))
        H = A.T @ A
        tot[0] = 100.0
        tot[1:22] = [H[i, j] for i, j in T.PAIRS]
        tot[22:28] = H @ (scale * rng.normal(size=6))
        pose = np.eye(4)[:3].reshape(12).copy()
        want = T.solve(tot, 1e-4, pose)
        assert probe.probe_track_solve(_p(tot), 1e-4, _p(pose)) == 1 and same_bits(pose, want)
        R = pose.reshape(3, 4)[:, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-15 and np.linalg.det(R) > 0.999, scale


def test_restated_tracking_recovers_the_room(truth_volume):
    depths, truth, perturbed, focal = TC.room()
    vol = truth_volume
    poses, states, histories = T.track(vol.tsdf, vol.weight, vol.origin, vol.v, vol.tau, depths, perturbed, focal)
    dt0, dr0 = T.pose_errors(perturbed, truth)
    dt, dr = T.pose_errors(poses, truth)
    used = np.array([min(histories[f, :int(states[f, 13]), 12]) / (depths[f] != 0).sum() for f in range(len(depths))])
    print(f"translation {dt0.mean():.6f} -> mean {dt.mean():.6f} max {dt.max():.6f} m; rotation {dr0.mean():.5f} -> mean {dr.mean():.5f} "
          f"max {dr.max():.5f} deg; pixels used >= {used.min():.4f}; iterations {states[:, 13].min():.0f} .. {states[:, 13].max():.0f}")
    assert dt0.mean() > 0.012 and dr0.mean() > 0.5, "the perturbation is what the issue states"
    assert (states[:, 12] != T.DEGENERATE).all() and used.min() >= TC.MIN_USED
    M, k = TC.MEASURED, TC.HEADROOM
    assert dt.mean() <= k * M["recovery_t_mean"] and dt.max() <= k * M["recovery_t_max"]
    assert dr.mean() <= k * M["recovery_r_mean"] and dr.max() <= k * M["recovery_r_max"]
    # the measured figures are this run's: the bounds have not drifted away from what they were taken from
    assert dt.mean() >= M["recovery_t_mean"] / k and dr.mean() >= M["recovery_r_mean"] / k


def test_restated_rounds_improve_the_room():
    depths, truth, perturbed, focal = TC.room()
    _, rounds = T.refine_poses(TC.ROOM_VOLUME, depths, perturbed, focal, 3)
    rpe = [T.relative_pose_error(perturbed, truth).mean()] + [T.relative_pose_error(p, truth).mean() for p, _, _ in rounds]
    rms_first = [h[:, 0, 14].mean() for _, _, h in rounds]
    rms_last = [s[:, 15].mean() for _, s, _ in rounds]
    print("relative pose error", [f"{v:.6f}" for v in rpe], "rms first", [f"{v:.6f}" for v in rms_first], "last", [f"{v:.6f}" for v in rms_last])
    assert all((s[:, 12] != T.DEGENERATE).all() for _, s, _ in rounds)
    assert all(b < a for a, b in zip(rpe, rpe[1:])) and all(b < a for a, b in zip(rms_last, rms_last[1:]))
    assert all(last < first for first, last in zip(rms_first, rms_last))
    M, k = TC.MEASURED, TC.HEADROOM
    for r in range(3):
        assert rpe[r + 1] <= k * M["round_rpe"][r] and rms_last[r] <= k * M["round_rms"][r], r
        assert rpe[r + 1] >= M["round_rpe"][r] / k and rms_last[r] >= M["round_rms"][r] / k, r


def test_restated_mixed_call():
    """The parity call meets what it is meant to meet."""
    tsdf, weight = TC.analytic_volume()
    m, V = TC.mixed_call(), TC.SMALL_VOLUME
    _, states, histories = T.track(tsdf, weight, V["origin"], V["voxel_size"], V["truncation"], m["depths"], m["poses"], m["focals"],
                                   min_weight=TC.SMALL_MIN_WEIGHT)
    assert [int(s) for s in states[:, 12]] == [T.CONVERGED, T.CONVERGED, T.DEGENERATE, T.DEGENERATE, T.RUNNING, T.CONVERGED]
    assert states[4, 13] == 10 and states[5, 13] < states[1, 13] and (histories[[2, 3], 0, 12] == 0).all()
    assert same_bits(states[2, :12], m["poses"][2, :3].reshape(12))
    count = lambda f, mw: T.terms(tsdf, weight, V["origin"], V["voxel_size"], V["truncation"], m["depths"][f], m["poses"][f, :3],
                                  m["focals"][f], m["depths"][f].shape[1] / 2.0, m["depths"][f].shape[0] / 2.0, min_weight=mw)[:, 0].sum()
    assert count(0, 1.0) == 4800 > count(0, 2.0) > 4000, "voxels of weight 1 lie just below min_weight 2"
    assert 0 < count(4, 2.0) < m["depths"][4].size / 2, "the corner frame straddles the volume's last cells"


def test_sparse_restatement_reads_missing_blocks_as_unknown():
    table = np.array([[[0, -1]], [[5, 1]]], np.int32)                  # [bz=2, by=1, bx=2]; 5 is no slot of two
    store_t = np.stack([np.full((8, 8, 8), 0.25, np.float32), np.full((8, 8, 8), -0.5, np.float32)])
    store_w = np.stack([np.full((8, 8, 8), 3.0, np.float32), np.full((8, 8, 8), 4.0, np.float32)])
    tsdf, weight = T.to_dense(store_t, store_w, table, (13, 7, 16))
    assert tsdf.shape == (16, 7, 13) and (tsdf[:8, :, :8] == 0.25).all() and (weight[8:, :, 8:] == 4.0).all()
    assert (tsdf[:8, :, 8:] == 1.0).all() and (weight[:8, :, 8:] == 0.0).all() and (weight[8:, :, :8] == 0.0).all()
    tsdf, weight = T.to_dense(None, None, table, (13, 7, 16))
    assert (tsdf == 1.0).all() and (weight == 0.0).all()


def test_entry_points_refuse_before_any_launch():
    from acezero_amd import _native as N
    lib = N.lib()
    rows = (N.TsdfFrame * 1)()
    rows[0].m[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    rows[0].focal, rows[0].ppx, rows[0].ppy, rows[0].h, rows[0].w, rows[0].offset = 30.0, 4.0, 3.0, 6, 8, 0
    buf = np.zeros(4096, np.float64)
    p = buf.ctypes.data                                               # never dereferenced: every call below is refused on the host

    def accumulate(**kw):
        a = dict(tsdf=p, weight=p, dims=(8, 8, 8), origin=(0.0, 0.0, 0.0), v=0.02, tau=0.08, depth=p, n_pixels=48, rows=rows, n=1, d_rows=p,
                 depth_unit=0.001, max_depth=4.0, min_weight=1.0, state=p, partials=p)
        a.update(kw)
        return lib.acez_tsdf_track_accumulate(a["tsdf"], a["weight"], *a["dims"], *a["origin"], a["v"], a["tau"], a["depth"], a["n_pixels"],
                                              a["rows"], a["n"], a["d_rows"], 1, a["depth_unit"], a["max_depth"], a["min_weight"], a["state"],
                                              a["partials"], None)

    def accumulate_blocks(**kw):
        a = dict(tsdf=p, weight=p, table=p, slots=p, n_blocks=1, min_weight=1.0, state=p)
        a.update(kw)
        return lib.acez_tsdf_track_accumulate_blocks(a["tsdf"], a["weight"], a["table"], a["slots"], a["n_blocks"], 8, 8, 8, 0.0, 0.0, 0.0, 0.02,
                                                     0.08, p, 48, rows, 1, p, 1, 0.001, 4.0, a["min_weight"], a["state"], p, None)

    def update(**kw):
        a = dict(partials=p, tiles=1, d_rows=p, n=1, rel_rms=1e-6, damping=1e-4, min_count=64, max_iterations=10, state=p, history=p)
        a.update(kw)
        return lib.acez_tsdf_track_update(a["partials"], a["tiles"], a["d_rows"], a["n"], a["rel_rms"], a["damping"], a["min_count"],
                                          a["max_iterations"], a["state"], a["history"], None)

    import torch
    accepted = 0 if torch.cuda.is_available() else -3                 # past the checks: a launch, or "no device"
    if not torch.cuda.is_available():
        assert accumulate() == accepted and accumulate_blocks() == accepted and update() == accepted
    for bad in (dict(tsdf=None), dict(weight=None), dict(depth=None), dict(rows=None), dict(d_rows=None), dict(state=None), dict(partials=None),
                dict(dims=(0, 8, 8)), dict(dims=(2048, 2048, 2048)), dict(v=0.0), dict(v=float("nan")), dict(origin=(0.0, float("inf"), 0.0)),
                dict(tau=0.0), dict(depth_unit=-1.0), dict(max_depth=0.0), dict(min_weight=float("nan")), dict(n=-1), dict(n=257),
                dict(n_pixels=47)):
        assert accumulate(**bad) == -1, bad
    rows[0].focal = 0.0
    assert accumulate() == -1
    rows[0].focal = 30.0
    for bad in (dict(table=None), dict(tsdf=None), dict(slots=None), dict(n_blocks=-1), dict(n_blocks=2), dict(min_weight=0.0), dict(state=None)):
        assert accumulate_blocks(**bad) == -1, bad
    for bad in (dict(partials=None), dict(d_rows=None), dict(state=None), dict(history=None), dict(max_iterations=0), dict(rel_rms=-1e-9),
                dict(rel_rms=float("nan")), dict(damping=-1.0), dict(damping=float("inf")), dict(min_count=5), dict(tiles=-1), dict(n=257)):
        assert update(**bad) == -1, bad
    assert b"min_count" in lib.acez_last_error() or b"frame count" in lib.acez_last_error()


def test_fuse_depth_flags():
    from acezero_amd import cli
    base = ["poses.txt", "rgb/*.png", "out.ply", "--depth_files", "depth/*.png"]
    opt = cli.fuse_depth_parser().parse_args(base)
    assert (opt.refine_poses, opt.refine_iterations, opt.refine_min_weight, opt.refined_pose_file) == (0, 10, 1.0, None)
    opt = cli.fuse_depth_parser().parse_args(base + ["--refine_poses", "2", "--refine_iterations", "6", "--refine_min_weight", "1.5",
                                                     "--refined_pose_file", "refined.txt"])
    assert (opt.refine_poses, opt.refine_iterations, opt.refine_min_weight, str(opt.refined_pose_file)) == (2, 6, 1.5, "refined.txt")


@pytest.mark.parametrize("extra", [["--refined_pose_file", "refined.txt"], ["--refine_poses", "-1"], ["--refine_poses", "1", "--refine_iterations", "0"],
                                   ["--refine_poses", "1", "--refine_min_weight", "0"]],
                         ids=["pose_file_alone", "negative_rounds", "no_iterations", "no_weight"])
def test_fuse_depth_refuses(extra, tmp_path):
    from acezero_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.fuse_depth_main([str(tmp_path / "poses.txt"), str(tmp_path / "*.png"), str(tmp_path / "out.ply"), "--depth_files",
                             str(tmp_path / "depth" / "*.png")] + extra)
    assert e.value.code not in (0, None)
    assert not (tmp_path / "out.ply").exists()
