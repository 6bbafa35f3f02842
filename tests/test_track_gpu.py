"""GPU: the tracking kernels of acezero_amd/csrc/fusion_api.hip (include/acez.h section K3) against the numpy restatement
(tests/track_restated.py) bit for bit: ACCUMULATE's rows of sums, the whole device-resident loop, the block-sparse twin against the
dense kernel, the split into calls; the wide-lens room within the bounds taken from the restatement (tests/track_cases.py); the entry
points' refusals with device buffers; fuse_depth.py --refine_poses end to end."""
import logging
import os
import re

import numpy as np
import pytest
import torch

from tests import fusion_cases as FC
from tests import track_cases as TC
from tests import track_restated as T
from tests.test_track_cpu import same_bits

pytestmark = pytest.mark.gpu


def dense_volume(spec, tsdf=None, weight=None):
    from acezero_amd.fusion import TSDFVolume
    vol = TSDFVolume(spec["origin"], spec["dims"], spec["voxel_size"], spec["truncation"], "cuda")
    if tsdf is not None:
        vol.tsdf.copy_(torch.as_tensor(tsdf))
        vol.weight.copy_(torch.as_tensor(weight))
    return vol


@pytest.fixture(scope="module")
def analytic():
    return dense_volume(TC.SMALL_VOLUME, *TC.analytic_volume())


@pytest.fixture(scope="module")
def mixed_restated():
    """The restated loop on the mixed call, computed once: (poses, states, histories)."""
    tsdf, weight = TC.analytic_volume()
    m, V = TC.mixed_call(), TC.SMALL_VOLUME
    return T.track(tsdf, weight, V["origin"], V["voxel_size"], V["truncation"], m["depths"], m["poses"], m["focals"],
                   min_weight=TC.SMALL_MIN_WEIGHT)


def mixed_track(vol, **kw):
    m = TC.mixed_call()
    return vol.track(m["depths"], m["poses"], m["focals"], min_weight=TC.SMALL_MIN_WEIGHT, **kw)


def test_accumulate_parity(analytic):
    from acezero_amd import _native as N
    from acezero_amd import fusion
    from acezero_amd._device import ptr, stream
    tsdf, weight = TC.analytic_volume()
    m, V = TC.mixed_call(), TC.SMALL_VOLUME
    n = len(m["depths"])
    (d_depth, _, rows, d_rows, k), = fusion.calls(m["depths"], None, m["poses"], m["focals"], None, None, None, 64, analytic.device)
    assert k == n
    tiles = max((d.size + 255) // 256 for d in m["depths"])
    state_h = np.zeros((n, T.STATE))
    state_h[:, :12] = m["poses"][:, :3].reshape(n, 12)
    state_h[5, 12] = T.CONVERGED                                      # a frame that has stopped: its workgroups write nothing
    state = torch.from_numpy(state_h).cuda()
    partials = torch.full((n, tiles, T.TERMS), -7.0, dtype=torch.float64, device="cuda")
    analytic._track_accumulate(ptr(d_depth), d_depth.numel(), rows, n, ptr(d_rows), 1, 0.001, 4.0, TC.SMALL_MIN_WEIGHT, ptr(state), ptr(partials),
                               stream())
    got = partials.cpu().numpy()
    assert same_bits(state.cpu().numpy(), state_h), "ACCUMULATE does not write the state"
    for f in range(n):
        h, w = m["depths"][f].shape
        own = (h * w + 255) // 256
        assert (got[f, own:] == -7.0).all(), f"frame {f}: tiles past its own count are not written"
        if f == 5:
            assert (got[f] == -7.0).all()
            continue
        want = T.block_sums(T.terms(tsdf, weight, V["origin"], V["voxel_size"], V["truncation"], m["depths"][f], m["poses"][f, :3], m["focals"][f],
                                    w / 2.0, h / 2.0, min_weight=TC.SMALL_MIN_WEIGHT))
        print(f"frame {f}: {h} x {w}, {own} tiles, {int(want[:, 0].sum())} samples")
        assert same_bits(got[f, :own], want), f
    counts = got[:, :, 0].clip(0).sum(1)
    assert counts[0] > 4000 and counts[1] > 2000 and counts[2] == 0 and counts[3] == 0 and 0 < counts[4] < 384


def test_loop_parity(analytic, mixed_restated):
    want_poses, want_states, want_hist = mixed_restated
    poses, info, hist = mixed_track(analytic)
    assert same_bits(hist, want_hist) and same_bits(poses[:, :3], want_poses[:, :3])
    assert [i["status"] for i in info] == [T.STATUS[int(s)] for s in want_states[:, 12]]
    assert [i["iterations"] for i in info] == [int(s) for s in want_states[:, 13]]
    assert [i["status"] for i in info] == ["converged", "converged", "degenerate", "degenerate", "max_iterations", "converged"]
    m = TC.mixed_call()
    for f, i in enumerate(info):
        assert (hist[f, i["iterations"]:] == 0.0).all(), "a frame that has stopped is passed over by the later pairs"
        assert i["count_first"] == want_hist[f, 0, 12] and i["rms_last"] == want_hist[f, i["iterations"] - 1, 14]
    assert info[5]["iterations"] < 10 and info[2]["iterations"] == 1 and info[2]["count_first"] == 0
    assert same_bits(poses[2], m["poses"][2]) and same_bits(poses[3], m["poses"][3]), "a degenerate frame keeps its input pose"


@pytest.mark.parametrize("frames_per_call", [1, 5])
def test_calls_do_not_matter(analytic, mixed_restated, frames_per_call):
    want_poses, _, want_hist = mixed_restated                           # test_loop_parity holds frames_per_call 64 to the same bits
    poses, _, hist = mixed_track(analytic, frames_per_call=frames_per_call)
    assert same_bits(hist, want_hist) and same_bits(poses[:, :3], want_poses[:, :3])


def test_sparse_equals_dense():
    from acezero_amd.fusion import SparseTSDFVolume
    s, V = TC.sparse_scene(), TC.SMALL_VOLUME
    sparse = SparseTSDFVolume(V["origin"], V["dims"], V["voxel_size"], V["truncation"], "cuda")
    fused = dict(cam_to_world=s["truth"][:10], focals=s["focal"])
    sparse.mark(s["depths"][:10], **fused)
    n_blocks = sparse.allocate()
    grid = sparse.grid[0] * sparse.grid[1] * sparse.grid[2]
    assert 0 < n_blocks < grid, "the room's middle has no block"
    sparse.integrate(s["depths"][:10], **fused)
    tsdf, weight, _ = sparse.to_dense()
    dense = dense_volume(V, tsdf, weight)
    got = sparse.track(s["depths"], s["poses"], s["focal"])
    want = dense.track(s["depths"], s["poses"], s["focal"])
    assert same_bits(got[2], want[2]) and same_bits(got[0], want[0]) and got[1] == want[1]
    # and both are the restatement's, on the sparse storage read the way to_dense() reads it
    r_tsdf, r_weight = T.to_dense(sparse.tsdf.cpu().numpy(), sparse.weight.cpu().numpy(), sparse.block_table.cpu().numpy(), V["dims"])
    assert same_bits(r_tsdf, tsdf.cpu().numpy()) and same_bits(r_weight, weight.cpu().numpy())
    r_poses, r_states, r_hist = T.track(r_tsdf, r_weight, V["origin"], V["voxel_size"], V["truncation"], s["depths"], s["poses"], s["focal"])
    assert same_bits(got[2], r_hist) and same_bits(got[0][:, :3], r_poses[:, :3])
    assert all(i["status"] != "degenerate" and i["count_last"] > 600 for i in got[1][:10])
    dt0, dt = T.pose_errors(s["poses"][:10], s["truth"][:10])[0], T.pose_errors(got[0][:10], s["truth"][:10])[0]
    assert dt.mean() < 0.5 * dt0.mean()
    # the last frame's points float in the room's middle, where a block has no slot: a corner there is unknown
    # in the densely fused volume those voxels are known, and some of them lie near enough to a wall to give samples
    assert sparse.block_table.cpu().numpy()[1, 1, 1] == -1
    full = dense_volume(V).integrate(s["depths"][:10], **fused)
    _, info_full, _ = full.track(s["depths"][10:], s["poses"][10:], s["focal"], max_iterations=1)
    print("the floating frame's samples: sparse", got[1][10]["count_first"], "densely fused", info_full[0]["count_first"])
    assert got[1][10]["count_first"] < info_full[0]["count_first"]
    # a volume without any block: every frame is degenerate, nothing is read
    empty = SparseTSDFVolume(V["origin"], V["dims"], V["voxel_size"], V["truncation"], "cuda")
    assert empty.allocate() == 0
    poses, info, _ = empty.track(s["depths"][:2], s["poses"][:2], s["focal"])
    assert [i["status"] for i in info] == ["degenerate"] * 2 and same_bits(poses, s["poses"][:2])


@pytest.fixture(scope="module")
def room_volume():
    depths, truth, _, focal = TC.room()
    V = TC.ROOM_VOLUME
    return dense_volume(V).integrate(depths, cam_to_world=truth, focals=focal)


def test_room_recovery(room_volume):
    depths, truth, perturbed, focal = TC.room()
    poses, info, hist = room_volume.track(depths, perturbed, focal)
    dt, dr = T.pose_errors(poses, truth)
    used = np.array([min(hist[f, :i["iterations"], 12]) / (depths[f] != 0).sum() for f, i in enumerate(info)])
    print(f"translation mean {dt.mean():.6f} max {dt.max():.6f} m; rotation mean {dr.mean():.5f} max {dr.max():.5f} deg; pixels used >= "
          f"{used.min():.4f}; iterations {min(i['iterations'] for i in info)} .. {max(i['iterations'] for i in info)}")
    assert all(i["status"] != "degenerate" for i in info) and used.min() >= TC.MIN_USED
    M, k = TC.MEASURED, TC.HEADROOM
    assert dt.mean() <= k * M["recovery_t_mean"] and dt.max() <= k * M["recovery_t_max"]
    assert dr.mean() <= k * M["recovery_r_mean"] and dr.max() <= k * M["recovery_r_max"]


def test_room_rounds():
    from acezero_amd import fusion
    depths, truth, perturbed, focal = TC.room()
    vol, poses, rounds = fusion.refine_poses(lambda: dense_volume(TC.ROOM_VOLUME), depths, perturbed, focal, rounds=3)
    rpe = [T.relative_pose_error(perturbed, truth).mean()] + [T.relative_pose_error(r["poses"], truth).mean() for r in rounds]
    rms = [r["rms_after"] for r in rounds]
    print("relative pose error", [f"{v:.6f}" for v in rpe], "rms", [(f"{r['rms_before']:.6f}", f"{r['rms_after']:.6f}") for r in rounds])
    assert all(r["degenerate"] == 0 and r["converged"] + r["out_of_iterations"] == len(depths) for r in rounds)
    assert all(b < a for a, b in zip(rpe, rpe[1:])) and all(b < a for a, b in zip(rms, rms[1:]))
    assert all(r["rms_after"] < r["rms_before"] for r in rounds)
    M, k = TC.MEASURED, TC.HEADROOM
    for r in range(3):
        assert rpe[r + 1] <= k * M["round_rpe"][r] and rms[r] <= k * M["round_rms"][r], r
    assert same_bits(poses, rounds[-1]["poses"]) and vol.frames_fused == len(depths)


def test_room_rounds_on_the_sparse_volume():
    """refine_poses marks and allocates a fresh sparse volume every round. The sparse volume holds the dense one's bits where it has
    blocks, and MARK gives blocks to everything from the surface to a truncation behind it and a voxel around that, so tracking loses
    only the samples whose cell reaches into a block before the surface that nothing marked: the figures are not the dense ones, and
    what is asserted is what any working round must give on this room -- no frame degenerate, most pixels used, the residual and the
    relative pose error falling every round, the latter to under half after the first (the dense volume: to a quarter)."""
    from acezero_amd import fusion
    depths, truth, perturbed, focal = TC.room()
    V = TC.ROOM_VOLUME
    seen = []

    def make_volume():
        seen.append(fusion.SparseTSDFVolume(V["origin"], V["dims"], V["voxel_size"], V["truncation"], "cuda"))
        return seen[-1]

    vol, poses, rounds = fusion.refine_poses(make_volume, depths, perturbed, focal, rounds=2)
    rpe = [T.relative_pose_error(perturbed, truth).mean()] + [T.relative_pose_error(r["poses"], truth).mean() for r in rounds]
    print("relative pose error", [f"{v:.6f}" for v in rpe], "rms", [(f"{r['rms_before']:.6f}", f"{r['rms_after']:.6f}") for r in rounds],
          "pixels", [r["pixels"] for r in rounds], "blocks", [v.allocated_blocks for v in seen])
    assert len(seen) == 3 and vol is seen[-1] and all(v.allocated_blocks > 0 for v in seen) and vol.frames_fused == len(depths)
    assert all(r["degenerate"] == 0 and r["pixels"] >= TC.MIN_USED * TC.ROOM_H * TC.ROOM_W for r in rounds)
    assert rpe[1] < 0.5 * rpe[0] and rpe[2] < rpe[1]
    assert all(r["rms_after"] < r["rms_before"] for r in rounds) and rounds[1]["rms_after"] < rounds[0]["rms_after"]


def test_entry_points_refuse_with_device_buffers(analytic):
    from acezero_amd import _native as N
    from acezero_amd import fusion
    from acezero_amd._device import ptr, stream
    m = TC.mixed_call()
    (d_depth, _, rows, d_rows, n), = fusion.calls(m["depths"], None, m["poses"], m["focals"], None, None, None, 64, analytic.device)
    state_h = np.zeros((n, T.STATE))
    state_h[:, :12] = m["poses"][:, :3].reshape(n, 12)
    state = torch.from_numpy(state_h).cuda()
    partials = torch.full((n, 19, T.TERMS), -7.0, dtype=torch.float64, device="cuda")
    history = torch.full((n, 10, T.RECORD), -7.0, dtype=torch.float64, device="cuda")
    lib = N.lib()

    def accumulate(v=0.02, tau=0.08, n_pixels=d_depth.numel(), min_weight=2.0, st=ptr(state), dims=analytic.dims):
        return lib.acez_tsdf_track_accumulate(ptr(analytic.tsdf), ptr(analytic.weight), *dims, *analytic.origin, v, tau, ptr(d_depth), n_pixels, rows, n,
                                              ptr(d_rows), 1, 0.001, 4.0, min_weight, st, ptr(partials), stream())

    def update(rel_rms=1e-6, damping=1e-4, min_count=64, max_iterations=10, hist=ptr(history)):
        return lib.acez_tsdf_track_update(ptr(partials), 19, ptr(d_rows), n, rel_rms, damping, min_count, max_iterations, ptr(state), hist, stream())

    assert accumulate(v=0.0) == -1 and accumulate(tau=-1.0) == -1 and accumulate(n_pixels=d_depth.numel() - 1) == -1
    assert accumulate(min_weight=float("inf")) == -1 and accumulate(st=None) == -1 and accumulate(dims=(24, 0, 28)) == -1
    assert update(rel_rms=-1.0) == -1 and update(damping=float("nan")) == -1 and update(min_count=5) == -1 and update(max_iterations=0) == -1
    assert update(hist=None) == -1
    assert lib.acez_tsdf_track_accumulate_blocks(ptr(analytic.tsdf), ptr(analytic.weight), None, None, 0, *analytic.dims, *analytic.origin, 0.02, 0.08,
                                                 ptr(d_depth), d_depth.numel(), rows, n, ptr(d_rows), 1, 0.001, 4.0, 2.0, ptr(state), ptr(partials),
                                                 stream()) == -1
    with pytest.raises(N.AcezError, match="ACEZ_ERR_INVALID"):
        N.check(update(min_count=0))
    torch.cuda.synchronize()
    assert (partials == -7.0).all() and (history == -7.0).all() and same_bits(state.cpu().numpy(), state_h), "nothing was launched"
    with pytest.raises(ValueError):
        analytic.track(m["depths"], m["poses"], m["focals"], max_iterations=0)


def test_fuse_depth_refines_end_to_end(tmp_path, caplog):
    from acezero_amd import cli, formats, fusion
    from acezero_amd.session import write_pose_file
    n, h, w, focal = TC.ROOM_FRAMES, TC.ROOM_H, TC.ROOM_W, TC.ROOM_FOCAL
    args = FC.write_room_scene(tmp_path, n, h, w, focal)
    truth = FC.room_cameras(n)
    perturbed = TC.perturb(truth, 11)
    names = [str(tmp_path / f"frame_{k:03d}.png") for k in range(n)]
    write_pose_file(args[0], names, perturbed, [5000 + k for k in range(n)], 2 * focal)
    # without the new flags: the bytes of integrate + extract_mesh + write_ply on the same inputs, the command's whole function before
    plain = str(tmp_path / "plain.ply")
    assert cli.fuse_depth_main(args[:2] + [plain] + args[3:]) == 0
    entries = formats.read_pose_file(args[0])
    c2w = np.stack([np.linalg.inv(e.w2c) for e in entries])
    depths = [formats.read_depth_png(str(tmp_path / "depth" / f"frame_{k:03d}.png")) for k in range(n)]
    from PIL import Image
    rgb = [np.ascontiguousarray(np.asarray(Image.open(f).convert("RGB").resize((w, h), Image.NEAREST), np.uint8)) for f in names]
    origin, dims = fusion.bounds_from_frames(depths, c2w, np.full(n, focal), 0.02, 0.08)
    vol = fusion.TSDFVolume(origin, dims, 0.02, 0.08, "cuda").integrate(depths, cam_to_world=c2w, focals=np.full(n, focal), rgb=rgb)
    v, c, f = (a.cpu() for a in vol.extract_mesh(2))
    formats.write_ply(str(tmp_path / "want.ply"), v, c, f)
    assert open(plain, "rb").read() == open(tmp_path / "want.ply", "rb").read()
    # with them
    refined, pose_out = str(tmp_path / "refined.ply"), str(tmp_path / "refined.txt")
    with caplog.at_level(logging.INFO):
        assert cli.fuse_depth_main(args[:2] + [refined] + args[3:] + ["--refine_poses", "2", "--refined_pose_file", pose_out]) == 0
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Pose refinement round")]
    assert len(lines) == 2
    rms = [[float(x) for x in re.search(r"residual ([0-9.]+) -> ([0-9.]+) mm", line).groups()] for line in lines]
    print(lines)
    assert rms[0][1] < rms[0][0] and rms[1][1] < rms[0][1] and "0 degenerate" in lines[0]
    out = formats.read_pose_file(pose_out)
    assert [e.file for e in out] == [e.file for e in entries] and [e.focal for e in out] == [e.focal for e in entries]
    assert [e.confidence_text for e in out] == [e.confidence_text for e in entries]
    got = np.stack([np.linalg.inv(e.w2c) for e in out])
    assert T.relative_pose_error(got, truth).mean() < 0.5 * T.relative_pose_error(perturbed, truth).mean()
    before = FC.wall_distance(FC.read_mesh_ply(plain)[0]).mean()
    after = FC.wall_distance(FC.read_mesh_ply(refined)[0]).mean()
    print(f"mean wall distance {before:.6f} -> {after:.6f} m")
    assert after <= before
