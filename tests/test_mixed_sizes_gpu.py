"""Folders of mixed frame sizes on the GPU: the table-driven buffer sampler against the one-size sampler (bitwise), then ace_zero.py,
train_ace.py + register_mapping.py and export on a synthetic room whose every third frame is rendered portrait."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from acezero_amd import _native as N
from acezero_amd import synth

pytestmark = pytest.mark.gpu

CH, S = 512, 1024


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _outs(n_views):
    dev = "cuda"
    return (torch.full((n_views * S, CH), 0x7fff, dtype=torch.int16, device=dev), torch.full((n_views * S, 2), -1.0, device=dev),
            torch.full((n_views * S,), -1, dtype=torch.int32, device=dev), torch.full((n_views * S,), -1, dtype=torch.int32, device=dev))


def _old(feat, mask, n_views, oh, ow, seed, first_view_id, base, outs):
    N.check(N.lib().acez_buffer_sample_views(_p(feat), _p(mask), n_views, oh, ow, CH, S, C.c_uint64(seed), C.c_uint64(first_view_id), base,
                                             *[_p(t) for t in outs], None))


def _new(store, mask, table, seed, first_view_id, base, outs):
    t = torch.as_tensor(np.asarray(table, np.int64)).to("cuda")
    max_hw = int((t[:, 1] * t[:, 2]).max())
    N.check(N.lib().acez_buffer_sample_views_table(_p(store), store.shape[0], _p(mask), mask.numel() if mask is not None else 0, _p(t), t.shape[0],
                                                   max_hw, CH, S, C.c_uint64(seed), C.c_uint64(first_view_id), base, *[_p(x) for x in outs], None))


@pytest.mark.parametrize("masked", [False, True])
def test_table_sampler_equals_one_size_sampler(masked):
    """One size: every output of the table entry point (features, target pixels, view indices, pixel ids) equals the one-size entry
    point's, view for view, including the views of a partial last pass (fewer views than images)."""
    g = torch.Generator().manual_seed(3)
    n, oh, ow = 7, 30, 40
    hw = oh * ow
    store = torch.randint(-30000, 30000, (n * hw + 5 * hw, CH), generator=g, dtype=torch.int16).cuda()   # resident store, frames in any order
    slot = [3, 0, 6, 1, 5, 2, 4]                                         # view v's map lives at slot[v]
    mask = (torch.rand(n, hw, generator=g) > 0.6).to(torch.uint8).cuda() if masked else None
    for v_count, fid in ((n, 0), (3, 1234567)):                        # a full pass, then a partial last one
        gathered = store[torch.tensor([s * hw + p for s in slot[:v_count] for p in range(hw)]).cuda()].contiguous()
        a, b = _outs(v_count), _outs(v_count)
        _old(gathered, mask[:v_count].contiguous() if masked else None, v_count, oh, ow, 2089, fid, 11, a)
        _new(store, mask, [(slot[v] * hw, oh, ow, v * hw if masked else -1) for v in range(v_count)], 2089, fid, 11, b)
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_table_sampler_mixed_views_equal_per_class_calls():
    """Views of three sizes interleaved in ONE launch: each view's rows equal the one-size entry point's on that view alone, called
    with first_view_id + v and view index base + v."""
    g = torch.Generator().manual_seed(4)
    shapes = [(30, 40), (40, 30), (30, 50), (30, 40), (40, 30), (30, 40)]
    hws = [h * w for h, w in shapes]
    rows = np.concatenate([[0], np.cumsum(hws)])
    store = torch.randint(-30000, 30000, (int(rows[-1]), CH), generator=g, dtype=torch.int16).cuda()
    mask = (torch.rand(int(rows[-1]), generator=g) > 0.5).to(torch.uint8).cuda()
    for masked in (False, True):
        table = [(int(rows[v]), h, w, int(rows[v]) if masked else -1) for v, (h, w) in enumerate(shapes)]
        b = _outs(len(shapes))
        _new(store, mask if masked else None, table, 77, 500, 3, b)
        a = _outs(len(shapes))
        for v, (h, w) in enumerate(shapes):
            sl = [t[v * S:(v + 1) * S] for t in a]
            _old(store[rows[v]:rows[v + 1]], mask[rows[v]:rows[v + 1]] if masked else None, 1, h, w, 77, 500 + v, 3 + v, sl)
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_fill_buffer_of_one_size_equals_gathered_sampling():
    """ReconstructionSession._fill_buffer (table sampler on the resident store) against the former gathered-copy path on the same
    session, with depth masks and a partial last view: identical buffers."""
    from acezero_amd.session import ReconstructionSession, default_options
    from acezero_amd.head import _ptr, _stream
    seq = synth.render_room_sequence(seed=3, n_frames=6, h=240, w=320, device="cuda")
    esd = {k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}
    o = default_options(use_aug=False, use_external_focal_length=seq["focal"], max_dataset_passes=3, samples_per_image=256)
    ses = ReconstructionSession(esd, seq["images"], opt=o, depth=seq["depth"])
    ids = [4, 1, 3]
    total = 3 * 3 * 256 - 100
    poses = seq["poses"][ids].cpu()
    buf = ses._fill_buffer(ids, poses, seq["focal"], True, total=total)
    # the former path: one gathered copy of the mapped maps, acez_buffer_sample_views per pass
    feats3 = ses.features.view(ses.n, ses.hw, -1)
    src = feats3[torch.tensor(ids).cuda()].reshape(-1, feats3.shape[2])
    d = ses.depth[torch.tensor(ids).cuda()]
    mask = ((d > 0) & (d <= 1000)).to(torch.uint8).reshape(3, ses.hw).contiguous()
    f = torch.empty((4 * 3 * 256, src.shape[1]), dtype=src.dtype, device="cuda")
    px = torch.empty((4 * 3 * 256, 2), device="cuda")
    vi = torch.empty((4 * 3 * 256,), dtype=torch.int32, device="cuda")
    pix = torch.empty((4 * 3 * 256,), dtype=torch.int32, device="cuda")
    filled, n_views = 0, 0
    vs = 0
    while filled < total:
        v = min(3, (total - filled + 255) // 256)
        sl = slice(n_views * 256, (n_views + v) * 256)
        N.check(N.lib().acez_buffer_sample_views(_ptr(src), _ptr(mask), v, ses.oh, ses.ow, src.shape[1], 256, o.base_seed + 4095, vs, n_views,
                                                 _ptr(f[sl]), _ptr(px[sl]), _ptr(vi[sl]), _ptr(pix[sl]), _stream()))
        filled += min(v * 256, total - filled)
        n_views += v
        vs += v
    torch.cuda.synchronize()
    assert buf["features"].shape[0] == total
    assert torch.equal(buf["features"], f[:total]) and torch.equal(buf["target_px"], px[:total]) and torch.equal(buf["view_idx"], vi[:total])
    K = ses._K(seq["focal"])
    assert torch.equal(buf["view_K"], K.repeat(n_views, 1, 1)) and torch.equal(buf["view_Kinv"], torch.linalg.inv(K).repeat(n_views, 1, 1))
    img = vi[:total].long() % 3
    dd = d.reshape(3, ses.hw)[img, pix[:total].long()]
    eye = torch.stack([(px[:total, 0] - ses.ppx) / seq["focal"] * dd, (px[:total, 1] - ses.ppy) / seq["focal"] * dd, dd, torch.ones_like(dd)], dim=1)
    want = torch.einsum("nij,nj->ni", poses.to("cuda", torch.float32)[img][:, :3], eye)
    assert torch.equal(buf["target_crds"], want)


# ------------------------------------------------------------------------------------------------------------------ end to end
def _pose_err(est, gt):
    dt = np.linalg.norm(est[:, :3, 3] - gt[:, :3, 3], axis=1)
    R = np.einsum("nij,nkj->nik", est[:, :3, :3], gt[:, :3, :3])
    ang = np.degrees(np.arccos(np.clip((np.trace(R, axis1=1, axis2=2) - 1) / 2, -1, 1)))
    return dt, ang


def _align_similarity(est, gt):
    a, b = est[:, :3, 3], gt[:, :3, 3]
    ma, mb = a.mean(0), b.mean(0)
    H = (b - mb).T @ (a - ma) / len(a)
    U, S_, Vt = np.linalg.svd(H)
    D = np.diag([1, 1, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ D @ Vt
    s = np.trace(np.diag(S_) @ D) / ((a - ma) ** 2).sum(1).mean()
    out = est.copy()
    out[:, :3, :3] = R @ est[:, :3, :3]
    out[:, :3, 3] = (s * (R @ (a - ma).T)).T + mb
    return out, s


def _mixed_room(tmp_path, seed, n, arc, portrait=lambda i: i % 3 == 2, depth=True):
    """PNG frames of a synthetic room (480 x 640, and 640 x 480 where `portrait(i)`, same focal), 16-bit depth, encoder weights."""
    from PIL import Image
    seq = synth.render_room_sequence(seed=seed, n_frames=n, arc_deg=arc, device="cuda")
    por = synth.render_room_sequence(seed=seed, n_frames=n, arc_deg=arc, h=640, w=480, focal=seq["focal"], device="cuda", pose_override=seq["poses"])
    files = []
    for i in range(n):
        s = por if portrait(i) else seq
        img = ((s["images"][i, 0] * 0.25 + 0.4).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
        files.append(str(tmp_path / f"rgb_{i:04d}.png"))
        Image.fromarray(np.stack([img] * 3, -1)).save(files[-1])
        if depth:
            dep = (s["depth"][i].cpu().numpy() * 1000).round().astype(np.uint16)
            Image.fromarray(np.kron(dep, np.ones((8, 8), np.uint16))).save(tmp_path / f"depth_{i:04d}.png")
    torch.save({k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}, tmp_path / "encoder.pt")
    return seq, files


def test_ace_zero_on_mixed_portrait_and_landscape_frames(tmp_path):
    from acezero_amd import cli
    seq, files = _mixed_room(tmp_path, 7, 48, 24.0)
    out = tmp_path / "result"
    it = "2500"
    rc = cli.ace_zero_main([str(tmp_path / "rgb_*.png"), str(out), "--depth_files", str(tmp_path / "depth_*.png"), "--encoder_path",
                            str(tmp_path / "encoder.pt"), "--use_external_focal_length", str(seq["focal"]), "--try_seeds", "1",
                            "--seed_iterations", it, "--refit_iterations", it, "--final_refit_posewait", "500", "--cooldown_iterations", "500",
                            "--iterations_max", "6", "--aug_rotation", "2", "--export_point_cloud", "True"])
    assert rc == 0
    final = [line.split() for line in open(out / "poses_final.txt").read().splitlines()]
    assert [r[0] for r in final] == sorted(files)
    conf = np.array([float(r[-1]) for r in final])
    por = np.array([i % 3 == 2 for i in range(48)])
    assert (conf > 500).mean() >= 0.9 and (conf[por] > 500).mean() >= 0.9
    fl, poses, focals = cli.read_ace_pose_file(out / "poses_final.txt", 500)
    idx = [files.index(f) for f in fl]
    gt = seq["poses"].cpu().numpy().astype(np.float64)
    aligned, scale = _align_similarity(poses, gt[idx])
    dt, _ = _pose_err(aligned, gt[idx])
    # the pose-error bounds of test_session_gpu.py's ACE0 loop. Its metric-scale bound (0.8 .. 1.25) is asserted on that test's longer,
    # wider sequence below (test_ace_zero_loop_on_mixed_frames_keeps_the_metric_scale); on this short 24-degree arc the scale is pinned
    # loosely for any folder (a portrait-only folder, which takes the one-size path, ends at 0.84; this mix at 0.62)
    assert 0.5 < scale < 2.0 and np.median(dt) < 0.05
    rel = np.einsum("nij,njk->nik", np.linalg.inv(poses[:-1]), poses[1:])
    rel_gt = np.einsum("nij,njk->nik", np.linalg.inv(gt[idx][:-1]), gt[idx][1:])
    assert np.median(_pose_err(rel, rel_gt)[1]) < 0.5                   # frame-to-frame rotations
    assert np.allclose(focals, focals[0])                                # one focal, refined (portrait and landscape share it)
    assert open(out / "pc_final.ply", "rb").read(200).startswith(b"ply\nformat binary_little_endian")


def test_train_and_register_on_mixed_frames(tmp_path):
    """train_ace.py --pose_files on the mixed folder, then register_mapping.py; the 80-column-wider frame is a class of one."""
    from PIL import Image
    from acezero_amd import cli
    seq, files = _mixed_room(tmp_path, 11, 40, 20.0, depth=False)
    gt = seq["poses"].cpu().numpy().astype(np.float64)
    wide = synth.render_room_sequence(seed=11, n_frames=1, arc_deg=20.0, h=480, w=720, focal=seq["focal"], device="cuda",
                                      pose_override=seq["poses"][5:6])
    img = ((wide["images"][0, 0] * 0.25 + 0.4).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
    Image.fromarray(np.stack([img] * 3, -1)).save(files[5])              # frame 5: 480 x 720, alone in its size class
    for i in range(len(files)):
        np.savetxt(tmp_path / f"pose_{i:04d}.txt", gt[i])
    out = tmp_path / "map" / "scene.pt"
    rc = cli.train_main([str(tmp_path / "rgb_*.png"), str(out), "--pose_files", str(tmp_path / "pose_*.txt"), "--encoder_path",
                         str(tmp_path / "encoder.pt"), "--use_external_focal_length", str(seq["focal"]), "--iterations", "2500",
                         "--learning_rate_cooldown_iterations", "500", "--aug_rotation", "2", "--aug_scale", "1.06"])
    assert rc == 0 and out.exists()
    fl, _, focals = cli.read_ace_pose_file(tmp_path / "map" / "poses_scene_preliminary.txt", 0)
    assert fl == sorted(files) and np.allclose(focals, seq["focal"])    # every written focal in its frame's original units
    rc = cli.register_main([str(tmp_path / "rgb_*.png"), str(out), "--encoder_path", str(tmp_path / "encoder.pt"), "--session", "query",
                            "--use_external_focal_length", str(seq["focal"]), "--hypotheses", "32", "--hypotheses_max_tries", "16"])
    assert rc == 0
    fl, poses, focals = cli.read_ace_pose_file(tmp_path / "map" / "poses_query.txt", 500)
    assert len(fl) >= 38 and np.allclose(focals, seq["focal"]) and files[5] in fl
    idx = [files.index(f) for f in fl]
    dt, ang = _pose_err(poses, gt[idx])
    assert np.median(dt) < 0.01 and np.median(ang) < 0.5
    # export_point_cloud.py on the mixed pose file
    rc = cli.export_point_cloud_main([str(tmp_path / "pc.txt"), "--network", str(out), "--pose_file", str(tmp_path / "map" / "poses_query.txt"),
                                      "--encoder_path", str(tmp_path / "encoder.pt"), "--convention", "opencv"])
    assert rc == 0
    pts = np.loadtxt(tmp_path / "pc.txt")
    assert pts.shape[1] == 6 and len(pts) > 1000 and np.allclose(pts[:, 3], pts[:, 4])


def test_ace_zero_loop_on_mixed_frames_keeps_the_metric_scale():
    """test_session_gpu.py's ACE0 loop (same sequence, options and bounds) with every third frame portrait: the metric scale still comes
    from the seed's depth, focal and principal point, now per frame."""
    from acezero_amd.session import ReconstructionSession, default_options
    seq = synth.render_room_sequence(seed=2089, n_frames=72, arc_deg=36.0, device="cuda")
    tall = synth.render_room_sequence(seed=2089, n_frames=72, arc_deg=36.0, h=640, w=480, focal=seq["focal"], device="cuda",
                                      pose_override=seq["poses"])
    esd = {k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}
    por = np.arange(2, 72, 3)
    land = np.setdiff1d(np.arange(72), por)
    images = [(land, seq["images"][land]), (por, tall["images"][por])]
    depth = [(tall if i % 3 == 2 else seq)["depth"][i] for i in range(72)]
    it = 3000
    opt = default_options(use_external_focal_length=seq["focal"], try_seeds=2, seed_iterations=it, iterations=it, refit_iterations=it,
                          iterations_max=8, final_refit_posewait=it // 5, learning_rate_warmup_iterations=it // 5, cooldown_iterations=it // 5,
                          aug_rotation=2, aug_scale=1.06, aug_black_white=0.02)
    ses = ReconstructionSession(esd, images, opt=opt, depth=depth)
    assert len(ses.classes) == 2
    res = ses.reconstruct()
    rates = [h["registration_rate"] for h in res["history"]]
    assert rates[-1] >= 0.97 and (res["confidence"][por] > 500).mean() >= 0.9
    ok = res["confidence"] > opt.registration_confidence
    gt = seq["poses"].cpu().numpy().astype(np.float64)
    aligned, scale = _align_similarity(res["poses"][ok].astype(np.float64), gt[ok])
    dt, _ = _pose_err(aligned, gt[ok])
    assert 0.8 < scale < 1.25, scale                                     # metric scale comes from the seed's depth
    assert np.median(dt) < 0.05, np.median(dt)
    rel = np.einsum("nij,njk->nik", np.linalg.inv(res["poses"][ok][:-1].astype(np.float64)), res["poses"][ok][1:].astype(np.float64))
    rel_gt = np.einsum("nij,njk->nik", np.linalg.inv(gt[ok][:-1]), gt[ok][1:])
    assert np.median(_pose_err(rel, rel_gt)[1]) < 0.5


def test_augmented_fill_of_one_size_keeps_its_intrinsics_bitwise():
    """A folder of one size: the augmented fill's per-view K and K^-1 are the float32 matrices built from the Python-float focal
    focal * hs / H and inverted in float32 -- exactly as before size classes existed."""
    from acezero_amd.session import ReconstructionSession, default_options
    seq = synth.render_room_sequence(seed=3, n_frames=4, device="cuda")
    esd = {k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}
    for with_depth in (False, True):
        ses = ReconstructionSession(esd, seq["images"], opt=default_options(use_external_focal_length=seq["focal"]), depth=seq["depth"])
        ids = [2] if with_depth else [0, 1, 2, 3]
        buf = ses._fill_buffer_augmented(ids, seq["poses"][ids].cpu(), seq["focal"], with_depth, total=len(ids) * 1024 * 10)
        K, Kinv = buf["view_K"], buf["view_Kinv"]
        assert K.dtype == torch.float32 and Kinv.dtype == torch.float32 and len(K) == len(ids) * 10
        for v in range(len(K)):
            hs, ws = round(float(K[v, 1, 2]) * 2), round(float(K[v, 0, 2]) * 2)
            f = seq["focal"] * (hs / ses.H)
            want = torch.tensor([[f, 0, ws / 2.0], [0, f, hs / 2.0], [0, 0, 1.0]])
            assert torch.equal(K[v], want) and torch.equal(Kinv[v], torch.linalg.inv(want)), v


def test_point_cloud_streams_are_keyed_by_registered_position():
    """On a mixed folder every frame's point selection is the filter's on that frame alone, keyed by its position among the registered
    frames -- not by where its size class puts it. 240 frames of 4800 map pixels: more points than points_per_image allows per frame,
    so every frame goes through the random sub-sampling branch (ace_vis_util.py:545-551)."""
    from acezero_amd.pointcloud import filter_scene_coordinates
    from acezero_amd.session import ReconstructionSession, default_options
    from acezero_amd.head import HeadTrainer
    n = 240
    g = torch.Generator().manual_seed(6)
    por = np.arange(2, n, 3)
    land = np.setdiff1d(np.arange(n), por)
    images = [(land, torch.randn(len(land), 1, 480, 640, generator=g)), (por, torch.randn(len(por), 1, 640, 480, generator=g))]
    esd = {k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}
    ses = ReconstructionSession(esd, images, opt=default_options(use_external_focal_length=500.0, use_aug=False))
    tr = HeadTrainer(torch.zeros(3), max_batch=5120, iterations=1)
    tr.load_flat((torch.rand(tr.n_params, generator=torch.Generator().manual_seed(1)) * 2 - 1) / 22.6)
    head = {k: v.detach().cpu().half() for k, v in tr.state_dict().items()}
    tr.close()
    poses = np.tile(np.eye(4), (n, 1, 1))
    conf = np.full(n, 1000)
    conf[4] = 0                                                          # one frame not registered: the later positions shift
    xyz, src, sel = ses.point_cloud(head, poses, conf, ses.focal0, dense=True, filter_depth=1e9)
    frame, pix, _ = ses.source_pixels(src, sel)
    assert len(sel) == n - 1 and set(frame.tolist()) == set(sel.tolist())
    for ci in range(len(ses.classes)):
        at = np.flatnonzero(ses.frame_class[sel] == ci)
        sc = ses.scene_coordinates(head, sel[at])
        for j, k in enumerate(at):
            i = sel[k]
            x1, s1, cnt, _ = filter_scene_coordinates(sc[j:j + 1], torch.eye(4)[None], ses._K(ses.focal0, i)[None], 1e9, True, len(sel),
                                                      seed=ses.opt.random_seed, first_frame_id=int(k), opengl=False)
            assert int(cnt[0]) < ses.classes[ci].hw                      # sub-sampled
            assert np.array_equal(xyz[frame == i], x1.cpu().numpy()) and np.array_equal(pix[frame == i], s1.cpu().numpy()), i


def test_train_writes_each_focal_in_its_original_units(tmp_path):
    """Frames at two original scales (every third portrait frame stored at twice the size, resize factor 0.5, its focal twice as large in
    its own pixels): train_ace.py --use_ace_pose_file converts every focal with the frame's own factor and writes it back in the frame's
    original units; export_point_cloud.py reads that pose file."""
    from PIL import Image
    from acezero_amd import cli
    seq, files = _mixed_room(tmp_path, 13, 12, 12.0, depth=False)
    big = [i for i in range(12) if i % 3 == 2]
    for i in big:
        im = Image.open(files[i])
        im.resize((im.size[0] * 2, im.size[1] * 2), Image.NEAREST).save(files[i])
    gt = seq["poses"].cpu().numpy().astype(np.float64)
    supplied = [seq["focal"] * (2 if i in big else 1) + 0.25 * i for i in range(12)]   # (distinct per frame)
    with open(tmp_path / "poses_in.txt", "w") as f:
        for i in range(12):
            cli.write_pose_line(f, files[i], np.linalg.inv(gt[i]), 2000, supplied[i])
    out = tmp_path / "map" / "scene.pt"
    rc = cli.train_main([str(tmp_path / "rgb_*.png"), str(out), "--use_ace_pose_file", str(tmp_path / "poses_in.txt"), "--encoder_path",
                         str(tmp_path / "encoder.pt"), "--iterations", "600", "--learning_rate_warmup_iterations", "100",
                         "--learning_rate_cooldown_iterations", "100", "--aug_rotation", "2", "--aug_scale", "1.06"])
    assert rc == 0
    fl, _, focals = cli.read_ace_pose_file(tmp_path / "map" / "poses_scene_preliminary.txt", 0)
    assert fl == files and np.allclose(focals, supplied, rtol=1e-12, atol=0)
    rc = cli.export_point_cloud_main([str(tmp_path / "pc.txt"), "--network", str(out), "--pose_file", str(tmp_path / "map" / "poses_scene_preliminary.txt"),
                                      "--encoder_path", str(tmp_path / "encoder.pt"), "--convention", "opencv", "--dense_point_cloud", "True"])
    assert rc == 0 and len(np.loadtxt(tmp_path / "pc.txt")) > 0
