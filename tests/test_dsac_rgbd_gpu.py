"""GPU: DSAC* RGB-D registration (acezero_amd/csrc/ransac_rgbd.hip) against the fp64 numpy restatement (tests/rgbd_restated.py),
known answers on synthetic frames, determinism, edge cases, the reference call shape and register_mapping_rgbd.py end to end."""
import numpy as np
import pytest
import torch

from tests import rgbd_restated as O
from acezero_amd import dsacstar

pytestmark = pytest.mark.gpu


def _rot(rng, deg=180.0):
    ax = rng.normal(size=3)
    return O.rodrigues(ax / np.linalg.norm(ax) * np.radians(rng.uniform(0, deg)))


def make_frames(seed, n=4, h=60, w=80, focal=525.0, noise=0.01, outliers=0.3, missing=0.2):
    """Scene coordinates from ground-truth poses, camera coordinates back-projected from a depth map (dsacstar.camera_coordinates), 1 cm
    Gaussian noise per axis on the camera coordinates, a share of outlier scene coordinates and of cells without depth.
    Returns (scene [n,3,h,w], camera [n,3,h,w], world->camera [n,4,4] f64)."""
    rng = np.random.default_rng(seed)
    depth = rng.uniform(1.0, 4.0, (n, h, w)).astype(np.float32)
    eye = dsacstar.camera_coordinates(torch.from_numpy(depth), focal, w * 4.0, h * 4.0).numpy().astype(np.float64)
    sc, gt = np.zeros((n, 3, h, w), np.float32), np.zeros((n, 4, 4))
    for i in range(n):
        R, t = _rot(rng), rng.uniform(-3, 3, 3)
        gt[i] = np.eye(4)
        gt[i][:3, :3], gt[i][:3, 3] = R, t
        X = np.einsum("ji,jhw->ihw", R, eye[i] - t[:, None, None])      # R^T (eye - t)
        bad = rng.random((h, w)) < outliers
        X[:, bad] = rng.uniform(-5, 5, (3, int(bad.sum())))
        sc[i] = X
    cc = (eye + rng.normal(0, noise, eye.shape) if noise else eye).astype(np.float32)
    miss = rng.random((n, h, w)) < missing
    cc[:, 2][miss] = 0.0
    cc[:, 0][miss] = 0.0
    cc[:, 1][miss] = 0.0
    return sc, cc, gt


def _run(sc, cc, hyps=64, tries=16, seed=1305, ids=None, thr=10.0, alpha=100.0, maxd=100.0):
    prm = dict(hyps=hyps, thr=thr, alpha=alpha, max_reproj=maxd, max_tries=tries)
    ids = list(range(len(sc))) if ids is None else ids
    p, i, m = dsacstar.register_batch_rgbd(torch.from_numpy(sc).cuda(), torch.from_numpy(cc).cuda(), prm, seed, ids)
    torch.cuda.synchronize()
    return p.cpu().numpy(), i.cpu().numpy(), m.cpu().numpy(), dsacstar.debug_fetch_rgbd(len(sc), hyps)


def _close(a, b, rtol=1e-9):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.allclose(a, b, rtol=rtol, atol=rtol * max(1.0, float(np.abs(b).max())))


@pytest.mark.parametrize("shape,outliers", [((60, 80), 0.3), ((60, 80), 0.7), ((96, 128), 0.3)])   # 96 x 128: lists in HBM
def test_against_the_numpy_restatement(shape, outliers):
    h, w = shape
    sc, cc, _ = make_frames(7 + h, n=3, h=h, w=w, outliers=outliers)
    hyps, tries, thr, alpha, maxd, seed = 64, 16, 10.0, 100.0, 100.0, 1305
    ids = [3, 900, 2 ** 40]
    poses, inl, masks, dbg = _run(sc, cc, hyps, tries, seed, ids, thr, alpha, maxd)
    for f in range(len(sc)):
        cells = O.valid_cells(cc[f])
        S, E = sc[f].reshape(3, -1).T[cells], cc[f].reshape(3, -1).T[cells]
        ref = O.sample(sc[f], cc[f], hyps, tries, thr, seed, ids[f])
        for hh, (trip, pose, ok) in enumerate(ref):
            assert np.array_equal(dbg["samples"][f, hh], trip), (f, hh)          # the same stream, the same accepted try
            if pose is None:
                assert not dbg["hyp_poses"][f, hh].any()
                continue
            assert _close(dbg["hyp_poses"][f, hh], pose), (f, hh)              # Kabsch of its triple
            sel = [int(np.flatnonzero(cells == m)[0]) for m in trip]
            if ok:
                assert (O.dist_errs(dbg["hyp_poses"][f, hh], S[sel], E[sel], np.inf) < thr).all()
        scores = np.array([O.score(O.dist_errs(dbg["hyp_poses"][f, hh], S, E, maxd), h * w, thr, alpha, maxd, h, w) for hh in range(hyps)])
        assert _close(dbg["scores"][f], scores), f
        assert dbg["best"][f] == int(np.argmax(dbg["scores"][f]))             # the first maximum
        pose, acc, cnt = O.refine(dbg["hyp_poses"][f, dbg["best"][f]], S, E, thr, maxd)
        mask = np.zeros(h * w, np.uint8)
        if acc is not None:
            mask[cells[acc]] = 1
        assert inl[f] == cnt and np.array_equal(masks[f].reshape(-1), mask), f
        assert _close(dbg["refined"][f], pose), f
        np.testing.assert_allclose(poses[f], O.pose2trans(pose).astype(np.float32), rtol=1e-6, atol=1e-6)


def test_known_answer():
    sc, cc, gt = make_frames(21, n=6)
    poses, inl, _, _ = _run(sc, cc)
    for i in range(len(sc)):
        est = np.linalg.inv(poses[i].astype(np.float64))                       # world -> camera
        dt = np.linalg.norm(est[:3, 3] - gt[i][:3, 3])
        ang = np.degrees(np.arccos(np.clip((np.trace(est[:3, :3] @ gt[i][:3, :3].T) - 1) / 2, -1, 1)))
        assert dt < 0.01 and ang < 0.1, (i, dt, ang)
        assert inl[i] > 0.5 * 0.7 * 0.8 * sc[i, 0].size
    sc, cc, gt = make_frames(22, n=4, noise=0.0)
    poses, inl, _, _ = _run(sc, cc)
    for i in range(len(sc)):
        np.testing.assert_allclose(poses[i], np.linalg.inv(gt[i]), atol=1e-5)


def test_determinism_over_batch_size_and_order():
    sc, cc, _ = make_frames(31, n=6)
    ids = [10, 11, 12, 13, 14, 15]
    p, i, m, _ = _run(sc, cc, ids=ids)
    for order in ([5, 2, 0], [3], [4, 3, 2, 1, 0, 5]):
        p2, i2, m2, _ = _run(sc[order], cc[order], ids=[ids[k] for k in order])
        assert np.array_equal(p2.view(np.uint32), p[order].view(np.uint32))
        assert np.array_equal(i2, i[order]) and np.array_equal(m2, m[order])


def test_edge_cases():
    h, w = 60, 80
    sc, cc, _ = make_frames(41, n=6)
    # 0: two valid cells; 1: every cell identical; 2: collinear cells (exactly on the x axis); 3: NaN depth everywhere;
    # 4: half the depth NaN, a quarter zero (still a good frame); 5: an all-zero frame
    cc[0] = 0.0
    cc[0][:, 3, 5] = (0.1, 0.2, 1.5)
    cc[0][:, 7, 9] = (0.3, 0.1, 2.0)
    sc[1] = np.array([1.0, 2.0, 3.0], np.float32)[:, None, None]
    cc[1] = np.array([0.5, -0.5, 2.0], np.float32)[:, None, None]
    xs = np.arange(h * w, dtype=np.float32).reshape(h, w) * 0.001
    sc[2] = np.stack([xs, np.zeros_like(xs), np.zeros_like(xs)])
    cc[2] = np.stack([xs, np.zeros_like(xs), np.full_like(xs, 2.0)])
    cc[3][2] = np.nan
    rng = np.random.default_rng(5)
    nanm, zerom = rng.random((h, w)) < 0.5, rng.random((h, w)) < 0.25
    cc[4][2][nanm] = np.nan
    cc[4][:, zerom] = 0.0
    sc[5] = 0.0
    cc[5] = 0.0
    poses, inl, masks, dbg = _run(sc, cc)
    assert np.isfinite(poses).all() and np.isfinite(dbg["scores"]).all() and np.isfinite(dbg["hyp_poses"]).all()
    for f in (0, 1, 2, 3, 5):          # < 3 valid cells, or every triple (and the identity's inlier set) rank-deficient
        assert np.array_equal(poses[f], np.eye(4, dtype=np.float32)) and inl[f] == 0 and not masks[f].any(), f
    assert (dbg["samples"][0] == -1).all() and (dbg["samples"][3] == -1).all()
    assert inl[4] > 500 and not masks[4][nanm | zerom].any()


def test_forward_rgbd_reference_call_shape():
    sc, cc, _ = make_frames(51, n=2)
    dsacstar.reset_call_counter(0)
    counts, outs = [], []
    for i in range(2):
        big_s, big_c = torch.zeros(1, 3, 60, 160), torch.zeros(1, 3, 60, 160)
        big_s[..., ::2], big_c[..., ::2] = torch.from_numpy(sc[i]), torch.from_numpy(cc[i])
        out = torch.zeros(4, 4)
        n = dsacstar.forward_rgbd(big_s[..., ::2], big_c[..., ::2], out, 64, 10.0, 100.0, 100.0)   # non-contiguous host views
        assert isinstance(n, int)
        counts.append(n)
        outs.append(out.numpy().copy())
    # the call counter keys the stream (seed 0): the batched device call with frame ids 0, 1 gives the same bits
    p, i, _, _ = _run(sc, cc, hyps=64, tries=dsacstar.MAX_HYPOTHESES_TRIES, seed=0, ids=[0, 1])
    assert counts == [int(x) for x in i]
    assert np.array_equal(np.stack(outs).view(np.uint32), p.view(np.uint32))
    import dsacstar as top
    top.reset_call_counter(1)
    out = torch.zeros(4, 4, device="cuda")
    assert top.forward_rgbd(torch.from_numpy(sc[1:2]).cuda(), torch.from_numpy(cc[1:2]).cuda(), out, 64, 10.0, 100.0, 100.0) == counts[1]
    assert np.array_equal(out.cpu().numpy().view(np.uint32), outs[1].view(np.uint32))


def test_register_mapping_rgbd_end_to_end(tmp_path):
    """train_ace.py on PNG frames + 16-bit depth, then register_mapping_rgbd.py: every frame in the pose file, bitwise the poses
    register_batch_rgbd gives on the session's scene and camera coordinates."""
    from PIL import Image
    from acezero_amd import cli, synth
    from acezero_amd.session import ReconstructionSession
    n = 16
    seq = synth.render_room_sequence(seed=5, n_frames=n, arc_deg=15.0, device="cuda")
    files = []
    for i in range(n):
        img = ((seq["images"][i, 0] * 0.25 + 0.4).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
        files.append(str(tmp_path / f"rgb_{i:04d}.png"))
        Image.fromarray(np.stack([img] * 3, -1)).save(files[-1])
        dep = (seq["depth"][i].cpu().numpy() * 1000).round().astype(np.uint16)
        Image.fromarray(np.kron(dep, np.ones((8, 8), np.uint16))).save(tmp_path / f"depth_{i:04d}.png")
        np.savetxt(tmp_path / f"pose_{i:04d}.txt", seq["poses"][i].cpu().numpy().astype(np.float64))
    torch.save({k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}, tmp_path / "encoder.pt")
    out = tmp_path / "map" / "scene.pt"
    f = str(seq["focal"])
    assert cli.train_main([str(tmp_path / "rgb_*.png"), str(out), "--pose_files", str(tmp_path / "pose_*.txt"), "--depth_files",
                           str(tmp_path / "depth_*.png"), "--encoder_path", str(tmp_path / "encoder.pt"), "--use_external_focal_length", f,
                           "--iterations", "1500", "--learning_rate_cooldown_iterations", "300", "--aug_rotation", "2"]) == 0
    assert cli.register_rgbd_main([str(tmp_path / "rgb_*.png"), str(out), "--depth_files", str(tmp_path / "depth_*.png"), "--encoder_path",
                                   str(tmp_path / "encoder.pt"), "--session", "rgbd", "--use_external_focal_length", f]) == 0
    lines = open(tmp_path / "map" / "poses_rgbd.txt").read().splitlines()
    assert [ln.split()[0] for ln in lines] == files
    # the same session by hand
    _, frames, fscale = cli.load_frames(str(tmp_path / "rgb_*.png"))
    H, W = frames.shape[2:]
    depth = torch.from_numpy(np.stack([cli.depth_map_at_cells(str(tmp_path / f"depth_{i:04d}.png"), H, W) for i in range(n)]))
    opt = cli.register_rgbd_parser().parse_args([str(tmp_path / "rgb_*.png"), str(out), "--depth_files", "x"])
    so = cli._session_options(opt, use_external_focal_length=float(f) * fscale, ransac_iterations=64, ransac_threshold=10.0,
                              register_seed=opt.base_seed, use_aug=False, registration_confidence=opt.confidence_threshold)
    ses = ReconstructionSession(torch.load(tmp_path / "encoder.pt"), frames, opt=so, depth=depth)
    ids = np.arange(n)
    sc = ses.scene_coordinates(torch.load(out), ids)
    cc = dsacstar.camera_coordinates(ses.frame_depth(ids), ses.focal0, ses.ppx, ses.ppy)
    p, inl, _ = dsacstar.register_batch_rgbd(sc, cc, dict(hyps=64, thr=10.0, alpha=100.0, max_reproj=100.0, max_tries=opt.hypotheses_max_tries),
                                             opt.base_seed, list(ids), want_masks=False)
    p, inl = p.cpu().numpy(), inl.cpu().numpy()
    import io
    buf = io.StringIO()
    for k in range(n):
        cli.write_pose_line(buf, files[k], np.linalg.inv(p[k].astype(np.float64)), int(inl[k]), ses.focal0 / fscale)
    assert buf.getvalue().splitlines() == lines
    gt = seq["poses"].cpu().numpy().astype(np.float64)
    dt = np.linalg.norm(p[:, :3, 3] - gt[:, :3, 3], axis=1)
    assert np.median(dt) < 0.05 and (inl > 100).mean() > 0.9
