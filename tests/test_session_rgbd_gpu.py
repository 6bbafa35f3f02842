"""RGB-D reconstruction end to end on the GPU: ace_zero.py --rgbd True on the synthetic room with depth for all
frames, next to the RGB run of the same folder (the yardstick): every frame registered, one line per image in every pose file, two
runs byte-identical, the result metric (similarity alignment to ground truth gives scale 1) and registered no worse than the RGB
run's; a folder of two frame sizes; and the depth -> camera-coordinate launch against a numpy restatement, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from acezero_amd import dsacstar
from acezero_amd import evaluate as ev
from acezero_amd.evaluate import estimate_alignment, evaluate_poses, read_pose_file_with_confidence
from tests.test_mixed_sizes_gpu import _mixed_room

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FRAMES, CONFIDENCE = 48, 500
RUN_LIMIT_S = 600          # one reconstruction of this folder takes well under a minute; a run that does not end is killed

# The bounds. Measured once on an MI355X (this folder, these flags; DESIGN.md section 4g has the same figures):
#   RGB-D run:               similarity scale 1.10976, rigid (no scale) median errors 0.698 cm / 3.7488 deg
#   RGB run (the yardstick): similarity scale 1.02840, rigid (no scale) median errors 0.272 cm / 1.6894 deg
# The camera centres of this 24-degree arc span 22 cm, so 0.7 cm of centre error is about 6 % of scale and the alignment's rotation is
# weakly held: both runs' figures are large for that reason, and the RGB-D run's are the larger ones (DESIGN.md section 4g says why).
# Headroom: the existing session tests put their bounds 20 to 25 % beyond what they measured (tests/test_session_gpu.py's scale window
# 0.8 .. 1.25 around 1; tests/test_mixed_sizes_gpu.py's 0.5 below a measured 0.62). Here: measured value x 1.25, rounded up.
SCALE_MARGIN = 0.14        # measured |scale - 1| = 0.10976; x 1.25 = 0.1372
T_MARGIN_CM = 0.54         # measured RGB-D minus RGB = 0.698 - 0.272 = 0.426 cm; x 1.25 = 0.5325
R_MARGIN_DEG = 2.58        # measured RGB-D minus RGB = 3.7488 - 1.6894 = 2.0594 deg; x 1.25 = 2.5743


def _run_ace_zero(folder, out, *extra):
    """ace_zero.py as its users start it -- a process of its own, killed at RUN_LIMIT_S -- with the short iteration caps of
    tests/test_session_gpu.py's script test."""
    it = "2500"
    cmd = [sys.executable, os.path.join(ROOT, "ace_zero.py"), str(folder / "rgb_*.png"), str(out), "--depth_files", str(folder / "depth_*.png"),
           "--encoder_path", str(folder / "encoder.pt"), "--use_external_focal_length", str(_run_ace_zero.focal), "--try_seeds", "1",
           "--seed_iterations", it, "--refit_iterations", it, "--final_refit_posewait", "500", "--cooldown_iterations", "500",
           "--iterations_max", "6", "--aug_rotation", "2", "--registration_confidence", str(CONFIDENCE), *extra]
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=RUN_LIMIT_S)
    except subprocess.TimeoutExpired:
        # a reconstruction that hangs leaves the device in an unknown state: nothing more is started on it
        pytest.exit(f"ace_zero.py did not end within {RUN_LIMIT_S} s: {' '.join(cmd)}", returncode=3)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return out


def _poses(out, files, name="poses_final.txt"):
    by_name = read_pose_file_with_confidence(out / name)
    assert list(by_name) == files                                        # one line per image, in the images' order
    return np.stack([by_name[f][0] for f in files]), np.array([by_name[f][1] for f in files])


def _figures(out, files, gt):
    """(similarity scale, rigid median translation error in cm, rigid median rotation error in degrees) of a run's final poses."""
    est, conf = _poses(out, files)
    T, scale = estimate_alignment([ev.TestEstimate(e, g, 0.0, c, f) for e, g, c, f in zip(est, gt, conf, files)], CONFIDENCE, estimate_scale=True)
    assert T is not None
    rigid = evaluate_poses(est, gt, conf, estimate_alignment_scale=False, estimate_alignment_conf_threshold=CONFIDENCE)
    assert rigid["T"] is not None
    return float(scale), float(rigid["median_t_cm"]), float(rigid["median_r_deg"])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    folder = tmp_path_factory.mktemp("room")
    seq, files = _mixed_room(folder, 7, N_FRAMES, 24.0, portrait=lambda i: False)      # one size: rgb_*.png, depth_*.png for ALL frames, encoder.pt
    _run_ace_zero.focal = seq["focal"]
    gt = seq["poses"].cpu().numpy().astype(np.float64)
    a = _run_ace_zero(folder, folder / "rgbd_a", "--rgbd", "True", "--export_point_cloud", "True")
    b = _run_ace_zero(folder, folder / "rgbd_b", "--rgbd", "True", "--export_point_cloud", "True")
    rgb = _run_ace_zero(folder, folder / "rgb")
    return dict(files=sorted(files), gt=gt, rgbd=a, rgbd_again=b, rgb=rgb)


def test_both_runs_register_every_frame_and_write_one_line_per_image(runs):
    for key in ("rgbd", "rgb"):
        out = runs[key]
        pose_files = sorted(f for f in os.listdir(out) if f.startswith("poses_") and f.endswith(".txt"))
        assert "poses_final.txt" in pose_files and "poses_iteration0_seed0.txt" in pose_files and "poses_iteration1.txt" in pose_files
        for name in pose_files:
            _, conf = _poses(out, runs["files"], name)
            assert len(conf) == N_FRAMES, (key, name)
            assert (out / (name[len("poses_"):-4] + ".pt")).exists() or name == "poses_final.txt"
        _, conf = _poses(out, runs["files"])
        print(f"{key}: final confidences min {conf.min():.0f} median {np.median(conf):.0f}")
        assert (conf >= CONFIDENCE).all(), (key, conf)                  # every frame registered at --registration_confidence
    # the confidence of an RGB-D pose file is the RGB-D estimator's inlier count: whole cells of the 60 x 80 map
    _, conf = _poses(runs["rgbd"], runs["files"])
    assert np.array_equal(conf, np.round(conf)) and conf.max() <= 60 * 80
    assert open(runs["rgbd"] / "pc_final.ply", "rb").read(200).startswith(b"ply\nformat binary_little_endian")


def test_two_rgbd_runs_with_one_seed_write_identical_pose_files(runs):
    a, b = runs["rgbd"], runs["rgbd_again"]
    assert open(a / "poses_final.txt", "rb").read() == open(b / "poses_final.txt", "rb").read()
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))


def test_rgbd_reconstruction_is_metric_and_no_worse_than_the_rgb_run(runs):
    scale, t_cm, r_deg = _figures(runs["rgbd"], runs["files"], runs["gt"])
    rgb_scale, rgb_t_cm, rgb_r_deg = _figures(runs["rgb"], runs["files"], runs["gt"])
    print(f"RGB-D: scale {scale:.5f}, rigid median errors {t_cm:.3f} cm / {r_deg:.4f} deg; "
          f"RGB (yardstick): scale {rgb_scale:.5f}, rigid median errors {rgb_t_cm:.3f} cm / {rgb_r_deg:.4f} deg")
    assert abs(scale - 1.0) < SCALE_MARGIN, scale
    assert t_cm <= rgb_t_cm + T_MARGIN_CM, (t_cm, rgb_t_cm)
    assert r_deg <= rgb_r_deg + R_MARGIN_DEG, (r_deg, rgb_r_deg)


def test_rgbd_reconstruction_of_two_frame_sizes_registers_every_frame(tmp_path):
    seq, files = _mixed_room(tmp_path, 7, N_FRAMES, 24.0)                # every third frame portrait (640 x 480), depth for all frames
    _run_ace_zero.focal = seq["focal"]
    out = _run_ace_zero(tmp_path, tmp_path / "result", "--rgbd", "True")
    _, conf = _poses(out, sorted(files))
    por = np.array([i % 3 == 2 for i in range(N_FRAMES)])
    print(f"mixed sizes: confidences landscape min {conf[~por].min():.0f}, portrait min {conf[por].min():.0f}")
    assert (conf >= CONFIDENCE).all(), conf
    scale, t_cm, r_deg = _figures(out, sorted(files), seq["poses"].cpu().numpy().astype(np.float64))
    print(f"mixed sizes: scale {scale:.5f}, rigid median errors {t_cm:.3f} cm / {r_deg:.4f} deg")


# --------------------------------------------------------------------------------------------- depth -> camera coordinates, one launch
def _camera_coordinates_restated(depth, focal, ppx, ppy, stride=8):
    """numpy restatement of acez_camera_coordinates: float32 throughout, ((px - ppx) / f) * d, ((py - ppy) / f) * d, d in this order;
    +0 in all three channels where d == 0."""
    d = np.asarray(depth, np.float32)
    n, h, w = d.shape
    f = np.broadcast_to(np.asarray(focal, np.float32), (n,)).reshape(n, 1, 1)
    px = (np.arange(w, dtype=np.int32) * stride + stride // 2).astype(np.float32).reshape(1, 1, w)
    py = (np.arange(h, dtype=np.int32) * stride + stride // 2).astype(np.float32).reshape(1, h, 1)
    with np.errstate(all="ignore"):
        x = (px - np.float32(ppx)) / f * d
        y = (py - np.float32(ppy)) / f * d
    out = np.stack([x, y, d], axis=1).astype(np.float32)
    out[np.broadcast_to((d == 0)[:, None], out.shape)] = 0.0
    return out


@pytest.mark.parametrize("n,h,w,ppx,ppy", [(7, 60, 80, 320.0, 240.0), (3, 80, 60, 240.0, 320.0), (5, 61, 77, 301.5, 250.25), (1, 128, 128, 512.0, 512.0)])
def test_camera_coordinate_launch_is_bit_identical_to_its_restatement(n, h, w, ppx, ppy):
    rng = np.random.default_rng(n * 1000 + h)
    depth = rng.uniform(0.3, 12.0, size=(n, h, w)).astype(np.float32)
    depth[rng.random((n, h, w)) < 0.3] = 0.0                              # holes
    depth[0, : h // 2] = 0.0                                              # a frame whose upper half has no depth
    depth[-1, 3, 5] = 1500.0                                              # beyond the mapping range: still back-projected
    if n > 2:
        depth[1] = 0.0                                                    # a frame without any depth
    focal = (525.0 + 3.7 * np.arange(n)).astype(np.float32)               # one focal per frame
    got = dsacstar.camera_coordinates_device(torch.from_numpy(depth).cuda(), focal, ppx, ppy).cpu().numpy()
    want = _camera_coordinates_restated(depth, focal, ppx, ppy)
    assert got.shape == (n, 3, h, w) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))      # bit for bit, the sign of zero included
    assert np.array_equal(got[:, 2], depth) and not got[np.broadcast_to((depth == 0)[:, None], got.shape)].any()
    # against the torch-op path it replaces in register(use_depth=True): the same values wherever there is depth
    old = dsacstar.camera_coordinates(torch.from_numpy(depth).cuda(), focal, ppx, ppy).cpu().numpy()
    have = np.broadcast_to((depth != 0)[:, None], got.shape)
    assert np.array_equal(got[have].view(np.uint32), old[have].view(np.uint32)) and not old[~have].any()
    # one focal for all frames
    one = dsacstar.camera_coordinates_device(torch.from_numpy(depth).cuda(), 525.0, ppx, ppy).cpu().numpy()
    assert np.array_equal(one.view(np.uint32), _camera_coordinates_restated(depth, 525.0, ppx, ppy).view(np.uint32))


def test_registration_from_the_launched_coordinates_equals_the_former_path():
    """register(use_depth=True) now takes its camera coordinates from the launch: the estimator sees the same valid cells with the same
    values, so poses and inlier counts are those of the torch-op path, bit for bit."""
    g = torch.Generator(device="cuda").manual_seed(5)
    n, h, w = 16, 60, 80
    depth = torch.rand(n, h, w, generator=g, device="cuda") * 3 + 1
    depth[torch.rand(n, h, w, generator=g, device="cuda") < 0.25] = 0
    focal = [525.0 + i for i in range(n)]
    old = dsacstar.camera_coordinates(depth, focal, 320.0, 240.0)
    new = dsacstar.camera_coordinates_device(depth, focal, 320.0, 240.0)
    c, s = float(np.cos(0.3)), float(np.sin(0.3))
    R = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], device="cuda")
    sc = torch.einsum("ij,njhw->nihw", R, old) + torch.tensor([0.5, -1.0, 2.0], device="cuda").view(1, 3, 1, 1)
    sc = sc + torch.randn(sc.shape, generator=g, device="cuda") * 0.01
    prm = dict(hyps=32, thr=10.0, alpha=100.0, max_reproj=100.0)
    p0, i0, m0 = dsacstar.register_batch_rgbd(sc, old, prm, 1305, list(range(n)))
    p1, i1, m1 = dsacstar.register_batch_rgbd(sc, new, prm, 1305, list(range(n)))
    assert torch.equal(p0, p1) and torch.equal(i0, i1) and torch.equal(m0, m1) and int(i0.min()) > 1000
