"""GPU: acez_render_frame bit-exact against tests/render_oracle.py on seeded scenes, repeatable, argument checks; the mapping and
registration phases of train_ace.py / register_mapping.py write their frames and state files."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_oracle as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _look_at(eye, target):
    """OpenGL cam->world looking from eye to target (y up)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross([0, 1.0, 0], z)
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def _scene(seed, n_points, n_tris, near=0.05):
    rng = np.random.default_rng(seed)
    T = _look_at([0.3, 0.5, 4.0], [0, 0, 0])
    xyz = rng.normal(size=(n_points, 3)).astype(np.float32) * 2
    rgb = rng.integers(0, 256, size=(n_points, 3)).astype(np.uint8)
    if n_points >= 64:
        cam = np.linalg.inv(T)
        xyz[:8] = (T[:3, :3] @ np.array([0.1, 0.05, near])[:, None] + T[:3, 3:4]).T.astype(np.float32)   # behind the camera
        on = T @ np.array([0.0, 0.0, -np.float32(near), 1.0])
        xyz[8] = on[:3]                                                         # near the near plane
        xyz[9:16] = xyz[16:23]                                                  # exact duplicates: equal depths, lower index wins
        xyz[23:30] = (T[:3, :3] @ np.array([50.0, 0, -1.0])[:, None] + T[:3, 3:4]).T.astype(np.float32)   # off-screen
        del cam
    ctr = rng.normal(size=(n_tris, 1, 3)) * 1.5
    tri = (ctr + rng.normal(size=(n_tris, 3, 3)) * 0.3).astype(np.float32)
    if n_tris >= 8:                                                             # crossing the near plane / behind the camera
        for k in range(4):
            a = T[:3, 3] + T[:3, :3] @ np.array([-0.5 + 0.2 * k, -0.3, -1.0])
            b = T[:3, 3] + T[:3, :3] @ np.array([0.6, -0.2 + 0.1 * k, 0.5])
            c = T[:3, 3] + T[:3, :3] @ np.array([0.1, 0.4, -0.8 + 0.5 * k])
            tri[k] = np.stack([a, b, c]).astype(np.float32)
        tri[5] = tri[4]                                                         # equal depths among triangles
    rgba = rng.integers(0, 256, size=(n_tris, 4)).astype(np.uint8)
    rgba[::3, 3] = 255
    return xyz, rgb, tri, rgba, T


def _gpu(xyz, rgb, tri, rgba, T, W, H, flipped=False, near=0.05, far=100.0):
    from acezero_amd.render import Renderer
    r = Renderer(W, H, flipped_portrait=flipped, znear=near, zfar=far)
    return r.render(torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda(), torch.from_numpy(tri).cuda(), torch.from_numpy(rgba).cuda(), T)


@pytest.mark.parametrize("seed,n_points,n_tris,W,H,flipped", [(1, 5000, 300, 320, 180, False), (2, 20000, 1000, 1280, 720, False),
                                                              (3, 3000, 200, 180, 320, True), (4, 0, 400, 160, 90, False),
                                                              (5, 4000, 0, 160, 90, False)])
def test_frame_matches_oracle(seed, n_points, n_tris, W, H, flipped):
    xyz, rgb, tri, rgba, T = _scene(seed, n_points, n_tris)
    rw, rh = (H, W) if flipped else (W, H)
    got = _gpu(xyz, rgb, tri, rgba, T, W, H, flipped)
    ref = R.render(xyz, rgb, tri, rgba, T, 0.05, 100.0, rw, rh, flipped)
    assert got.shape == ref.shape
    bad = np.argwhere((got != ref).any(axis=2))
    assert len(bad) == 0, (len(bad), bad[:5].tolist())
    assert got.any()


def test_two_million_points_match_oracle():
    xyz, rgb, tri, rgba, T = _scene(7, 2_000_000, 50)
    got = _gpu(xyz, rgb, tri, rgba, T, 1280, 720)
    ref = R.render(xyz, rgb, tri, rgba, T, 0.05, 100.0, 1280, 720)
    assert np.array_equal(got, ref)


def test_repeat_renders_are_identical():
    xyz, rgb, tri, rgba, T = _scene(8, 300000, 2000)
    a = _gpu(xyz, rgb, tri, rgba, T, 640, 360)
    b = _gpu(xyz, rgb, tri, rgba, T, 640, 360)
    assert np.array_equal(a, b)


def test_bad_arguments():
    from acezero_amd import _native as N
    lib = N.lib()
    work = torch.empty(2 * 64 * 32, dtype=torch.int64, device="cuda")
    out = torch.empty(64 * 32 * 3, dtype=torch.uint8, device="cuda")
    cam = (C.c_double * 16)(*np.eye(4).reshape(16).tolist())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    wp, op = C.c_void_p(work.data_ptr()), C.c_void_p(out.data_ptr())
    assert lib.acez_render_frame(None, None, 0, None, None, 0, cam, 0.05, 100.0, 64, 32, 0, None, op, s) == -1
    assert b"null" in lib.acez_last_error()
    assert lib.acez_render_frame(None, None, 5, None, None, 0, cam, 0.05, 100.0, 64, 32, 0, wp, op, s) == -1
    assert lib.acez_render_frame(None, None, 0, None, None, 0, cam, 0.0, 100.0, 64, 32, 0, wp, op, s) == -1
    assert lib.acez_render_frame(None, None, 0, None, None, 0, cam, 0.05, 100.0, 0, 32, 0, wp, op, s) == -1
    bad = (C.c_double * 16)(*([float("nan")] + [0.0] * 15))
    assert lib.acez_render_frame(None, None, 0, None, None, 0, bad, 0.05, 100.0, 64, 32, 0, wp, op, s) == -1
    assert b"not finite" in lib.acez_last_error()
    assert lib.acez_render_frame(None, None, 0, None, None, 0, cam, 0.05, 100.0, 64, 32, 0, wp, op, s) == 0
    torch.cuda.synchronize()
    assert not out.any()                                   # nothing to draw: black


def _run(script, *args, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + [str(a) for a in args], capture_output=True, text=True, cwd=cwd,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def _frames(folder):
    return sorted(f for f in os.listdir(folder) if f.startswith("frame_") and f.endswith(".png"))


def _drawn(im):
    """Non-black pixels of a 1280 x 720 frame outside the caption and histogram areas (rows 60-600, columns 0-960)."""
    return int(im[60:600, :960].any(axis=2).sum())


def test_mapping_registration_and_sweep_write_their_frames(tmp_path):
    from PIL import Image
    from acezero_amd import cli, synth
    prob = synth.make_training_problem(seed=4, n_images=8, views_per_image=2, patches_per_view=512)
    buf = tmp_path / "buffer.npz"
    cli.save_feature_buffer(buf, prob)
    rend = tmp_path / "renderings"
    train = ["train_ace.py", "synthetic/*.png", tmp_path / "scene.pt", "--feature_buffer", buf, "--iterations", "60", "--learning_rate_schedule",
             "constant", "--repro_loss_type", "tanh", "--batch_size", "1024", "--render_target_path", rend]
    # flag off (the default): no renderings folder
    _run(*train[:-2], "--iterations_output", "20", cwd=tmp_path)
    assert not rend.exists() and not (tmp_path / "renderings").exists()
    # mapping: one frame per iterations_output steps that were trained, then 10 transition frames: 60 // 20 + 10 = 13
    _run(*train, "--iterations_output", "20", "--render_visualization", "True", cwd=tmp_path)
    frames = _frames(rend)
    assert frames == [f"frame_{i:05d}.png" for i in range(60 // 20 + 10)]
    im = np.asarray(Image.open(rend / frames[-1]))
    assert im.shape == (720, 1280, 3)
    assert _drawn(im) > 100                                           # the map and the cameras, not just the captions
    st = pickle.load(open(rend / "scene_mapping.pkl", "rb"))
    assert {"map_xyz", "map_clr", "frame_idx", "camera_buffer", "pan_cameras"} <= set(st) and st["frame_idx"] == 13
    assert len(st["pan_cameras"]) == 100 + 10 and st["map_xyz"].shape[1] == 3 and len(st["map_xyz"]) == len(st["map_clr"])
    # registration: one frame per query (<= 60 queries), the register state continues the frame count
    fr = synth.make_registration_frames(seed=6, n_frames=5)
    ff = tmp_path / "frames.npz"
    np.savez(ff, scene_coordinates=fr["scene_coords"], focal=np.float32(fr["focal"]), ppx=np.float32(fr["ppx"]), ppy=np.float32(fr["ppy"]),
             image_files=np.array([f"f{i}.png" for i in range(5)]))
    _run("register_mapping.py", "synthetic/*.png", tmp_path / "scene.pt", "--feature_file", ff, "--session", "iteration1", "--hypotheses", "32",
         "--hypotheses_max_tries", "16", "--render_visualization", "True", "--render_target_path", rend, cwd=tmp_path)
    assert _frames(rend) == [f"frame_{i:05d}.png" for i in range(13 + 5)]
    reg = pickle.load(open(rend / "scene_register.pkl", "rb"))
    assert reg["frame_idx"] == 18 and np.array_equal(reg["map_xyz"], st["map_xyz"])
    # final sweep: render_final_sweep.py finds iteration<k>_register.pkl and ../poses_iteration<k>.txt and draws 150 frames
    os.rename(rend / "scene_register.pkl", rend / "iteration1_register.pkl")
    _run("render_final_sweep.py", rend, cwd=tmp_path)
    assert _frames(rend) == [f"frame_{i:05d}.png" for i in range(18 + 150)]


def test_ace_zero_renders_every_phase_and_the_sweep(tmp_path):
    """ace_zero.py --render_visualization True on image files: results/renderings holds the frames of every round (the best seed
    mapped again, then mapping and registration of each round) and, after the last round's registration state, the final sweep's
    150 frames; without ffmpeg on PATH the frames stay and the command is logged."""
    from PIL import Image
    from acezero_amd import cli, synth
    seq = synth.render_room_sequence(seed=7, n_frames=32, arc_deg=20.0, device="cuda")
    img = ((seq["images"][:, 0] * 0.25 + 0.4).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
    dep = (seq["depth"].cpu().numpy() * 1000).round().astype(np.uint16)
    for i in range(len(img)):
        Image.fromarray(np.stack([img[i]] * 3, -1)).save(tmp_path / f"rgb_{i:04d}.png")
        Image.fromarray(np.kron(dep[i], np.ones((8, 8), np.uint16))).save(tmp_path / f"depth_{i:04d}.png")
    torch.save({k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}, tmp_path / "encoder.pt")
    out = tmp_path / "result"
    it = "2000"
    rc = cli.ace_zero_main([str(tmp_path / "rgb_*.png"), str(out), "--depth_files", str(tmp_path / "depth_*.png"), "--encoder_path",
                            str(tmp_path / "encoder.pt"), "--use_external_focal_length", str(seq["focal"]), "--try_seeds", "1",
                            "--seed_iterations", it, "--refit_iterations", it, "--final_refit_posewait", "400", "--cooldown_iterations", "400",
                            "--iterations_max", "3", "--aug_rotation", "2", "--iterations_output", "1000", "--render_visualization", "True"])
    assert rc == 0
    rend = out / "renderings"
    assert (rend / "iteration0_seed0_mapping.pkl").exists() and (rend / "iteration0_seed0_register.pkl").exists()
    regs = sorted(int(f[len("iteration"):-len("_register.pkl")]) for f in os.listdir(rend) if f.endswith("_register.pkl") and "seed" not in f)
    assert regs and (rend / f"iteration{regs[-1]}_mapping.pkl").exists()
    last = pickle.load(open(rend / f"iteration{regs[-1]}_register.pkl", "rb"))
    frames = _frames(rend)
    assert frames == [f"frame_{i:05d}.png" for i in range(last["frame_idx"] + 150)]     # every phase, then the sweep's 150 frames
    assert last["frame_idx"] >= 2 * (10 + 32)                       # >= two rendered rounds: 10 transition frames + 32 queries each
    im = np.asarray(Image.open(rend / frames[-1]))
    assert im.shape == (720, 1280, 3) and _drawn(im) > 100
    assert not (out / "reconstruction.mp4").exists() or os.path.getsize(out / "reconstruction.mp4") > 0
