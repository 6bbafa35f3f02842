"""GPU: the seed trials trained side by side (ace_zero.py --seed_parallel_workers) give exactly what the one-after-the-other flow gives:
the same seed rates, the same chosen seed, bit-identical seed heads; the command line writes byte-identical pose files."""
import os

import numpy as np
import pytest
import torch

from acezero_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def room():
    seq = synth.render_room_sequence(seed=2089, n_frames=48, arc_deg=30.0, device="cuda")
    esd = {k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}
    return seq, esd


def _seed_stage(room, workers):
    from acezero_amd.session import ReconstructionSession, default_options
    seq, esd = room
    it = 384
    opt = default_options(use_external_focal_length=seq["focal"], try_seeds=5, seed_iterations=it, learning_rate_warmup_iterations=it // 5,
                          cooldown_iterations=it // 5, aug_rotation=2, aug_scale=1.06, aug_black_white=0.02)
    ses = ReconstructionSession(esd, seq["images"], opt=opt, depth=seq["depth"])
    np.random.seed(opt.random_seed)                                  # reconstruct()'s draw of the seed images
    seeds = np.random.uniform(size=opt.try_seeds)
    trials = ses.run_seed_trials(list(range(len(seeds))), list(seeds), workers)
    return trials


def test_seed_trials_are_identical_for_every_worker_count(room):
    runs = {w: _seed_stage(room, w) for w in (1, 3, -1)}
    ref = runs[1]
    rates = [r for _, r in ref]
    assert len(ref) == 5
    for w, trials in runs.items():
        assert [r for _, r in trials] == rates, w
        assert int(np.argmax([r for _, r in trials])) == int(np.argmax(rates)), w
        for k, ((m, _), (m0, _)) in enumerate(zip(trials, ref)):
            assert m["iterations"] == m0["iterations"] and m["batch_inliers"] == m0["batch_inliers"] and m["loss"] == m0["loss"], (w, k)
            assert m["head"].keys() == m0["head"].keys()
            for name in m["head"]:
                a, b = m["head"][name], m0["head"][name]
                assert a.dtype == b.dtype == torch.float16 and torch.equal(a.view(torch.int16), b.view(torch.int16)), (w, k, name)


def test_ace_zero_pose_files_do_not_depend_on_seed_parallel_workers(tmp_path):
    from PIL import Image
    from acezero_amd import cli
    seq = synth.render_room_sequence(seed=7, n_frames=48, arc_deg=24.0, device="cuda")
    img = ((seq["images"][:, 0] * 0.25 + 0.4).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
    dep = (seq["depth"].cpu().numpy() * 1000).round().astype(np.uint16)
    for i in range(len(img)):
        Image.fromarray(np.stack([img[i]] * 3, -1)).save(tmp_path / f"rgb_{i:04d}.png")
        Image.fromarray(np.kron(dep[i], np.ones((8, 8), np.uint16))).save(tmp_path / f"depth_{i:04d}.png")
    torch.save({k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}, tmp_path / "encoder.pt")
    it = "2500"
    outs = {}
    for w in ("1", "3"):
        out = tmp_path / f"result_{w}"
        rc = cli.ace_zero_main([str(tmp_path / "rgb_*.png"), str(out), "--depth_files", str(tmp_path / "depth_*.png"), "--encoder_path",
                                str(tmp_path / "encoder.pt"), "--use_external_focal_length", str(seq["focal"]), "--try_seeds", "2",
                                "--seed_parallel_workers", w, "--seed_iterations", it, "--refit_iterations", it,
                                "--final_refit_posewait", "500", "--cooldown_iterations", "500", "--iterations_max", "3", "--aug_rotation", "2"])
        assert rc == 0
        outs[w] = out
    files = sorted(f for f in os.listdir(outs["1"]) if f.startswith("poses_") and f.endswith(".txt"))
    assert "poses_final.txt" in files
    assert files == sorted(f for f in os.listdir(outs["3"]) if f.startswith("poses_") and f.endswith(".txt"))
    for f in files:
        assert (outs["1"] / f).read_bytes() == (outs["3"] / f).read_bytes(), f
