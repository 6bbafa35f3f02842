"""The parts the command lines share, below cli.py: the seeded --max_estimates subset (session.estimate_subset), the posed images of
fuse_depth.py / estimate_depth.py (formats.read_posed_images) and the pose pairs of eval_poses.py / eval_geometry.py
(evaluate.read_pose_pairs). tests/test_mixed_sizes_cpu.py holds images.session_frames' cases."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from acezero_amd import cli, dsacstar, evaluate, formats, session


@pytest.mark.parametrize("k", [0, 3, 7, 9])
def test_estimate_subset_is_the_sorted_seeded_permutation(k):
    n, seed = 7, 1305
    ids = session.estimate_subset(n, k, seed)
    if k == 0:                                                           # --max_estimates <= 0 (its default is -1): every frame
        assert np.array_equal(ids, np.arange(n))
    else:
        assert np.array_equal(ids, np.sort(torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:k].numpy()))
    assert len(ids) == (k if 0 < k < n else n) and len(set(ids.tolist())) == len(ids)


def test_register_draws_its_subset_from_estimate_subset(monkeypatch):
    """register() on a host-only skeleton (tests/test_session_rgbd_cpu.py's): registered_ids, the RNG keys and the frames that reach
    the estimator are the seeded subset under opt.register_seed."""
    class RegisterOnly(session.ReconstructionSession):
        def __init__(self, opt, n):
            self.opt, self.n, self.world, self.rank, self.group = opt, n, 1, 0, None
            self.dev, self.depth, self.timings = torch.device("cpu"), None, {"register_s": 0.0}
            self.classes = [SimpleNamespace(ids=np.arange(n), oh=6, ow=8, hw=48, ppx=32.0, ppy=24.0)]
            self.frame_class, self.frel = np.zeros(n, np.int64), np.ones(n)

        def scene_coordinates(self, head_sd, frame_ids=None):
            return torch.zeros(len(frame_ids), 3, 6, 8)

    seen = []

    def fake(sc, intrinsics, params, seed, frame_ids=None, want_masks=True):
        seen.append(list(frame_ids))
        return torch.eye(4).repeat(len(sc), 1, 1), torch.full((len(sc),), 333, dtype=torch.int32), None
    monkeypatch.setattr(dsacstar, "register_batch", fake)
    ses = RegisterOnly(session.default_options(register_seed=77), 7)
    want = np.sort(torch.randperm(7, generator=torch.Generator().manual_seed(77))[:3].numpy())
    poses, _ = ses.register({}, 500.0, max_estimates=3)
    assert np.array_equal(ses.registered_ids, want) and seen[-1] == want.tolist() and len(poses) == 3
    ses.register({}, 500.0)
    assert np.array_equal(ses.registered_ids, np.arange(7)) and seen[-1] == list(range(7))


def _pose_file(path, names, confidences, focals):
    with open(path, "w") as f:
        for k, (name, c, focal) in enumerate(zip(names, confidences, focals)):
            w2c = np.eye(4)
            w2c[:3, 3] = [k, 0, 0]
            cli.write_pose_line(f, name, w2c, c, focal)


def test_read_posed_images_maps_files_to_rows_and_refuses(tmp_path):
    """Four entries, one below the threshold; five files, one of them without a pose and one whose pose is the dropped entry."""
    _pose_file(tmp_path / "p.txt", ["seq/a.png", "seq/b.png", "seq/c.png", "seq/d.png"], [2000, 50, 3000, 1000], [500.0, 510.0, 520.0, 530.0])
    files = ["other/d.png", "seq/a.png", "seq/b.png", "seq/c.png", "seq/e.png"]
    c2w, focals, rows = formats.read_posed_images(tmp_path / "p.txt", files, 1000)
    assert rows == [2, 0, None, 1, None] and focals == [500.0, 520.0, 530.0] and c2w.shape == (3, 4, 4)   # d.png by its basename
    assert [float(-c2w[k][0, 3]) for k in rows if k is not None] == [3.0, 0.0, 2.0]                      # each file got its own entry
    with pytest.raises(ValueError, match="^no pose above the confidence threshold$"):
        formats.read_posed_images(tmp_path / "p.txt", files, 5000)
    with pytest.raises(ValueError, match="^no image of the glob has a pose above the confidence threshold in the pose file$"):
        formats.read_posed_images(tmp_path / "p.txt", ["seq/b.png", "seq/e.png"], 1000)
    assert formats.focal_at_height(500.0, 240, 480) == 500.0 * 240 / 480


def test_read_pose_pairs_zips_sorted_estimates_with_sorted_ground_truth(tmp_path):
    """Three estimates (written out of order) against two ground-truth files: two pairs, in the order of the names; three read."""
    _pose_file(tmp_path / "p.txt", ["c.png", "a.png", "b.png"], [300, 100, 200], [500.0] * 3)
    for k in range(2):
        gt = np.eye(4)
        gt[:3, 3] = [0, 10 + k, 0]
        np.savetxt(tmp_path / f"gt_{k}.txt", gt)
    est, gt, conf, n_read = evaluate.read_pose_pairs(tmp_path / "p.txt", str(tmp_path / "gt_*.txt"))
    assert n_read == 3 and est.shape == gt.shape == (2, 4, 4) and conf.tolist() == [100.0, 200.0]
    assert np.allclose(est[:, 0, 3], [-1.0, -2.0]) and gt[:, 1, 3].tolist() == [10.0, 11.0]      # a.png, b.png: cam->world of rows 1, 2
    est, gt, conf, n_read = evaluate.read_pose_pairs(tmp_path / "p.txt", str(tmp_path / "none_*.txt"))
    assert n_read == 3 and est.shape == gt.shape == (0, 4, 4) and len(conf) == 0
