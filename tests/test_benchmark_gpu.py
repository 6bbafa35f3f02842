"""GPU: the reprojection scorer of benchmark_poses.py (acezero_amd/csrc/reproject_api.hip through acezero_amd.benchmark) against
its numpy restatement bit for bit, its independence of the point order, its sensitivity to a wrong pose, and the command line end
to end on files."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from acezero_amd import benchmark, synth
from tests import reproject_cases as cases
from tests import reproject_restated as rr

pytestmark = pytest.mark.gpu


def _gpu(case, want_image=True):
    pts, clr, views, targets, band = case
    out = benchmark.score_views(torch.from_numpy(pts).cuda(), torch.from_numpy(clr).cuda(), torch.from_numpy(views).cuda(),
                                torch.from_numpy(targets).cuda(), band, want_image=want_image)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _assert_equal(case):
    got = _gpu(case)
    sse, cov, image, mask = rr.score_views(*case)
    assert got["sse"].dtype == np.int64 and got["sse"].tolist() == sse.tolist()
    assert got["covered"].tolist() == cov.tolist()
    assert np.array_equal(got["image"], image) and np.array_equal(got["mask"], mask)
    bare = _gpu(case, want_image=False)                                   # the optional outputs left out: the same numbers
    assert bare["image"] is None and bare["sse"].tolist() == sse.tolist() and bare["covered"].tolist() == cov.tolist()
    return got


@pytest.mark.parametrize("n_points", [1000, 1, 257])
def test_score_equals_the_restatement_bit_for_bit(n_points):
    got = _assert_equal(cases.random_case(n_points))
    if n_points == 1000:
        assert got["covered"].min() > 10
    # depths on a grid of 1/4: cells with several points of equal depth, and points exactly on a band limit
    _assert_equal(cases.random_case(n_points, quantise_depth=True, seed=1))


def test_many_views_take_the_grid_stride_path():
    """4096 views leave one block of 256 threads per view: 300 points go through the point loop twice."""
    got = _assert_equal(cases.random_case(300, n_views=4096, seed=2))
    assert (got["covered"] > 0).all()


def test_constructed_points():
    case, expect0 = cases.constructed_scene()
    got = _assert_equal(case)
    assert got["covered"].tolist()[:2] == [5, 0] and got["image"][0, 4, 5].tolist() == [255, 255, 255]
    assert got["image"][0, 3, 1].tolist() == [150, 150, 150] and got["image"][0, 1, 2].tolist() == [31, 40, 51]
    psnr = benchmark.psnr_of(got["sse"], got["covered"])
    assert psnr[1] is None and psnr[0] is not None
    pts, clr, views, targets, band = case
    targets = targets.copy()
    targets[2] = got["image"][2]                                          # a view whose render equals its target
    again = _assert_equal((pts, clr, views, targets, band))
    assert again["sse"][2] == 0 and again["covered"][2] > 0 and benchmark.psnr_of(again["sse"], again["covered"])[2] == math.inf
    res = benchmark.summarise(again["sse"], again["covered"], cases.OH * cases.OW)
    assert res["n_uncovered_views"] == 1 and res["psnr"][1] is None and res["coverage"][1] == 0.0 and res["mean_psnr"] == math.inf
    assert json.loads(json.dumps(res))["psnr"][1] is None


def test_edges_and_negative_zero():
    case, expect = cases.edge_scene()
    got = _assert_equal(case)
    assert got["covered"].tolist() == [3] and sorted(zip(*np.nonzero(got["mask"][0]))) == sorted(expect)


def test_no_points_at_all():
    _, _, views, targets, band = cases.random_case(10)
    got = _assert_equal((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), views, targets, band))
    assert got["covered"].tolist() == [0, 0, 0] and got["sse"].tolist() == [0, 0, 0]


def test_outputs_do_not_depend_on_the_point_order():
    pts, clr, views, targets, band = cases.random_case(1000)             # continuous depths: no two points of equal depth
    a = _gpu((pts, clr, views, targets, band))
    perm = np.random.default_rng(7).permutation(len(pts))
    b = _gpu((pts[perm], clr[perm], views, targets, band))
    c = _gpu((pts, clr, views, targets, band))
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k


@pytest.mark.parametrize("hw", [(19, 27), (16, 24)])
def test_cell_means_equal_the_restatement(hw):
    fr = np.random.default_rng(hw[0]).integers(0, 256, (3, hw[0], hw[1], 3)).astype(np.uint8)
    got = benchmark.cell_means(torch.from_numpy(fr).cuda()).cpu().numpy()
    assert got.shape == (3, (hw[0] + 7) // 8, (hw[1] + 7) // 8, 3) and np.array_equal(got, rr.cell_means(fr))


def test_invalid_arguments_are_refused_before_any_launch():
    import ctypes as C
    from acezero_amd import _native as N
    lib = N.lib()
    n = C.c_int64(0)
    assert lib.acez_reproject_scratch_size(3, 6, 8, C.byref(n)) == 0 and n.value == 3 * 48 * 24
    assert lib.acez_reproject_scratch_size(0, 6, 8, C.byref(n)) == -1 and lib.acez_reproject_scratch_size(1, 6, 4097, C.byref(n)) == -1
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    args = lambda m, band, scratch: (p, p, m, p, 3, 6, 8, p, band, p, scratch, p, p, None, None, None)   # noqa: E731
    assert lib.acez_reproject_score(*args(1, 0.05, 3 * 48 * 24 - 1)) == -1 and b"scratch" in lib.acez_last_error()
    assert lib.acez_reproject_score(*args((1 << 24) + 1, 0.05, 1 << 20)) == -1
    assert lib.acez_reproject_score(*args(1, -0.1, 1 << 20)) == -1


def test_true_poses_score_above_turned_poses():
    """The property users rely on: a held-out pose that is wrong by 2 degrees scores clearly worse. On the synthetic room
    (tests/reproject_cases.sensitivity_scene: 12 frames of 192 x 256 px, frame 4 held out, 8448 source points from the true geometry)
    the numpy restatement gives 35.19 dB for the true pose and 20.00 dB for the pose turned by 2 degrees about the vertical axis, both
    with every cell covered (0.5 / 1 / 4 degrees: 29.04 / 24.81 / 15.72 dB). The device result is bit-identical to the restatement
    (the tests above), so half of the measured gap of 15.2 dB is asserted: room for a changed generator, not for a broken kernel."""
    pts, clr, v_true, v_turn, targets = cases.sensitivity_scene()
    score = {}
    for name, views in (("true", v_true), ("turned", v_turn)):
        out = _gpu((pts, clr, views, targets, 0.05), want_image=False)
        score[name] = benchmark.summarise(out["sse"], out["covered"], targets.shape[1] * targets.shape[2])
    print("sensitivity:", {k: (v["mean_psnr"], v["mean_coverage"]) for k, v in score.items()})
    assert score["true"]["n_uncovered_views"] == 0 and score["true"]["mean_coverage"] >= 0.5
    assert score["true"]["mean_psnr"] - score["turned"]["mean_psnr"] >= 0.5 * (35.19 - 20.00)


def _last_head(out):
    ks = [int(m.group(1)) for m in (re.match(r"iteration(\d+)\.pt$", f) for f in os.listdir(out)) if m]
    return f"iteration{max(ks)}.pt"


def test_benchmark_poses_script_end_to_end(tmp_path):
    """ace_zero.py on a folder of PNG frames, then benchmark_poses.py on its poses_final.txt and its last head: the written results
    have the documented schema and are the numbers score_views gives for the same inputs."""
    from PIL import Image
    from acezero_amd import cli
    seq = synth.render_room_sequence(seed=7, n_frames=48, arc_deg=24.0, device="cuda")
    img = ((seq["images"][:, 0] * 0.25 + 0.4).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
    dep = (seq["depth"].cpu().numpy() * 1000).round().astype(np.uint16)
    for i in range(len(img)):
        Image.fromarray(np.stack([img[i]] * 3, -1)).save(tmp_path / f"rgb_{i:04d}.png")
        Image.fromarray(np.kron(dep[i], np.ones((8, 8), np.uint16))).save(tmp_path / f"depth_{i:04d}.png")
    torch.save({k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}, tmp_path / "encoder.pt")
    out = tmp_path / "result"
    it = "2500"
    rc = cli.ace_zero_main([str(tmp_path / "rgb_*.png"), str(out), "--depth_files", str(tmp_path / "depth_*.png"), "--encoder_path",
                            str(tmp_path / "encoder.pt"), "--use_external_focal_length", str(seq["focal"]), "--try_seeds", "1",
                            "--seed_iterations", it, "--refit_iterations", it, "--final_refit_posewait", "500", "--cooldown_iterations", "500",
                            "--iterations_max", "6", "--aug_rotation", "2", "--export_point_cloud", "True"])
    assert rc == 0
    head = out / _last_head(out)
    bench = tmp_path / "bench"
    rc = cli.benchmark_poses_main(["--pose_file", str(out / "poses_final.txt"), "--images_glob_pattern", str(tmp_path / "rgb_*.png"),
                                   "--output_dir", str(bench), "--network", str(head), "--encoder_path", str(tmp_path / "encoder.pt")])
    assert rc == 0
    tr = json.load(open(bench / "nerf_data" / "transforms.json"))
    assert tr["ply_file_path"] == "pc_final.ply" and len(tr["frames"]) == 48
    res = json.load(open(bench / "results_reproject.json"))
    n_test = (48 - 4 + 7) // 8
    assert res["n_test"] == n_test == len(tr["test_filenames"]) and res["test_filenames"] == tr["test_filenames"]
    for key in ("psnr", "coverage", "sse", "covered_cells"):
        assert len(res[key]) == n_test, key
    assert res["n_train_used"] == len(tr["train_filenames"]) > 0 and res["n_points"] > 0 and res["cells"] == [60, 80]
    assert "reprojection PSNR at 1/8 resolution" in res["metric"] and "not nerfacto" in res["metric"]
    assert res["n_uncovered_views"] == sum(p is None for p in res["psnr"])
    # the same inputs through score_views directly
    points, colours, views, targets, info = benchmark.reproject_inputs(bench / "nerf_data" / "transforms.json", head, tmp_path / "encoder.pt")
    direct = benchmark.score_views(points, colours, views, targets, 0.05)
    want = benchmark.summarise(direct["sse"].cpu().numpy(), direct["covered"].cpu().numpy(), 60 * 80)
    assert info["n_points"] == res["n_points"]
    for key in ("psnr", "coverage", "sse", "covered_cells", "mean_psnr", "mean_coverage", "n_uncovered_views"):
        assert res[key] == want[key], key
    assert res["mean_coverage"] > 0
    print("end to end:", res["mean_psnr"], res["mean_coverage"], res["n_points"], res["n_train_used"])
