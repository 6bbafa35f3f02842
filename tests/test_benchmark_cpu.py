"""CPU: benchmark_poses.py's host half (the data set the reference writes for nerfstudio: flags, pose conversion, frames, split,
refusals) against fixtures of the reference's own output, and the numpy restatement of the reprojection score
(tests/reproject_restated.py) against expectations written down by hand -- the definition the GPU tests compare the kernels with."""
import json
import math
import os

import numpy as np
import pytest
from PIL import Image

from acezero_amd import benchmark, cli
from tests import reproject_cases as cases
from tests import reproject_restated as rr

ADDED_FLAGS = {"network", "encoder_path", "image_resolution", "depth_band", "use_half", "compute_dtype"}


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "benchmark_transforms.json")) as f:
        return json.load(f)


def _write_inputs(root, golden):
    h, w = golden["image_size"]
    os.makedirs(root / "imgs", exist_ok=True)
    for i, name in enumerate(golden["images"]):
        Image.fromarray(np.full((h, w, 3), 10 * i, np.uint8)).save(root / name)
    (root / "poses.txt").write_text(golden["pose_file"])
    (root / "split.json").write_text(json.dumps(golden["split"]))


# ---------------------------------------------------------------------------------------------------------------- flags
def test_flags_are_the_references_plus_the_documented_additions(golden_dir):
    with open(os.path.join(golden_dir, "benchmark_flags.json")) as f:
        ref = json.load(f)
    mine = {a.dest: a for a in cli.benchmark_poses_parser()._actions if a.dest != "help"}
    assert set(mine) - set(ref) == ADDED_FLAGS
    for dest, spec in ref.items():
        a = mine[dest]
        assert list(a.option_strings) == spec["flags"], dest
        assert (a.type.__name__ if a.type else None) == spec["type"], dest
        assert bool(a.required) == spec["required"], dest
        assert type(a).__name__ == ("_StoreTrueAction" if spec["store_true"] else "_StoreAction"), dest
        if dest == "method":                                             # the one documented change: a third choice, the default here
            assert list(a.choices) == ["reproject"] + spec["choices"] and a.default == "reproject"
            continue
        assert (list(a.choices) if a.choices else None) == spec["choices"], dest
        assert a.default == spec["default"], dest
    opt = cli.benchmark_poses_parser().parse_args(["--pose_file", "p", "--output_dir", "o", "--images_glob_pattern", "g"])
    assert (opt.image_resolution, opt.depth_band, opt.use_half, opt.network) == (480, 0.05, True, None)


def test_entry_script_is_a_thin_wrapper():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "benchmark_poses.py")).read()
    assert "from acezero_amd.cli import benchmark_poses_main" in text and "sys.exit(benchmark_poses_main())" in text


# ------------------------------------------------------------------------------------------------------ transforms.json
def _same_transforms(mine, ref):
    assert set(mine) == set(ref)
    a, b = {fr["file_path"]: fr for fr in mine["frames"]}, {fr["file_path"]: fr for fr in ref["frames"]}
    assert set(a) == set(b) and len(mine["frames"]) == len(ref["frames"])
    for name, fr in b.items():
        assert set(a[name]) == set(fr), name
        for key, val in fr.items():
            if key == "transform_matrix":
                assert np.abs(np.array(a[name][key]) - np.array(val)).max() <= 1e-12, name
            else:
                assert a[name][key] == val and type(a[name][key]) is type(val), (name, key)
    assert mine["val_filenames"] == ref["val_filenames"] == []
    return a


def test_transforms_equal_the_references_for_the_default_split(golden, tmp_path, monkeypatch):
    _write_inputs(tmp_path, golden)
    monkeypatch.chdir(tmp_path)
    mine = benchmark.make_transforms("poses.txt", "imgs/*.png")
    ref = golden["default"]
    frames = _same_transforms(mine, ref)
    assert mine["train_filenames"] == ref["train_filenames"] and mine["test_filenames"] == ref["test_filenames"]
    assert mine["test_filenames"] == sorted(golden["images"])[4::8]
    assert frames["imgs/f_07.png"]["confidence_score"] == 0.0 and frames["imgs/f_07.png"]["fl_x"] == golden["image_size"][0] * 0.7
    assert "imgs/f_03.png" not in mine["train_filenames"] and "imgs/f_05.png" in mine["train_filenames"]   # 999 dropped, 1000 kept


def test_transforms_equal_the_references_for_a_split_file(golden, tmp_path, monkeypatch):
    _write_inputs(tmp_path, golden)
    monkeypatch.chdir(tmp_path)
    mine = benchmark.make_transforms("poses.txt", "imgs/*.png", "split.json")
    ref = golden["with_split"]
    _same_transforms(mine, ref)
    # the lists follow the order of `frames`, which is the order glob returns the files in on the machine that wrote them
    order = [fr["file_path"] for fr in mine["frames"]]
    for key in ("train_filenames", "test_filenames"):
        assert sorted(mine[key]) == sorted(ref[key]), key
        assert mine[key] == [n for n in order if n in set(mine[key])], key
    # a frame in neither list
    part = dict(golden["split"], test_filenames=golden["split"]["test_filenames"][1:])
    (tmp_path / "part.json").write_text(json.dumps(part))
    with pytest.raises(Exception, match="not found in split file"):
        benchmark.make_transforms("poses.txt", "imgs/*.png", "part.json")


def test_pose_conversion_by_hand():
    # identity: the camera sits at the origin; OpenGL's camera looks down -z with y up, so the y and z axes flip
    T = benchmark.transform_matrix_from_pose([1, 0, 0, 0], [0, 0, 0])
    assert np.array_equal(T, np.diag([1.0, -1.0, -1.0, 1.0]))
    # world -> camera: 90 degrees about y, then t = (1, 2, 3). R = [[0,0,1],[0,1,0],[-1,0,0]]; centre = -R^T t = (3, -2, -1);
    # camera -> world rotation R^T = [[0,0,-1],[0,1,0],[1,0,0]], its y and z columns negated for OpenGL
    s = math.sqrt(0.5)
    T = benchmark.transform_matrix_from_pose([s, 0, s, 0], [1, 2, 3])
    want = np.array([[0, 0, 1, 3], [0, -1, 0, -2], [1, 0, 0, -1], [0, 0, 0, 1.0]])
    assert np.abs(T - want).max() < 1e-15
    back = benchmark.pose_from_transform_matrix(T)
    assert np.abs(back - np.array([[0, 0, 1, 1], [0, 1, 0, 2], [-1, 0, 0, 3], [0, 0, 0, 1.0]])).max() < 1e-15


def test_confidence_threshold_is_inclusive(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    os.makedirs("im")
    lines = []
    for i in range(6):
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(f"im/{i}.png")
        lines.append(f"im/{i}.png 1 0 0 0 0 0 {i} 10.0 {[1000, 999, 1001, 0, 5000, 1000][i]}")
    (tmp_path / "p.txt").write_text("\n".join(lines) + "\n")
    tr = benchmark.make_transforms("p.txt", "im/*.png")
    assert tr["test_filenames"] == ["im/4.png"] and tr["train_filenames"] == ["im/0.png", "im/2.png", "im/5.png"]


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    os.makedirs("im")
    for i in range(6):
        Image.fromarray(np.zeros((8, 8 if i else 16, 3), np.uint8)).save(f"im/{i}.png")
    (tmp_path / "p.txt").write_text("".join(f"im/{i}.png 1 0 0 0 0 0 0 10.0 {2000 if i > 1 else 10}\n" for i in range(6)))
    with pytest.raises(AssertionError, match="all resolutions equal"):           # mixed frame sizes
        benchmark.make_transforms("p.txt", "im/*.png")
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save("im/0.png")
    assert len(benchmark.make_transforms("p.txt", "im/*.png")["train_filenames"]) == 3
    (tmp_path / "low.txt").write_text("".join(f"im/{i}.png 1 0 0 0 0 0 0 10.0 999\n" for i in range(6)))
    with pytest.raises(AssertionError, match="[Nn]o train filenames"):           # every train frame below the threshold
        benchmark.make_transforms("low.txt", "im/*.png")
    base = ["--pose_file", "p.txt", "--output_dir", str(tmp_path / "out"), "--images_glob_pattern", "im/*.png"]
    for method in ("nerfacto", "splatfacto"):
        with pytest.raises(SystemExit, match="nerfstudio"):
            cli.benchmark_poses_main(base + ["--method", method])
    with pytest.raises(SystemExit, match="camera_optimizer"):
        cli.benchmark_poses_main(base + ["--camera_optimizer", "SE3"])
    with pytest.raises(SystemExit, match="use_half False"):
        cli.benchmark_poses_main(base + ["--use_half", "False"])
    assert not (tmp_path / "out").exists()                                        # refused on the arguments alone


def test_dry_run_writes_the_data_set(tmp_path, monkeypatch):
    """--method nerfacto --no_run_nerfstudio: transforms.json with absolute paths, the copied point cloud, the down-scaled frames."""
    monkeypatch.chdir(tmp_path)
    os.makedirs("im/sub")
    names = [f"im/sub/{i:02d}.png" for i in range(10)]
    for i, n in enumerate(names):
        Image.fromarray(np.full((20, 30, 3), i, np.uint8)).save(n)
    (tmp_path / "p.txt").write_text("".join(f"{n} 1 0 0 0 0 0 0 25.0 2000\n" for n in names))
    (tmp_path / "pc_final.ply").write_bytes(b"ply\n")
    rc = cli.benchmark_poses_main(["--pose_file", "p.txt", "--output_dir", "out", "--images_glob_pattern", "im/sub/*.png", "--method", "nerfacto",
                                   "--no_run_nerfstudio", "--max_resolution", "10"])
    assert rc == 0 and not (tmp_path / "out" / "results_reproject.json").exists()
    tr = json.load(open(tmp_path / "out" / "nerf_data" / "transforms.json"))
    assert tr["ply_file_path"] == "pc_final.ply" and (tmp_path / "out" / "nerf_data" / "pc_final.ply").read_bytes() == b"ply\n"
    assert benchmark.downscale_factor(20, 30, 10) == 3 and benchmark.downscale_factor(480, 640, 640) == 1
    small = tmp_path / "out" / "nerf_data" / "images_3"
    assert sorted(os.listdir(small)) == [f"im_sub_{i:02d}.png" for i in range(10)]
    assert Image.open(small / "im_sub_04.png").size == (10, 6)
    paths = {fr["file_path"] for fr in tr["frames"]}
    assert paths == {str(small / f"im_sub_{i:02d}.png") for i in range(10)} and all(os.path.isabs(p) for p in paths)
    assert tr["test_filenames"] == [str(small / "im_sub_04.png")] and len(tr["train_filenames"]) == 9 and set(tr["train_filenames"]) < paths
    assert tr["frames"][0]["w"] == 30 and tr["frames"][0]["fl_x"] == 25.0        # intrinsics stay those of the original frames


# ------------------------------------------------------------------------------------------- the restated definition
def _image_of(expect):
    img, mask = np.zeros((cases.OH, cases.OW, 3), np.uint8), np.zeros((cases.OH, cases.OW), np.uint8)
    for (r, c), col in expect.items():
        img[r, c], mask[r, c] = col, 1
    return img, mask


def test_restated_constructed_scene():
    (pts, clr, views, targets, band), expect0 = cases.constructed_scene()
    sse, cov, image, mask = rr.score_views(pts, clr, views, targets, band)
    img0, mask0 = _image_of(expect0)
    assert np.array_equal(image[0], img0) and np.array_equal(mask[0], mask0)
    assert cov.tolist()[:2] == [5, 0]
    assert sse[0] == sum((v - 7) ** 2 for col in expect0.values() for v in col) and sse[1] == 0
    assert not mask[1].any() and not image[1].any()
    assert rr.psnr(sse, cov)[1] is None                                           # a view no point reaches
    # a view whose render equals its target
    targets[2] = image[2]
    sse2, cov2, _, _ = rr.score_views(pts, clr, views, targets, band)
    assert cov2[2] == cov[2] > 0 and sse2[2] == 0 and rr.psnr(sse2, cov2)[2] == math.inf
    assert rr.psnr([3 * 255 ** 2 * 4], [4])[0] == 0.0 and abs(rr.psnr([3 * 4], [4])[0] - 20 * math.log10(255)) < 1e-12
    assert benchmark.psnr_of(sse2, cov2) == rr.psnr(sse2, cov2)


def test_restated_band_limit_is_one_float32_product():
    lim = cases.band_limit()
    assert lim.dtype == np.float32 and lim == np.float32(2.0) * np.float32(1.05) and float(lim) != 2.0 * 1.05


def test_restated_edges_and_negative_zero():
    (pts, clr, views, targets, band), expect = cases.edge_scene()
    valid, cell, _ = rr.project(pts, views[0], cases.OH, cases.OW)
    assert valid.tolist() == [True, False, False, True, False, True, False]
    m = views[0]
    u0 = m[13] + (m[12] * (((m[0] * pts[0, 0] + m[1] * pts[0, 1]) + m[2] * pts[0, 2]) + m[3])) * (np.float32(1) / pts[0, 2])
    assert u0 == 0 and np.signbit(u0)                                             # the projection IS -0.0, and it is cell 0
    assert cell[[0, 3, 5]].tolist() == [2 * cases.OW, 2 * cases.OW + 7, 5 * cases.OW + 2]
    sse, cov, image, mask = rr.score_views(pts, clr, views, targets, band)
    img, msk = _image_of(expect)
    assert np.array_equal(image[0], img) and np.array_equal(mask[0], msk) and cov[0] == 3 and sse[0] == 3 * (100 + 400 + 900)


def test_restated_does_not_depend_on_point_order():
    pts, clr, views, targets, band = cases.random_case(1000)
    a = rr.score_views(pts, clr, views, targets, band)
    perm = np.random.default_rng(1).permutation(len(pts))
    b = rr.score_views(pts[perm], clr[perm], views, targets, band)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[1].min() > 0


def test_restated_cell_means():
    rng = np.random.default_rng(3)
    fr = rng.integers(0, 256, (2, 19, 27, 3)).astype(np.uint8)                    # ragged: the last cells are 3 rows / 3 columns
    m = rr.cell_means(fr)
    assert m.shape == (2, 3, 4, 3)
    for (f, r, c) in [(0, 0, 0), (1, 2, 3), (0, 2, 0), (1, 0, 3)]:
        blk = fr[f, r * 8:(r + 1) * 8, c * 8:(c + 1) * 8].reshape(-1, 3).astype(np.float64)
        assert np.array_equal(m[f, r, c], np.floor(blk.mean(0) + 0.5).astype(np.uint8))
    assert fr[1, 16:, 24:].shape[:2] == (3, 3)
    half = np.zeros((1, 8, 8, 3), np.uint8)
    half[0, :4] = 1                                                               # mean exactly 0.5: goes up
    assert rr.cell_means(half)[0, 0, 0].tolist() == [1, 1, 1]


def test_make_views_agree():
    rng = np.random.default_rng(5)
    w2c = rng.normal(size=(4, 3, 4))
    f = rng.uniform(400, 600, 4)
    assert np.array_equal(benchmark.make_views(w2c, f, 320.0, 240.0).view(np.uint32), rr.make_views(w2c, f, 320.0, 240.0).view(np.uint32))
    assert rr.make_views(w2c, 525.0, 320.0, 240.0)[0, 12:].tolist() == [np.float32(525 / 8), 40.0, 30.0]


def test_scorer_has_no_cpu_path():
    import torch
    with pytest.raises(RuntimeError, match="no CPU path"):
        benchmark.score_views(torch.zeros(1, 3), torch.zeros(1, 3, dtype=torch.uint8), torch.zeros(1, 15), torch.zeros(1, 6, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        benchmark.cell_means(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
