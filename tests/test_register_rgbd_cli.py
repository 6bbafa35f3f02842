"""CPU: register_mapping_rgbd.py's command line is register_mapping.py's plus a required --depth_files, and a depth-file count that
differs from the image count ends the run with a clear message before any frame is encoded."""
import os
import subprocess
import sys

import numpy as np
import pytest

from acezero_amd import cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _surface(parser):
    return {a.dest: (list(a.option_strings), a.default, list(a.choices) if a.choices else None, a.required)
            for a in parser._actions if a.dest != "help"}


def test_parser_is_register_mapping_plus_depth_files():
    base, rgbd = _surface(cli.register_parser()), _surface(cli.register_rgbd_parser())
    assert set(rgbd) - set(base) == {"depth_files"}
    assert all(rgbd[k] == v for k, v in base.items())
    assert rgbd["depth_files"][0] == ["--depth_files"] and rgbd["depth_files"][3]
    with pytest.raises(SystemExit):
        cli.register_rgbd_parser().parse_args(["rgb/*.png", "map.pt"])          # --depth_files is required
    opt = cli.register_rgbd_parser().parse_args(["rgb/*.png", "map.pt", "--depth_files", "d/*.png", "-t", "5", "-maxerrr", "50"])
    assert (opt.depth_files, opt.threshold, opt.maxpixelerror, opt.hypotheses) == ("d/*.png", 5.0, 50.0, 64)


def _files(tmp_path, n_rgb, n_depth):
    from PIL import Image
    for i in range(n_rgb):
        Image.fromarray(np.zeros((48, 64, 3), np.uint8)).save(tmp_path / f"rgb_{i:03d}.png")
    for i in range(n_depth):
        Image.fromarray(np.full((48, 64), 1500, np.uint16)).save(tmp_path / f"depth_{i:03d}.png")


@pytest.mark.parametrize("n_depth", [2, 4])
def test_depth_count_mismatch_is_a_clear_error(tmp_path, n_depth):
    _files(tmp_path, 3, n_depth)
    with pytest.raises(SystemExit) as e:
        cli.register_rgbd_main([str(tmp_path / "rgb_*.png"), str(tmp_path / "map.pt"), "--depth_files", str(tmp_path / "depth_*.png")])
    assert f"--depth_files matches {n_depth} files for 3 images" in str(e.value)


def test_script_reports_the_mismatch(tmp_path):
    _files(tmp_path, 2, 1)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "register_mapping_rgbd.py"), str(tmp_path / "rgb_*.png"), str(tmp_path / "map.pt"),
                        "--depth_files", str(tmp_path / "depth_*.png")], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and "--depth_files matches 1 files for 2 images" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "register_mapping_rgbd.py"), "--help"], capture_output=True, text=True, cwd=ROOT,
                       timeout=300)
    assert r.returncode == 0 and "--depth_files" in r.stdout and "CENTIMETRES" in r.stdout


def test_feature_file_is_refused(tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.register_rgbd_main(["rgb/*.png", str(tmp_path / "map.pt"), "--depth_files", "d/*.png", "--feature_file", "f.npz"])
    assert "--feature_file" in str(e.value)
