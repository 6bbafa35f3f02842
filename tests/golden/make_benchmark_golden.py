"""Fixtures of benchmark_poses.py from the REFERENCE's benchmarks/preprocess_data.py and benchmarks/benchmark_poses.py ->
tests/golden/benchmark_transforms.json and tests/golden/benchmark_flags.json. Build container only (needs /root/reference, scipy, Pillow).

benchmark_transforms.json holds the inputs this script made up (20 tiny PNGs of one size, a 20-line pose file: two lines below
confidence 1000, one line for a file that is not in the folder, so one image has no pose; a split file) and the transforms.json the
reference's convert_ace_zero_to_nerf_blender_format wrote for them, once with the default split and once with the split file.
benchmark_flags.json holds the parser's surface: flags, type, default, choices, required. Data the reference writes; none of its text.

    python tests/golden/make_benchmark_golden.py
"""
import argparse
import json
import os
import runpy
import sys
import tempfile
from pathlib import Path

import numpy as np
from PIL import Image
from scipy.spatial.transform import Rotation

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

H, W, N = 12, 16, 20


def make_inputs():
    rng = np.random.default_rng(20)
    names = [f"imgs/f_{i:02d}.png" for i in range(N)]
    lines = []
    for i in range(N):
        name = names[i] if i != 7 else "imgs/not_in_folder.png"         # image 7 has no pose
        q = Rotation.from_rotvec(rng.normal(0, 0.4, 3)).as_quat()       # xyzw
        t = rng.normal(0, 1.5, 3)
        conf = 999 if i == 3 else 17 if i == 12 else 1000 if i == 5 else int(rng.integers(1001, 5000))
        lines.append(f"{name} {q[3]} {q[0]} {q[1]} {q[2]} {t[0]} {t[1]} {t[2]} {20.0 + 0.25 * (i % 3)} {conf}")
    split = {"train_filenames": [n for i, n in enumerate(names) if i % 5 != 2], "test_filenames": [n for i, n in enumerate(names) if i % 5 == 2]}
    return names, "\n".join(lines) + "\n", split


def write_inputs(root, names, pose_text, split):
    os.makedirs(os.path.join(root, "imgs"), exist_ok=True)
    for i, n in enumerate(names):
        Image.fromarray(np.full((H, W, 3), 10 * i, np.uint8)).save(os.path.join(root, n))
    with open(os.path.join(root, "poses.txt"), "w") as f:
        f.write(pose_text)
    with open(os.path.join(root, "split.json"), "w") as f:
        json.dump(split, f)


def parser_surface():
    box = {}

    class Captured(Exception):
        pass

    def fake_parse(self, *a, **k):
        box["p"] = self
        raise Captured()
    orig = argparse.ArgumentParser.parse_args
    argparse.ArgumentParser.parse_args = fake_parse
    try:
        runpy.run_path(os.path.join(REF, "benchmarks", "benchmark_poses.py"), run_name="__main__")
    except Captured:
        pass
    finally:
        argparse.ArgumentParser.parse_args = orig
    out = {}
    for act in box["p"]._actions:
        if act.dest == "help":
            continue
        out[act.dest] = {"flags": list(act.option_strings), "type": act.type.__name__ if act.type else None, "default": act.default,
                         "choices": list(act.choices) if act.choices else None, "required": bool(act.required),
                         "store_true": isinstance(act, argparse._StoreTrueAction)}
    return out


if __name__ == "__main__":
    from benchmarks.preprocess_data import convert_ace_zero_to_nerf_blender_format   # the reference's
    names, pose_text, split = make_inputs()
    res = {"image_size": [H, W], "images": names, "pose_file": pose_text, "split": split}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        write_inputs(d, names, pose_text, split)
        os.chdir(d)
        try:
            for key, sp in (("default", None), ("with_split", Path("split.json"))):
                os.makedirs(key)
                convert_ace_zero_to_nerf_blender_format(poses_path=Path("poses.txt"), images_glob_pattern="imgs/*.png", output_path=Path(key),
                                                        split_file_path=sp)
                with open(os.path.join(key, "transforms.json")) as f:
                    res[key] = json.load(f)
        finally:
            os.chdir(cwd)
    with open(os.path.join(HERE, "benchmark_transforms.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    with open(os.path.join(HERE, "benchmark_flags.json"), "w") as f:
        json.dump(parser_surface(), f, indent=1, sort_keys=True)
    print({k: (len(v["frames"]), len(v["train_filenames"]), len(v["test_filenames"])) for k, v in res.items() if isinstance(v, dict) and "frames" in v})
