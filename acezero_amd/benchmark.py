"""benchmark_poses.py: score a pose file by view synthesis (the reference's benchmarks/ folder).

Host half (no GPU): the data set the reference writes for nerfstudio -- benchmarks/preprocess_data.py and the dry-run half of
benchmarks/run_benchmark.py: `<output_dir>/nerf_data/transforms.json` (+ pc_final.ply, + images_<N>/ when the frames exceed
--max_resolution). Every 8th frame is held out, train frames below confidence 1000 are dropped.

GPU half (--method reproject, the default here): the reference fits a NeRF to the train frames in nerfstudio and reports the PSNR of
the held-out views; nerfstudio is not part of this package. `reproject` instead renders every held-out view from the OTHER frames'
coloured geometry -- the point cloud of the given head over the train frames (acez_point_cloud_filter with its defaults), every point
coloured with the mean of its own 8 x 8 px cell -- at the held-out view's pose and focal on the grid of the scene-coordinate map,
and compares it with the held-out frame's cell means (acez_reproject_score, include/acez.h section J). The result is a PSNR over the
covered cells at 1/8 resolution: a measure of whether poses, map and images agree, NOT the reference's nerfacto PSNR and not
comparable with published numbers. Like NeRF PSNR it cannot see a global similarity or a consistent drift of focal and scale.
There is no CPU path for the scorer.
"""
import glob
import json
import logging
import math
import shutil
from pathlib import Path

import numpy as np

from .formats import pose_matrix, read_pose_file

_logger = logging.getLogger("acezero_amd.benchmark")

TRAIN_CONFIDENCE = 1000        # train frames below it are left out of the fit
SAMPLE_INTERVAL = 8            # every 8th frame is a test frame, from index SAMPLE_INTERVAL // 2 on
MAX_TEST_IMAGES = 1000
METRIC = ("reprojection PSNR at 1/8 resolution: held-out frames' 8x8-cell means against the train frames' coloured point cloud seen "
          "from the held-out poses, over the covered cells (not nerfacto / splatfacto PSNR; not comparable with published numbers)")
GL_FROM_CV = np.diag([1.0, -1.0, -1.0, 1.0])


# ------------------------------------------------------------------------------------------------------ pose conversion
def parse_pose_file(path):
    """An ACE0 pose file: [(file, world -> camera 4 x 4 (OpenCV), focal, confidence)], one per line of ten fields. The confidence is
    an integer literal, as transforms.json keeps it: anything else (inf included) is a ValueError."""
    return [(e.file, e.w2c, e.focal, int(e.confidence_text)) for e in read_pose_file(path)]


def transform_matrix_from_pose(q_wxyz, t):
    """World -> camera (OpenCV: x right, y down, z forward) quaternion + translation -> camera -> world 4 x 4 in the OpenGL / Blender
    convention (x right, y up, z back) nerfstudio reads."""
    return np.linalg.inv(GL_FROM_CV @ pose_matrix(q_wxyz, t))


def pose_from_transform_matrix(transform_matrix):
    """The way back: camera -> world (OpenGL) 4 x 4 -> world -> camera (OpenCV) 4 x 4 float64."""
    return GL_FROM_CV @ np.linalg.inv(np.asarray(transform_matrix, np.float64))


# --------------------------------------------------------------------------------------------------------------- frames
def _image_size(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.height, im.width


def build_frames(pose_file, images_glob_pattern):
    """transforms.json's `frames`: one per globbed image, in glob order; an image without a pose gets the identity, 0.7 * height as
    focal and confidence 0."""
    images = [Path(p) for p in glob.glob(images_glob_pattern)]
    assert len(images) > 0, "Expected at least one frame"
    by_file = {}
    for file, w2c, focal, conf in parse_pose_file(pose_file):
        by_file[file] = {"file_path": file, "transform_matrix": np.linalg.inv(GL_FROM_CV @ w2c).tolist(), "confidence_score": conf,
                         "fl_x": focal, "fl_y": focal}
    sizes = [_image_size(p) for p in images]
    assert len(set(sizes)) == 1, f"Expected all resolutions equal, but got {sorted(set(sizes))} (height, width)"
    h, w = sizes[0]
    frames = []
    for p in images:
        fr = by_file.get(str(p))
        if fr is None:
            _logger.warning(f"No pose found for frame {p}; using identity pose instead!")
            fr = {"file_path": str(p), "transform_matrix": np.eye(4).tolist(), "fl_x": h * 0.7, "fl_y": h * 0.7, "confidence_score": 0.0}
        fr.update({"k1": 0.0, "k2": 0.0, "p1": 0.0, "p2": 0.0, "cx": w / 2.0, "cy": h / 2.0, "w": w, "h": h})
        frames.append(fr)
    return frames


def split_every_nth(frames, sample_interval=SAMPLE_INTERVAL):
    """The default split: the frames sorted by file, every sample_interval-th one from index sample_interval // 2 on is a test frame."""
    ordered = sorted(frames, key=lambda fr: fr["file_path"])
    test = set(range(len(frames))[int(sample_interval / 2)::sample_interval])
    return {"train": [ordered[i] for i in range(len(ordered)) if i not in test], "test": [ordered[i] for i in sorted(test)]}


def split_from_file(frames, split_json):
    """A given split ({"train_filenames": [...], "test_filenames": [...]}), in frame order; a frame in neither list is an error."""
    with open(split_json) as f:
        given = json.load(f)
    train_names, test_names = set(given["train_filenames"]), set(given["test_filenames"])
    out = {"train": [], "test": []}
    for fr in frames:
        if fr["file_path"] in train_names:
            out["train"].append(fr)
        elif fr["file_path"] in test_names:
            out["test"].append(fr)
        else:
            raise Exception(f"Frame {fr} not found in split file {split_json}")
    return out


def make_transforms(pose_file, images_glob_pattern, split_json=None):
    """The transforms.json dict (without ply_file_path)."""
    frames = build_frames(pose_file, images_glob_pattern)
    split = split_from_file(frames, split_json) if split_json is not None else split_every_nth(frames)
    train = [fr for fr in split["train"] if fr["confidence_score"] >= TRAIN_CONFIDENCE]
    out = {"frames": frames, "train_filenames": [fr["file_path"] for fr in train], "val_filenames": [],
           "test_filenames": [fr["file_path"] for fr in split["test"]]}
    assert len(out["train_filenames"]) > 0, "No train filenames! Must have at least one"
    return out


def downscale_factor(height, width, max_resolution):
    """The smallest integer factor that brings both sides to max_resolution or below."""
    d = 1
    while height // d > max_resolution or width // d > max_resolution:
        d += 1
    return d


def write_dataset(pose_file, images_glob_pattern, output_dir, split_json=None, max_resolution=640):
    """What the reference's dry run leaves in output_dir: nerf_data/transforms.json (absolute paths, at most 1000 test frames),
    nerf_data/pc_final.ply if one lies beside the pose file, nerf_data/images_<N>/ with the frames down-scaled by N if a side exceeds
    max_resolution. Returns (path of transforms.json, down-scale factor)."""
    from PIL import Image
    pose_file, output_dir = Path(pose_file), Path(output_dir)
    output_dir.mkdir(exist_ok=True)
    data_dir = output_dir / "nerf_data"
    data_dir.mkdir(exist_ok=True)
    tr = make_transforms(pose_file, images_glob_pattern, split_json)
    assert len(tr["test_filenames"]) > 0, "No test filenames! Must have at least one"
    cloud = pose_file.parent / "pc_final.ply"
    if cloud.exists():
        shutil.copy(cloud, data_dir / "pc_final.ply")
        tr["ply_file_path"] = "pc_final.ply"
    tests = sorted(tr["test_filenames"])
    if len(tests) > MAX_TEST_IMAGES:                                      # keeps the evaluation bounded
        tr["test_filenames"] = tests[::len(tests) // MAX_TEST_IMAGES]
        _logger.info(f"The test set is subsampled: {len(tests)} -> {len(tr['test_filenames'])} images")
    factor = downscale_factor(tr["frames"][0]["h"], tr["frames"][0]["w"], max_resolution)
    renamed = {}
    if factor > 1:                                                       # blender-style data sets keep them in images_<N>, flat
        small = data_dir / f"images_{factor}"
        small.mkdir(exist_ok=True)
        written = set()
        for fr in tr["frames"]:
            src = Path(fr["file_path"])
            dst = small / src.as_posix().replace("/", "_")
            assert dst not in written, f"Internal error: output file {dst} already exists"
            written.add(dst)
            with Image.open(src) as im:
                im.resize((im.width // factor, im.height // factor)).save(dst)
            renamed[fr["file_path"]] = str(dst)
    for fr in tr["frames"]:                                              # absolute paths, in the frames and in the lists
        now = Path(renamed.get(fr["file_path"], fr["file_path"]))
        renamed[fr["file_path"]] = str(now if now.is_absolute() else now.resolve())
        fr["file_path"] = renamed[fr["file_path"]]
    for key in ("train_filenames", "test_filenames"):
        tr[key] = [renamed[name] for name in tr[key]]
    path = data_dir / "transforms.json"
    with open(path, "w") as f:
        json.dump(tr, f, indent=4)
    _logger.info(f"Wrote {path}: {len(tr['frames'])} frames, {len(tr['train_filenames'])} train, {len(tr['test_filenames'])} test, "
                 f"down-scale factor {factor}")
    return path, factor


# --------------------------------------------------------------------------------------------------------------- scorer
def make_views(w2c, focal_px, ppx_px, ppy_px, sub=8):
    """View records of acez_reproject_score, float32 numpy [T,15]: 3 x 4 world -> camera rows (OpenCV), then focal, cx, cy in cell
    units (pixels / sub, divided in float64 and rounded once). w2c [T,3,4] or [T,4,4]; focal and principal point scalars or [T]."""
    w2c = np.asarray(w2c, np.float64)
    w2c = w2c.reshape(-1, w2c.shape[-2], 4)[:, :3]
    T = w2c.shape[0]
    out = np.zeros((T, 15), np.float32)
    out[:, :12] = w2c.reshape(T, 12).astype(np.float32)
    for k, v in enumerate((focal_px, ppx_px, ppy_px)):
        out[:, 12 + k] = (np.broadcast_to(np.asarray(v, np.float64), (T,)) / sub).astype(np.float32)
    return out


def cell_means(frames):
    """uint8 device tensor [n,H,W,3] -> uint8 [n,ceil(H/8),ceil(W/8),3] cell means (acez_reproject_cell_means)."""
    import torch
    from . import _native as N
    from ._device import ptr as _ptr, stream as _stream
    if not (torch.is_tensor(frames) and frames.is_cuda):
        raise RuntimeError("cell_means needs a device tensor: it is a HIP kernel, there is no CPU path")
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
    fr = frames.contiguous()
    n, H, W, _ = fr.shape
    out = torch.empty((n, (H + 7) // 8, (W + 7) // 8, 3), dtype=torch.uint8, device=fr.device)
    N.check(N.lib().acez_reproject_cell_means(_ptr(fr), n, H, W, _ptr(out), _stream()))
    return out


def score_views(points, colours, views, targets, depth_band=0.05, want_image=True):
    """acez_reproject_score on device tensors: points [M,3] float32, colours [M,3] uint8, views [T,15] float32 (make_views), targets
    [T,oh,ow,3] uint8. Returns {"sse": int64 [T], "covered": int32 [T], "image": uint8 [T,oh,ow,3], "mask": uint8 [T,oh,ow]} on the
    device (image and mask None without want_image)."""
    import ctypes as C
    import torch
    from . import _native as N
    from ._device import no_cpu, ptr as _ptr, stream as _stream
    if not (torch.is_tensor(targets) and targets.is_cuda):
        raise no_cpu("score_views", "the scorer is a HIP kernel")
    dev = targets.device
    tg = targets.to(torch.uint8).contiguous()
    T, oh, ow, _ = tg.shape
    pts = torch.as_tensor(points).to(dev, torch.float32).reshape(-1, 3).contiguous()
    clr = torch.as_tensor(colours).to(dev, torch.uint8).reshape(-1, 3).contiguous()
    vw = torch.as_tensor(views).to(dev, torch.float32).reshape(-1, 15).contiguous()
    if vw.shape[0] != T or clr.shape[0] != pts.shape[0]:
        raise ValueError(f"{vw.shape[0]} views for {T} targets, {clr.shape[0]} colours for {pts.shape[0]} points")
    need = C.c_int64(0)
    N.check(N.lib().acez_reproject_scratch_size(T, oh, ow, C.byref(need)))
    scratch = torch.empty((need.value // 8,), dtype=torch.int64, device=dev)
    sse = torch.empty((T,), dtype=torch.int64, device=dev)
    covered = torch.empty((T,), dtype=torch.int32, device=dev)
    image = torch.empty((T, oh, ow, 3), dtype=torch.uint8, device=dev) if want_image else None
    mask = torch.empty((T, oh, ow), dtype=torch.uint8, device=dev) if want_image else None
    N.check(N.lib().acez_reproject_score(_ptr(pts), _ptr(clr), pts.shape[0], _ptr(vw), T, oh, ow, _ptr(tg), float(depth_band),
                                         _ptr(scratch), need.value, _ptr(sse), _ptr(covered), _ptr(image), _ptr(mask), _stream()))
    return {"sse": sse, "covered": covered, "image": image, "mask": mask}


def psnr_of(sse, covered):
    """Per view 10 log10(255^2 * 3 * covered / sse) in float64: inf for sse 0, None for a view without a covered cell."""
    out = []
    for s, c in zip(np.asarray(sse).tolist(), np.asarray(covered).tolist()):
        out.append(None if c == 0 else math.inf if s == 0 else float(10.0 * np.log10(np.float64(255.0 ** 2 * 3.0 * c) / np.float64(s))))
    return out


def summarise(sse, covered, cells_per_view):
    """The per-view lists and their means over the views that have coverage."""
    psnr = psnr_of(sse, covered)
    coverage = [float(c) / cells_per_view for c in np.asarray(covered).tolist()]
    seen = [i for i, p in enumerate(psnr) if p is not None]
    return {"psnr": psnr, "coverage": coverage, "sse": [int(s) for s in np.asarray(sse).tolist()],
            "covered_cells": [int(c) for c in np.asarray(covered).tolist()],
            "mean_psnr": float(np.mean([psnr[i] for i in seen])) if seen else None,
            "mean_coverage": float(np.mean([coverage[i] for i in seen])) if seen else None,
            "n_uncovered_views": len(psnr) - len(seen)}


def reproject_inputs(transforms_json, network, encoder_path, image_resolution=480, compute_dtype=None, chunk=64):
    """What `reproject` hands to score_views for a written transforms.json: (points [M,3] f32, colours [M,3] u8, views [T,15] f32
    numpy, targets [T,oh,ow,3] u8, info) with the train frames' point cloud of `network` (head checkpoint) as sources and the test
    frames' cell means as targets, poses and focals as the file states them."""
    import torch
    from .images import _default_encoder_path, load_frames
    from .session import ReconstructionSession, default_options
    with open(transforms_json) as f:
        tr = json.load(f)
    by_file = {fr["file_path"]: fr for fr in tr["frames"]}
    train, test = [by_file[n] for n in tr["train_filenames"]], [by_file[n] for n in tr["test_filenames"]]
    if not test:
        raise SystemExit("the split has no test frame")
    # focal lengths refer to the frames' stated size (w x h); the network sees them resized to a short side of image_resolution
    scale = image_resolution / min(train[0]["w"], train[0]["h"])
    focals = np.array([fr["fl_x"] * scale for fr in train], np.float64)
    if not np.allclose(focals, focals[0]):
        raise SystemExit("reproject supports a single focal length over the train frames (as export_point_cloud.py does)")
    _, frames, _, rgb = load_frames(None, image_resolution, files=[fr["file_path"] for fr in train], return_rgb=True)
    so = default_options(use_external_focal_length=float(focals[0]), use_aug=False, registration_confidence=0, compute_dtype=compute_dtype)
    ses = ReconstructionSession(torch.load(_default_encoder_path(encoder_path), map_location="cpu"), frames, opt=so, chunk=chunk)
    c2w = np.stack([np.linalg.inv(pose_from_transform_matrix(fr["transform_matrix"])) for fr in train])
    xyz, src, _ = ses.point_cloud(torch.load(network, map_location="cpu"), c2w, np.full(len(train), np.inf), ses.focal0, dense=False,
                                  filter_depth=100, opengl=False)
    dev = ses.dev
    means = torch.cat([cell_means(torch.from_numpy(rgb[i:i + chunk]).to(dev)) for i in range(0, len(rgb), chunk)])
    assert tuple(means.shape[1:3]) == (ses.oh, ses.ow)
    colours = means.reshape(-1, 3)[torch.from_numpy(np.asarray(src, np.int64)).to(dev)]   # src = position * oh * ow + cell
    points = torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(dev)
    H, W = int(frames.shape[2]), int(frames.shape[3])
    del ses
    _, tframes, _, trgb = load_frames(None, image_resolution, files=[fr["file_path"] for fr in test], return_rgb=True)
    if tuple(tframes.shape[2:]) != (H, W):
        raise SystemExit("the test frames resize to another shape than the train frames")
    targets = torch.cat([cell_means(torch.from_numpy(trgb[i:i + chunk]).to(dev)) for i in range(0, len(trgb), chunk)])
    views = make_views(np.stack([pose_from_transform_matrix(fr["transform_matrix"]) for fr in test]),
                       np.array([fr["fl_x"] * scale for fr in test]), W / 2.0, H / 2.0)
    info = {"n_test": len(test), "n_train_used": len(train), "n_points": int(points.shape[0]), "test_filenames": tr["test_filenames"],
            "cells": [int(targets.shape[1]), int(targets.shape[2])]}
    return points, colours, views, targets, info


def run(pose_file, images_glob_pattern, output_dir, split_json=None, no_run_nerfstudio=False, method="reproject", camera_optimizer="off",
        max_resolution=640, network=None, encoder_path="<path>", image_resolution=480, depth_band=0.05, compute_dtype=None):
    """The file-level path of benchmark_poses.py: the data set always; with method "reproject" (and without --no_run_nerfstudio) the
    score, written to <output_dir>/results_reproject.json. Returns that path, or None for a dry run."""
    check_method(method, no_run_nerfstudio, camera_optimizer)
    transforms_json, _ = write_dataset(pose_file, images_glob_pattern, output_dir, split_json, max_resolution)
    if no_run_nerfstudio:
        return None
    if network is None:
        raise SystemExit("--method reproject needs --network: the head (.pt) whose scene coordinates give the train frames' geometry")
    points, colours, views, targets, info = reproject_inputs(transforms_json, network, encoder_path, image_resolution, compute_dtype)
    out = score_views(points, colours, views, targets, depth_band, want_image=False)
    res = summarise(out["sse"].cpu().numpy(), out["covered"].cpu().numpy(), info["cells"][0] * info["cells"][1])
    res.update(info)
    res.update({"metric": METRIC, "depth_band": float(depth_band), "image_resolution": int(image_resolution)})
    path = Path(output_dir) / "results_reproject.json"
    with open(path, "w") as f:
        json.dump(res, f, indent=4)
    _logger.info(f"Reprojection PSNR (1/8 resolution, {res['n_test']} test views, {res['n_train_used']} train frames, {res['n_points']} "
                 f"points): mean {res['mean_psnr'] if res['mean_psnr'] is None else round(res['mean_psnr'], 2)} dB, mean coverage "
                 f"{res['mean_coverage'] if res['mean_coverage'] is None else round(res['mean_coverage'], 3)}, "
                 f"{res['n_uncovered_views']} views without coverage -> {path}")
    return path


def check_method(method, no_run_nerfstudio, camera_optimizer):
    """The refusals that need nothing but the arguments."""
    if method in ("nerfacto", "splatfacto") and not no_run_nerfstudio:
        raise SystemExit(f"--method {method} fits a model in nerfstudio, which is not part of this package: it is refused rather than "
                         "replaced by another metric. Pass --no_run_nerfstudio to write the data set for a nerfstudio elsewhere, or use "
                         "--method reproject.")
    if method not in ("reproject", "nerfacto", "splatfacto"):
        raise SystemExit(f"unknown --method {method!r}")
    if method == "reproject" and camera_optimizer != "off":
        raise SystemExit("--camera_optimizer other than off is refused with --method reproject: the score is of the poses as given, and "
                         "nothing here optimises cameras.")
