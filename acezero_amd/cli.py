"""Command-line surfaces of the hot path: same flag names and defaults as the reference's train_ace.py (:21-228)
and register_mapping.py (:47-114), driving the MI355X kernels through libacez.so.

What these entry points do NOT contain is the reference's image pipeline (dataset.py image decoding/augmentation
and the pre-trained encoder): the encoder features are taken from a file

    train_ace.py        --feature_buffer  buffer.npz     (layout of acez_train_buffer, see save_feature_buffer)
    register_mapping.py --feature_file    frames.npz     (per-frame encoder features or scene coordinates)

written by whatever fills the buffer (the reference's create_training_buffer with the 6-line hook of
INTEGRATION.md, or acezero_amd.synth for synthetic scenes). Everything after that point -- the training loop, the
schedule and early stopping, head checkpoints, pose files -- follows the reference's formats.
"""
import argparse
import logging
import math
import os
import time
from pathlib import Path

import numpy as np

from . import DEFAULT_DTYPE
from .formats import (_strtobool, focal_at_height, read_ace_pose_file, read_crop_file, read_depth_png, read_ply_mesh,
                      read_ply_points, read_ply_vertices, read_posed_images, write_depth_png, write_ply, write_pose_line,
                      write_poses_like)
# the host loaders live in images.py; their names stay in this namespace (cli.load_frames, ...) for callers and tests
from .images import (_default_encoder_path, check_calibration_focals, check_single_focal, depth_map_at_cells, focals_in_original_units,
                     frame_shapes, frame_size_classes, initial_focals, load_depth_maps, load_frames, load_session_frames, session_frames)

_logger = logging.getLogger("acezero_amd")


def _require_gpu(name, why):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{name}.py needs a GPU: {why}, there is no CPU path")


def _require_ply(path):
    if not str(path).endswith(".ply"):
        raise SystemExit("output file format not supported: use .ply")


# (flags, type, default, choices, help) -- train_ace.py:21-228
TRAIN_FLAGS = [
    (("--base_seed",), int, 2089, None, "seed of the derived random generators"),
    (("--pose_files",), str, None, None, "glob of per-image pose files"),
    (("--use_ace_pose_file",), Path, None, None, "ACE pose file (file qw qx qy qz tx ty tz f conf)"),
    (("--ace_pose_file_conf_threshold",), float, 1000, None, "ignore pose-file entries below this confidence"),
    (("--use_pose_seed",), float, -1, None, "map a single image with identity pose"),
    (("--depth_files",), str, None, None, "glob of depth files"),
    (("--refine_calibration",), _strtobool, False, None, "optimise the focal length during mapping"),
    (("--refine_calibration_lr",), float, 0.001, None, "learning rate of the focal-length refinement"),
    (("--use_heuristic_focal_length",), _strtobool, False, None, "use 70%% of the image diagonal as focal length"),
    (("--use_external_focal_length",), float, None, None, "externally provided focal length"),
    (("--image_resolution",), int, 480, None, "short side of the training images"),
    (("--num_data_workers",), int, 12, None, "data loader workers"),
    (("--encoder_path",), Path, "<path>", None, "pre-trained encoder weights"),
    (("--load_weights",), Path, None, None, "head weights to start from"),
    (("--num_head_blocks",), int, 1, None, "residual blocks of the head"),
    (("--use_half",), _strtobool, True, None, "16-bit matrix arithmetic (True: bf16, or fp16 with --compute_dtype fp16; False = fp32 is NOT "
                                                "implemented and is rejected, never replaced by another precision)"),
    (("--use_homogeneous",), _strtobool, True, None, "homogeneous scene-coordinate output"),
    (("--learning_rate_min",), float, 0.0005, None, ""),
    (("--learning_rate_max",), float, 0.005, None, ""),
    (("--learning_rate_schedule",), str, "circle", ["circle", "constant", "1cyclepoly"], ""),
    (("--learning_rate_warmup_iterations",), int, 1000, None, ""),
    (("--learning_rate_warmup_learning_rate",), float, 0.0005, None, ""),
    (("--learning_rate_cooldown_iterations",), int, 5000, None, ""),
    (("--learning_rate_cooldown_trigger_px_threshold",), int, 10, None, ""),
    (("--learning_rate_cooldown_trigger_percent_threshold",), float, 0.7, None, ""),
    (("--max_training_buffer_size",), int, 8000000, None, ""),
    (("--max_dataset_passes",), int, 10, None, ""),
    (("--samples_per_image",), int, 1024, None, ""),
    (("--training_buffer_cpu",), _strtobool, False, None, "accepted for compatibility; the buffer lives in HBM"),
    (("--batch_size",), int, 5120, None, ""),
    (("--iterations",), int, 25000, None, ""),
    (("--iterations_output",), int, 300, None, ""),
    (("--repro_loss_hard_clamp",), int, 1000, None, ""),
    (("--repro_loss_soft_clamp",), int, 50, None, ""),
    (("--repro_loss_soft_clamp_min",), int, 1, None, ""),
    (("--repro_loss_type",), str, "dyntanh", ["l1", "l1+sqrt", "l1+log", "tanh", "dyntanh"], ""),
    (("--repro_loss_schedule",), str, "circle", ["circle", "linear"], ""),
    (("--depth_min",), float, 0.1, None, ""),
    (("--depth_target",), float, 10, None, ""),
    (("--depth_max",), float, 1000, None, ""),
    (("--use_aug",), _strtobool, True, None, ""),
    (("--aug_rotation",), int, 15, None, ""),
    (("--aug_scale",), float, 1.5, None, ""),
    (("--render_visualization",), _strtobool, False, None, "render the mapping frames and write <map stem>_mapping.pkl"),
    (("--render_target_path",), Path, "renderings", None, ""),
    (("--use_existing_vis_buffer",), Path, None, None, ""),
    (("--render_flipped_portrait",), _strtobool, False, None, ""),
    (("--render_map_error_threshold",), int, 10, None, ""),
    (("--render_map_depth_filter",), int, 100, None, ""),
    (("--render_camera_z_offset",), int, 4, None, ""),
    (("--render_marker_size",), float, 0.03, None, ""),
    (("--pose_refinement",), str, "none", ["none", "naive", "mlp"], ""),
    (("--pose_refinement_weight",), float, 0.1, None, ""),
    (("--pose_refinement_wait",), int, 0, None, ""),
    (("--pose_refinement_lr",), float, 0.001, None, ""),
    (("--refinement_ortho",), str, "gram-schmidt", ["gram-schmidt", "procrustes"], ""),
]

# register_mapping.py:47-114
REGISTER_FLAGS = [
    (("--encoder_path",), Path, "<path>", None, "pre-trained encoder weights"),
    (("--session", "-sid"), None, "", None, "session name appended to the output file"),
    (("--image_resolution",), int, 480, None, ""),
    (("--num_data_workers",), int, 12, None, ""),
    (("--hypotheses", "-hyps"), int, 64, None, "RANSAC hypotheses"),
    (("--hypotheses_max_tries",), int, 1000000, None, "re-tries of an invalid minimal set"),
    (("--threshold", "-t"), float, 10, None, "inlier threshold in px"),
    (("--inlieralpha", "-ia"), float, 100, None, "soft inlier count alpha"),
    (("--maxpixelerror", "-maxerrr"), float, 100, None, "reprojection errors are clamped to this value"),
    (("--render_visualization",), _strtobool, False, None, "render one frame per query and write <network stem>_register.pkl"),
    (("--render_target_path",), Path, "renderings", None, ""),
    (("--render_flipped_portrait",), _strtobool, False, None, ""),
    (("--render_pose_conf_threshold",), int, 5000, None, ""),
    (("--render_map_depth_filter",), int, 10, None, ""),
    (("--render_camera_z_offset",), int, 4, None, ""),
    (("--base_seed",), int, 1305, None, "torch and RANSAC seed"),
    (("--confidence_threshold",), float, 1000, None, ""),
    (("--max_estimates",), int, -1, None, "stop after this many images"),
    (("--use_external_focal_length",), float, -1, None, ""),
    (("--render_marker_size",), float, 0.03, None, ""),
]


# ace_zero.py:41-177
ACE_ZERO_FLAGS = [
    (("--depth_files",), str, None, None, "depth maps (16 bit, millimetres), one per image: read for the seed images, with --rgbd True for every image in every round; without them the reference downloads ZoeDepth"),
    (("--iterations_max",), int, 100, None, "maximum number of mapping / relocalisation rounds"),
    (("--registration_threshold",), float, 0.99, None, "stop when this ratio of images is registered"),
    (("--relative_registration_threshold",), float, 0.01, None, "stop when fewer new images than this were registered"),
    (("--final_refine",), _strtobool, True, None, "one more mapping round after the stopping criteria are met"),
    (("--final_refit",), _strtobool, True, None, "refit a fresh network in the last round"),
    (("--final_refit_posewait",), int, 5000, None, ""),
    (("--refit_iterations",), int, 25000, None, ""),
    (("--registration_confidence",), int, 500, None, "inlier count above which an image counts as registered"),
    (("--try_seeds",), int, 5, None, "number of seed images to try"),
    (("--seed_parallel_workers",), int, 3, None, "accepted; the seed trials are mapped one after the other: trained side by side "
                                                 "(ReconstructionSession.reconstruct(seed_parallel_workers=...), one head group) they give the "
                                                 "same result and measured no faster on one MI355X"),
    (("--seed_iterations",), int, 10000, None, ""),
    (("--seed_network",), Path, None, None, "pre-trained head to start from"),
    (("--warmstart",), _strtobool, True, None, ""),
    (("--export_point_cloud",), _strtobool, False, None, ""),
    (("--dense_point_cloud",), _strtobool, False, None, ""),
    (("--refinement",), str, "mlp", ["mlp", "none", "naive"], ""),
    (("--refinement_ortho",), str, "gram-schmidt", ["gram-schmidt", "procrustes"], ""),
    (("--pose_refinement_wait",), int, 0, None, ""),
    (("--pose_refinement_lr",), float, 0.001, None, ""),
    (("--refine_calibration",), _strtobool, True, None, ""),
    (("--use_external_focal_length",), float, -1, None, "-1: 70%% of the image diagonal"),
    (("--learning_rate_schedule",), str, "1cyclepoly", ["circle", "constant", "1cyclepoly"], ""),
    (("--learning_rate_max",), float, 0.003, None, ""),
    (("--cooldown_iterations",), int, 5000, None, ""),
    (("--cooldown_threshold",), float, 0.7, None, ""),
    (("--image_resolution",), int, 480, None, ""),
    (("--num_head_blocks",), int, 1, None, ""),
    (("--max_dataset_passes",), int, 10, None, ""),
    (("--repro_loss_type",), str, "tanh", ["l1", "l1+sqrt", "l1+log", "tanh", "dyntanh"], ""),
    (("--repro_loss_hard_clamp",), int, 1000, None, ""),
    (("--repro_loss_soft_clamp",), int, 50, None, ""),
    (("--aug_rotation",), int, 15, None, ""),
    (("--num_data_workers",), int, 12, None, "accepted; frames are decoded once by the main process (with --gpu_ingest True: decode threads)"),
    (("--training_buffer_cpu",), _strtobool, False, None, "accepted; the buffer lives in HBM"),
    (("--ransac_iterations",), int, 32, None, ""),
    (("--ransac_threshold",), float, 10, None, ""),
    (("--render_visualization",), _strtobool, False, None, "render every round, the final sweep and (ffmpeg on PATH) "
                                                         "results/reconstruction.mp4 into results/renderings"),
    (("--render_flipped_portrait",), _strtobool, False, None, ""),
    (("--render_marker_size",), float, 0.03, None, ""),
    (("--iterations_output",), int, 500, None, ""),
    (("--random_seed",), int, 1305, None, ""),
]


def _add(parser, table):
    for flags, typ, default, choices, hlp in table:
        kw = {"default": default, "help": hlp}
        if typ is not None:
            kw["type"] = typ
        if choices is not None:
            kw["choices"] = choices
        parser.add_argument(*flags, **kw)


def _add_dtype(p):
    p.add_argument("--compute_dtype", default=None, choices=["bf16", "fp16"],
                   help="[additive] 16-bit operand format of encoder and head (fp32 accumulation in both): fp16 is the reference's autocast "
                        "arithmetic (ace_trainer.py:366-367,517-518, register_mapping.py:209-210), bf16 what BASELINE.json's north_star "
                        "names; default: $ACEZ_DTYPE, else " + DEFAULT_DTYPE)


def train_parser():
    p = argparse.ArgumentParser(description="Fast training of a scene coordinate regression network (MI355X head trainer).",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("rgb_files", type=str, help="glob of the RGB files (recorded in the outputs; pixels are not read here)")
    p.add_argument("output_map_file", type=Path, help="target file for the trained head")
    _add(p, TRAIN_FLAGS)
    p.add_argument("--feature_buffer", type=Path, default=None, help="[additive] .npz training buffer (acez_train_buffer layout)")
    _add_dtype(p)
    p.add_argument("--num_gpus", type=int, default=1, help="[additive] informational; multi-GPU reconstructions are launched as "
                   "`torchrun --nproc-per-node G ace_zero.py ...` (the mapping rounds inside are data parallel)")
    return p


def register_parser():
    p = argparse.ArgumentParser(description="Estimate camera poses for a set of images (MI355X DSAC*).",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("rgb_files", type=str, help="glob of the RGB files")
    p.add_argument("network", type=Path, help="head weights of the scene")
    _add(p, REGISTER_FLAGS)
    p.add_argument("--feature_file", type=Path, default=None, help="[additive] .npz with per-frame encoder features or scene coordinates")
    _add_dtype(p)
    return p


def register_rgbd_parser():
    """register_mapping_rgbd.py: register_mapping.py's flags plus the depth maps; --threshold / --maxpixelerror are read in centimetres
    (DSAC*'s RGB-D convention, dsacstar.cpp:498-500)."""
    p = register_parser()
    p.description = ("Estimate camera poses for a set of RGB-D images (MI355X DSAC* RGB-D: Kabsch on scene <-> camera coordinates). "
                     "--threshold and --maxpixelerror are in CENTIMETRES here.")
    p.add_argument("--depth_files", type=str, required=True, help="glob of the depth maps (16 bit, millimetres), one per image, in the "
                   "sorted order of the images (the format ace_zero.py --depth_files reads)")
    return p


def ace_zero_parser():
    p = argparse.ArgumentParser(description="Run ACE0 for a scene in ONE process on one MI355X (acezero_amd.session).",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("rgb_files", type=str, help="glob of the RGB files, e.g. 'datasets/scene/*.jpg'")
    p.add_argument("results_folder", type=Path, help="output folder")
    _add(p, ACE_ZERO_FLAGS)
    p.add_argument("--encoder_path", type=Path, default=Path(__file__).resolve().parent.parent / "ace_encoder_pretrained.pt",
                   help="[additive] pre-trained encoder weights (train_ace.py / register_mapping.py take the same flag)")
    _add_dtype(p)
    return p


def ace_zero_cli_parser():
    """What ace_zero.py parses: ace_zero_parser() -- the reference's flag surface, which tests/test_cli.py pins -- plus the flags of the
    modes the reference does not have."""
    p = ace_zero_parser()
    p.add_argument("--rgbd", type=_strtobool, default=False,
                   help="[additive] RGB-D reconstruction: --depth_files must match one depth map per image (not only the seeds'); every "
                        "mapping round is depth-supervised and every registration DSAC*'s RGB-D estimator, so the result is in the "
                        "sensor's metres. --ransac_threshold is then read in CENTIMETRES of 3D distance (10 = 10 cm), as "
                        "register_mapping_rgbd.py reads --threshold, and the distance errors are clamped at 100 cm; "
                        "--registration_confidence stays an inlier count over cells. One GPU.")
    return p


def with_ingest_flag(p):
    """What the image-reading scripts parse on top of their parser: the surfaces that tests/test_cli.py pins stay as they are."""
    p.add_argument("--gpu_ingest", type=_strtobool, default=False,
                   help="[additive] read the images through acezero_amd.ingest: --num_data_workers threads (at most 16) decode the files, "
                        "resize, grey conversion and normalisation run as HIP kernels on the decoded frames. The frames, and so every "
                        "result, are bit for bit those of the default host path.")
    return p


def _frame_loaders(opt):
    """(load_frames, load_session_frames) of a run: the host functions below or, with --gpu_ingest True, their device counterparts
    with --num_data_workers decode threads."""
    if not getattr(opt, "gpu_ingest", False):
        return load_frames, load_session_frames
    import functools
    from . import ingest
    workers = getattr(opt, "num_data_workers", 12)
    return (functools.partial(ingest.load_frames_device, workers=workers),
            functools.partial(ingest.load_session_frames_device, workers=workers))


def export_point_cloud_parser():
    """export_point_cloud.py:26-58."""
    p = argparse.ArgumentParser(description="Extract point cloud from network or visualization buffer file; .txt and .ply are supported.",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("output_file", type=Path)
    p.add_argument("--network", type=Path, help="network to extract point cloud from.")
    p.add_argument("--pose_file", type=Path, help="pose file of images that trained the network")
    p.add_argument("--visualization_buffer", type=Path, help="vis buffer file that contains a pre-calculated point cloud.")
    p.add_argument("--encoder_path", type=Path, default="<path>", help="file containing pre-trained encoder weights")
    p.add_argument("--image_resolution", type=int, default=480, help="base image resolution")
    p.add_argument("--confidence_threshold", type=int, default=500)
    p.add_argument("--convention", type=str, default="opengl", choices=["opengl", "opencv"], help="coordinate convention of the point cloud")
    p.add_argument("--dense_point_cloud", type=_strtobool, default=False, help="do not filter points based on reprojection error")
    _add_dtype(p)
    return p


# ------------------------------------------------------------------------------------------------------- feature buffer
def save_feature_buffer(path, prob, image_files=None, with_depth_targets=False):
    """Write a training buffer (dict in the layout of acezero_amd.synth.make_training_problem) as .npz."""
    n_img = prob["image_pose_inv"].shape[0]
    files = image_files if image_files is not None else [f"frame_{i:06d}.png" for i in range(n_img)]
    np.savez(path, features=prob["features"].astype(np.float16), target_px=prob["target_px"], view_idx=prob["view_idx"],
             view_aug_inv=prob["view_aug_inv"], view_K=prob["view_K"], view_Kinv=prob["view_Kinv"], view_image=prob["view_image"],
             image_pose_inv=prob["image_pose_inv"], mean=prob["mean"], focal=np.float32(prob["focal"]), image_files=np.array(files),
             **({"target_crds": prob["target_crds"]} if with_depth_targets else {}))


# ------------------------------------------------------------------------------------------------------------ train
def train_main(argv=None):
    opt = with_ingest_flag(train_parser()).parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    return train_with_options(opt)


def train_with_options(opt):
    """The body of train_ace.py after argument parsing: what the reference runs as TrainerACE(options).train() (train_ace.py:240-241;
    the top-level ace_trainer.TrainerACE shim calls this)."""
    import torch
    from .head import HeadTrainer
    if opt.batch_size % 512 != 0:
        raise SystemExit("batch_size must be a multiple of 512 (train_ace.py:138)")
    if not opt.use_half:
        raise SystemExit("--use_half False (fp32 head arithmetic, ace_trainer.py:330) is not implemented on this path; it is refused rather "
                         "than silently run in 16 bits. Use --use_half True [--compute_dtype fp16 for the reference's autocast precision].")
    dtype = getattr(opt, "compute_dtype", None)
    if opt.feature_buffer is None:
        return _train_from_images(opt)   # (the session's encoder and head take opt.compute_dtype: _session_options)
    buf = np.load(opt.feature_buffer, allow_pickle=False)
    n = min(int(buf["features"].shape[0]), opt.max_training_buffer_size)
    focal = float(opt.use_external_focal_length) if opt.use_external_focal_length is not None else float(buf["focal"])
    tr = HeadTrainer(buf["mean"], num_head_blocks=opt.num_head_blocks, use_homogeneous=opt.use_homogeneous, max_batch=opt.batch_size,
                     loss_type=opt.repro_loss_type, soft_clamp=opt.repro_loss_soft_clamp, soft_clamp_min=opt.repro_loss_soft_clamp_min,
                     circle_schedule=opt.repro_loss_schedule == "circle", hard_clamp=opt.repro_loss_hard_clamp, depth_min=opt.depth_min,
                     depth_max=opt.depth_max, depth_target=opt.depth_target,
                     inlier_px_threshold=opt.learning_rate_cooldown_trigger_px_threshold, schedule=opt.learning_rate_schedule,
                     iterations=opt.iterations, lr_min=opt.learning_rate_min, lr_max=opt.learning_rate_max,
                     warmup_iterations=opt.learning_rate_warmup_iterations, warmup_lr=opt.learning_rate_warmup_learning_rate,
                     cooldown_iterations=opt.learning_rate_cooldown_iterations,
                     cooldown_trigger_percent=opt.learning_rate_cooldown_trigger_percent_threshold,
                     refine_calibration=opt.refine_calibration, focal_init=focal, calib_lr=opt.refine_calibration_lr,
                     pose_refinement=opt.pose_refinement, pose_refinement_wait=opt.pose_refinement_wait,
                     pose_refinement_lr=opt.pose_refinement_lr, pose_refinement_weight=opt.pose_refinement_weight,
                     refinement_ortho=opt.refinement_ortho,
                     pose_seed=opt.base_seed + 511, initial_poses=buf["image_pose_inv"][:, :3] if opt.pose_refinement == "naive" else None,
                     dtype=dtype)
    if opt.load_weights is not None:
        tr.load_state_dict(torch.load(opt.load_weights, map_location="cpu"))
        _logger.info(f"Loaded weights from: {opt.load_weights}")
    else:
        g = torch.Generator().manual_seed(opt.base_seed + 1023)     # ace_trainer.py:66-69 network-initialisation generator
        bound = 1.0 / math.sqrt(512.0)
        tr.load_flat((torch.rand(tr.n_params, generator=g) * 2 - 1) * bound)
    tr.set_buffer(buf["features"][:n].astype(np.float32), buf["target_px"][:n], buf["view_idx"][:n], buf["view_aug_inv"], buf["view_K"],
                  buf["view_Kinv"], buf["view_image"], buf["image_pose_inv"],
                  target_crds=buf["target_crds"][:n] if "target_crds" in buf.files else None)   # present = use_depth (ace_trainer.py:86-92)
    _logger.info(f"Training buffer: {n} patches, {buf['image_pose_inv'].shape[0]} images.")

    log_path = opt.output_map_file.with_suffix(".txt")
    start = time.time()
    epoch, launched, done = 0, 0, False
    orig_poses = np.linalg.inv(buf["image_pose_inv"].astype(np.float64))[:, :3, 3]
    vis = _mapping_visualizer(opt, buf) if opt.render_visualization else None
    with open(log_path, "w", 1) as log:
        from .head import epoch_batches
        pairs = epoch_batches(n, opt.batch_size, opt.base_seed + 8191, tr.device)   # ace_trainer.py:79-80,466 (drawn on the device)
        while not done:
            for _ in range(n // opt.batch_size):
                rows, nxt = next(pairs)
                tr.step(rows, nxt)                                   # (rows, next rows): the next batch is gathered ahead
                launched += 1
                if launched % opt.iterations_output == 0 or launched % 64 == 0:
                    st = tr.state()                                  # the only host synchronisation of the loop
                    if st["nan"]:
                        raise SystemExit("Aborting because of NaN loss")          # ace_trainer.py:615-617
                    if launched % opt.iterations_output == 0:
                        it = st["iteration"] - 1
                        elapsed = time.time() - start
                        _logger.info(f"Iteration: {it:6d}|{st['max_iterations']:6d} / Epoch {epoch:03d}, Loss: {st['loss']:.1f}, "
                                     f"Batch inliers ({opt.learning_rate_cooldown_trigger_px_threshold}px): "
                                     f"{st['batch_inliers'] * 100:.1f}%, Time: {elapsed:.0f}s")
                        cur = np.linalg.inv(np.concatenate([tr.current_poses(), np.tile([[[0, 0, 0, 1.0]]], (len(orig_poses), 1, 1))], 1))[:, :3, 3]
                        d = np.linalg.norm(cur - orig_poses, axis=1)
                        row = f"{it} {elapsed} {st['loss']} {st['batch_inliers']} {d.mean()} {d.min()} {d.max()}"
                        if opt.refine_calibration:
                            row += f" {st['focal_scale'] * focal}"
                        log.write(row + "\n")
                        if vis is not None and launched <= st["max_iterations"]:
                            vis.render_mapping_frame_from_trainer(tr, rows, launched)
                    if st["iteration"] >= st["max_iterations"]:
                        done = True
                        break
            epoch += 1
    st = tr.state()
    elapsed = time.time() - start
    if vis is not None:
        _finalize_mapping_visualization(opt, vis, tr, buf, n)
    _logger.info(f"Done without errors. Training time: {elapsed:.1f}s, {st['iteration']} iterations, "
                 f"{st['iteration'] * opt.batch_size / max(elapsed, 1e-9):.0f} patches/s.")
    # save_model (ace_trainer.py:681-694): half-precision head state_dict
    opt.output_map_file.parent.mkdir(parents=True, exist_ok=True)
    torch.save({k: v.detach().cpu().half() for k, v in tr.state_dict().items()}, opt.output_map_file)
    # save_poses (ace_trainer.py:696-728)
    pose_file = opt.output_map_file.parent / f"poses_{opt.output_map_file.stem}_preliminary.txt"
    files = [str(x) for x in buf["image_files"]] if "image_files" in buf.files else [f"{i}" for i in range(len(orig_poses))]
    f_out = st["focal_scale"] * focal if opt.refine_calibration else focal
    with open(pose_file, "w") as f:
        for i, p34 in enumerate(tr.current_poses()):
            write_pose_line(f, files[i], p34, float("inf"), f_out)
    _logger.info(f"Saved trained head weights to: {opt.output_map_file}; refined poses to: {pose_file}")
    return 0


def _mapping_visualizer(opt, buf):
    """train_ace.py --render_visualization: the mapping phase's visualiser, its pan around the buffer's (original) poses."""
    vis = _train_visualizer(opt)
    vis.setup_mapping(list(np.linalg.inv(buf["image_pose_inv"].astype(np.float64))), existing_state=opt.use_existing_vis_buffer)
    return vis


def _train_visualizer(opt, frame_rgb=None):
    from .render import Visualizer
    return Visualizer(opt.render_target_path, opt.render_flipped_portrait, opt.render_map_depth_filter,
                      mapping_error_threshold=opt.render_map_error_threshold, state_file_name=opt.output_map_file.stem + "_mapping.pkl",
                      marker_size=opt.render_marker_size, camera_z_offset=opt.render_camera_z_offset, every=opt.iterations_output,
                      existing_state=opt.use_existing_vis_buffer, frame_rgb=frame_rgb)


def _register_visualizer(opt, n):
    """register_mapping.py --render_visualization (None without it): continues from `<network stem>_mapping.pkl` in
    --render_target_path, set up for n registration frames."""
    if not opt.render_visualization:
        return None
    from .render import Visualizer
    vis = Visualizer(opt.render_target_path, opt.render_flipped_portrait, opt.render_map_depth_filter,
                     reloc_conf_threshold=opt.render_pose_conf_threshold, confidence_threshold=opt.confidence_threshold,
                     state_file_name=Path(opt.network).stem + "_mapping.pkl", marker_size=opt.render_marker_size,
                     camera_z_offset=opt.render_camera_z_offset)
    vis.setup_reloc(n)
    return vis


def _save_reloc_state(opt, vis):
    if vis is not None:
        vis.save_reloc_state(os.path.join(str(opt.render_target_path), Path(opt.network).stem + "_register.pkl"))


def _session_pose_file(opt):
    return Path(opt.network).parent / f"poses_{opt.session}.txt"


def _register_session(opt, enc_sd, frames, fscale, depth_files=None):
    """The session a registration from images runs in: frames of one size and their resize factor, register_mapping.py's flags as
    session options (the external focal in resized pixels) and, for RGB-D registration, the frames' depth files read at the cells."""
    import torch
    from .session import ReconstructionSession
    depth = None
    if depth_files is not None:
        H, W = frames.shape[2:]
        depth = torch.from_numpy(np.stack([depth_map_at_cells(f, H, W) for f in depth_files]))
    so = _session_options(opt, use_external_focal_length=opt.use_external_focal_length * fscale if opt.use_external_focal_length > 0 else -1.0,
                          ransac_iterations=opt.hypotheses, ransac_threshold=opt.threshold, register_seed=opt.base_seed, use_aug=False,
                          registration_confidence=opt.confidence_threshold)
    return ReconstructionSession(enc_sd, frames, opt=so, depth=depth)


def _finalize_mapping_visualization(opt, vis, tr, buf, n, max_points=1_000_000):
    """The transition frames and `<map stem>_mapping.pkl`: the trained head on (at most max_points, evenly strided) buffer rows, in
    buffer order, kept where the reprojection error is below the threshold and the depth within --render_map_depth_filter, coloured by
    reprojection error (a feature buffer carries no image colours). OpenGL convention."""
    import torch
    from .render import errors_to_colors, trainer_batch_errors
    rows = np.arange(0, n, -(-n // max_points))                     # ceil stride: at most max_points rows
    feats = buf["features"]                                          # (an NpzFile decodes the array on every access: read it once)
    poses = tr.current_poses()
    xyz, err, depth = [], [], []
    for c0 in range(0, len(rows), 65536):
        r = torch.from_numpy(rows[c0:c0 + 65536]).to(tr.device)
        x = tr.get_scene_coordinates(torch.from_numpy(feats[rows[c0:c0 + 65536]].astype(np.float32)).to(tr.device)).cpu().numpy()
        xyz.append(x)
        err.append(trainer_batch_errors(tr, r, x, poses))
        img = tr._buf["view_image"][tr._buf["view_idx"][r].long()].long().cpu().numpy()
        P = np.asarray(poses, np.float64)[img]
        depth.append(np.einsum("kj,kj->k", P[:, 2, :3], x.astype(np.float64)) + P[:, 2, 3])
    del feats
    xyz = np.concatenate(xyz) if xyz else np.zeros((0, 3), np.float32)
    err = np.concatenate(err) if err else np.zeros(0)
    depth = np.concatenate(depth) if depth else np.zeros(0)
    keep = (err < opt.render_map_error_threshold) & (depth > 0) & (depth < opt.render_map_depth_filter)
    clr, _ = errors_to_colors(err[keep], opt.render_map_error_threshold, vis.mapping_cmap)
    xyz = xyz[keep].copy()
    xyz[:, 1:] *= -1
    vis.finalize_mapping(xyz, clr, poses, vis.poses_w2c_orig)


def _session_options(opt, **extra):
    from .session import default_options
    known = vars(default_options())
    over = {k: v for k, v in vars(opt).items() if k in known and v is not None}
    over.update(extra)
    return default_options(**over)


def _train_from_images(opt):
    """train_ace.py on image files: poses from --use_ace_pose_file / --pose_files / --use_pose_seed, one mapping run of the session."""
    import glob
    import torch
    from .session import ReconstructionSession
    focal_flags = dict(external=opt.use_external_focal_length, heuristic=opt.use_heuristic_focal_length, return_rgb=opt.render_visualization)
    if opt.use_ace_pose_file is not None:
        files, poses, focals = read_ace_pose_file(opt.use_ace_pose_file, opt.ace_pose_file_conf_threshold)
        s = session_frames(_frame_loaders(opt)[1], None, opt.image_resolution, files=files, file_focals=focals, **focal_flags)
    else:
        s = session_frames(_frame_loaders(opt)[1], opt.rgb_files, opt.image_resolution, **focal_flags)
        poses = np.stack([np.loadtxt(f) for f in sorted(glob.glob(opt.pose_files))]) if opt.pose_files is not None else None   # dataset_io.load_pose
    files = s.files
    ids = list(range(len(files)))
    if opt.use_pose_seed >= 0:                                           # dataset.py:110-124
        ids, poses = [int(opt.use_pose_seed * len(files))], np.eye(4)[None]
        if opt.depth_files is None:
            raise SystemExit("--use_pose_seed needs --depth_files here (the reference's ZoeDepth fallback is a network download)")
    elif poses is None or len(poses) != len(files):
        raise SystemExit("need one pose per image: --use_ace_pose_file, --pose_files or --use_pose_seed")
    if s.mixed and opt.refine_calibration:
        check_calibration_focals(s.frame_focals[ids])                    # the frames that are mapped; before any frame is encoded
    depth = load_depth_maps(opt.depth_files, len(files), s.hw) if opt.depth_files is not None else None
    so = _session_options(opt, cooldown_iterations=opt.learning_rate_cooldown_iterations, use_external_focal_length=s.focal,
                          cooldown_threshold=opt.learning_rate_cooldown_trigger_percent_threshold)
    ses = ReconstructionSession(torch.load(_default_encoder_path(opt.encoder_path), map_location="cpu"), s.frames, opt=so, depth=depth,
                                focals=s.frame_focals)
    m = ses.map(ids, torch.from_numpy(np.asarray(poses, np.float64)), ses.focal0 if s.mixed else s.focal, iterations=opt.iterations, loss_type=opt.repro_loss_type,
                schedule=opt.learning_rate_schedule, lr_max=opt.learning_rate_max, refinement=opt.pose_refinement,
                pose_wait=opt.pose_refinement_wait, refine_calibration=opt.refine_calibration,
                load_weights=torch.load(opt.load_weights, map_location="cpu") if opt.load_weights is not None else None,
                with_depth=opt.use_pose_seed >= 0 or opt.depth_files is not None, tag=opt.output_map_file.stem,
                visualizer=_train_visualizer(opt, s.rgb) if opt.render_visualization else None)
    f_out = s.original_focals(m["focal"], ses.frel)                      # each frame's focal back in its own original units
    opt.output_map_file.parent.mkdir(parents=True, exist_ok=True)
    torch.save(m["head"], opt.output_map_file)                           # save_model (ace_trainer.py:681-694)
    pose_file = opt.output_map_file.parent / f"poses_{opt.output_map_file.stem}_preliminary.txt"
    with open(pose_file, "w") as f:                                      # save_poses (ace_trainer.py:696-728)
        for j, i in enumerate(ids):
            write_pose_line(f, files[i], np.vstack([m["poses_w2c"][j], [0, 0, 0, 1.0]]), float("inf"), float(f_out[i]))
    _logger.info(f"Done without errors. {m['iterations']} iterations in {m['seconds']:.1f}s ({m['patches_per_s']:.0f} patches/s). "
                 f"Saved trained head weights to: {opt.output_map_file}; refined poses to: {pose_file}")
    return 0


def _register_mixed_sizes(opt, files, classes, depth_files=None):
    """register_mapping.py on a folder whose frames have several sizes: registration is independent per frame, so every size class
    gets its own encoder / RANSAC context (one ReconstructionSession each); --max_estimates draws its seeded subset over the whole
    list, the random streams are keyed by the position in the whole list, the pose file keeps the list's order. depth_files (one per
    file, same order): RGB-D registration."""
    import torch
    from .session import estimate_subset
    keep = set(int(i) for i in estimate_subset(len(files), opt.max_estimates, opt.base_seed))
    load_frames, _ = _frame_loaders(opt)
    vis = _register_visualizer(opt, len(keep))                              # one video over all size classes, in size-class order
    enc_sd = torch.load(_default_encoder_path(opt.encoder_path), map_location="cpu")
    head_sd = torch.load(opt.network, map_location="cpu")
    rows = {}
    for (w, h), pos in sorted(classes.items()):
        pos = [i for i in pos if i in keep]
        if not pos:
            continue
        sub_files, frames, fscale, *rgb = load_frames(None, opt.image_resolution, files=[files[i] for i in pos],
                                                      return_rgb=opt.render_visualization)
        ses = _register_session(opt, enc_sd, frames, fscale, None if depth_files is None else [depth_files[i] for i in pos])
        poses, inl = ses.register(head_sd, ses.focal0, max_tries=opt.hypotheses_max_tries, rng_ids=pos, tag=f"register {w}x{h}",
                                  visualizer=vis, images=rgb[0] if rgb else None, use_depth=depth_files is not None)
        for k, i in enumerate(pos):
            rows[i] = (poses[k], int(inl[k]), ses.focal0 / fscale)
        del ses
    out = _session_pose_file(opt)
    with open(out, "w") as f:
        for i in sorted(rows):
            p, c, focal = rows[i]
            write_pose_line(f, files[i], np.linalg.inv(np.asarray(p, np.float64)), c, float(focal))
    _logger.info(f"Registered {len(rows)} images of {len(classes)} sizes -> {out}")
    _save_reloc_state(opt, vis)
    return 0


def _register_from_images(opt, depth_files=None):
    """register_mapping.py on image files: encoder -> head -> RANSAC for every frame (register_mapping.py:201-276). depth_files (one
    per image, in the sorted order of the images): RGB-D registration."""
    import torch
    from .session import write_pose_file
    all_files, classes = frame_size_classes(opt.rgb_files)
    if len(classes) > 1:
        return _register_mixed_sizes(opt, all_files, classes, depth_files)
    load_frames, _ = _frame_loaders(opt)
    files, frames, fscale, *rgb = load_frames(opt.rgb_files, opt.image_resolution, return_rgb=opt.render_visualization)
    ses = _register_session(opt, torch.load(_default_encoder_path(opt.encoder_path), map_location="cpu"), frames, fscale, depth_files)
    vis = _register_visualizer(opt, len(files) if opt.max_estimates <= 0 else min(opt.max_estimates, len(files)))
    poses, inl = ses.register(torch.load(opt.network, map_location="cpu"), ses.focal0, max_estimates=opt.max_estimates, max_tries=opt.hypotheses_max_tries,
                              visualizer=vis, images=rgb[0] if rgb else None, use_depth=depth_files is not None)
    out = _session_pose_file(opt)
    write_pose_file(out, [files[i] for i in ses.registered_ids], poses, inl, ses.focal0 / fscale)
    _logger.info(f"Registered {len(poses)} images -> {out}")
    _save_reloc_state(opt, vis)
    return 0


# --------------------------------------------------------------------------------------------------------- register
def register_main(argv=None):
    import torch
    from . import dsacstar
    from .head import HeadTrainer
    from .session import estimate_subset
    opt = with_ingest_flag(register_parser()).parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    if opt.feature_file is None:
        return _register_from_images(opt)
    torch.manual_seed(opt.base_seed)
    data = np.load(opt.feature_file, allow_pickle=False)
    files = [str(x) for x in data["image_files"]]
    ids = estimate_subset(len(files), opt.max_estimates, opt.base_seed)   # a seeded random subset in file order, not the first n frames
    n = len(ids)
    t0 = time.time()
    if "scene_coordinates" in data.files:
        sc = torch.from_numpy(data["scene_coordinates"][ids].astype(np.float32)).cuda()
    else:
        sd = torch.load(opt.network, map_location="cpu")
        nb = sum(1 for k in sd if k.endswith("c0.weight"))
        head = HeadTrainer(sd["mean"].float().view(3), num_head_blocks=nb, use_homogeneous=sd["fc3.weight"].shape[0] == 4, max_batch=8192,
                           iterations=1, inference_only=True, dtype=opt.compute_dtype)
        head.load_state_dict(sd)                                    # fp16 checkpoint -> fp32 masters -> 16-bit compute copies
        h, w = int(data["h"]), int(data["w"])
        feats = torch.from_numpy(data["features"][ids].astype(np.float32)).cuda().reshape(-1, 512)
        sc = head.get_scene_coordinates(feats).reshape(n, h, w, 3).permute(0, 3, 1, 2).contiguous()
    f_ext = opt.use_external_focal_length
    focal = np.broadcast_to(np.asarray(data["focal"], np.float32), (len(files),)) if f_ext < 0 else np.full(len(files), f_ext, np.float32)
    ppx = np.broadcast_to(np.asarray(data["ppx"], np.float32), (len(files),))
    ppy = np.broadcast_to(np.asarray(data["ppy"], np.float32), (len(files),))
    prm = dict(hyps=opt.hypotheses, thr=opt.threshold, alpha=opt.inlieralpha, max_reproj=opt.maxpixelerror, sub=8, max_tries=opt.hypotheses_max_tries)
    poses, inl, _ = dsacstar.register_batch(sc, [(focal[i], ppx[i], ppy[i]) for i in ids], prm, opt.base_seed, [int(i) for i in ids],
                                            want_masks=False)
    poses, inl = poses.cpu().numpy(), inl.cpu().numpy()
    pose_log_file = _session_pose_file(opt)
    with open(pose_log_file, "w") as f:
        for k, i in enumerate(ids):
            _logger.info(f"Frame: {files[i]}, Confidence: {int(inl[k])}")
            write_pose_line(f, files[i], np.linalg.inv(poses[k].astype(np.float64)), int(inl[k]), float(focal[i]))   # :261-276
    dt = time.time() - t0
    _logger.info(f"Registered {n} images in {dt:.2f}s ({n / max(dt, 1e-9):.0f} images/s) -> {pose_log_file}")
    vis = _register_visualizer(opt, n)
    if vis is not None:
        _logger.info("--feature_file holds no pixels: the registration frames show the frustums without their images")
        for k in range(n):
            vis.render_reloc_frame(poses[k].astype(np.float64), int(inl[k]))
        _save_reloc_state(opt, vis)
    return 0


def register_rgbd_main(argv=None):
    """register_mapping_rgbd.py: register_mapping.py's image path with DSAC*'s RGB-D estimator (dsacstar.forward_rgbd): the depth map
    of every image gives camera coordinates at the feature-map cells, --threshold / --maxpixelerror are centimetres. Writes the same
    poses_<session>.txt."""
    import glob
    opt = with_ingest_flag(register_rgbd_parser()).parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    if opt.feature_file is not None:
        raise SystemExit("register_mapping_rgbd.py reads the images and their depth maps; --feature_file holds neither the frames' pixels "
                         "nor their depth (use register_mapping.py for it)")
    files = sorted(glob.glob(opt.rgb_files))
    if not files:
        raise SystemExit(f"no files match {opt.rgb_files!r}")
    depth_files = sorted(glob.glob(opt.depth_files))
    if len(depth_files) != len(files):
        raise SystemExit(f"--depth_files matches {len(depth_files)} files for {len(files)} images: one depth map per image is needed, "
                         "paired with the images in sorted order")
    return _register_from_images(opt, depth_files)


# --------------------------------------------------------------------------------------------------------- ace_zero
def ace_zero_main(argv=None):
    import torch
    from .session import ReconstructionSession, default_options, write_pose_file
    opt = with_ingest_flag(ace_zero_cli_parser()).parse_args(argv)
    # `torchrun --nproc-per-node G ace_zero.py ...`: one process per GPU (RCCL). Frames, buffer and registration are sharded inside
    # the session; rank 0 writes the files. Without torchrun this is the single-GPU run.
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        if not dist.is_initialized():
            dist.init_process_group(os.environ.get("ACEZ_DIST_BACKEND", "nccl"))
        if opt.export_point_cloud:
            raise SystemExit("--export_point_cloud True runs on one GPU: export from the written pose file with export_point_cloud.py")
        if opt.render_visualization:
            raise SystemExit("--render_visualization True runs on one GPU")
        if opt.rgbd:
            raise SystemExit("--rgbd True runs on one GPU: the depth-supervised buffer fill is not sharded over ranks (run without torchrun)")
    if opt.rgbd and opt.depth_files is None:
        raise SystemExit("--rgbd True needs --depth_files matching one depth map (16 bit, millimetres) per image")
    logging.basicConfig(level=logging.INFO if rank == 0 else logging.WARNING)
    opt.results_folder.mkdir(parents=True, exist_ok=True)
    external = opt.use_external_focal_length if opt.use_external_focal_length > 0 else None
    s = session_frames(_frame_loaders(opt)[1], opt.rgb_files, opt.image_resolution, external=external, return_rgb=True)
    files, rgb = s.files, s.rgb
    if s.mixed:
        if opt.refine_calibration:
            check_calibration_focals(s.frame_focals)                     # before any frame is encoded
        check_single_focal(s.frame_focals / s.factors)
    depth = load_depth_maps(opt.depth_files, len(files), s.hw) if opt.depth_files is not None else None
    if depth is None and opt.seed_network is None:
        raise SystemExit("ace_zero.py (MI355X): seeds need --depth_files (or --seed_network); the reference's ZoeDepth fallback is a "
                         "network download and not part of this package")
    known = vars(default_options())
    over = {k: v for k, v in vars(opt).items() if k in known and k != "seed_network"}
    if external is not None:
        over["use_external_focal_length"] = s.focal
    if opt.seed_network is not None:
        over["seed_network"] = torch.load(opt.seed_network, map_location="cpu")
    ses = ReconstructionSession(torch.load(_default_encoder_path(opt.encoder_path), map_location="cpu"), s.frames, opt=default_options(**over), depth=depth,
                                focals=s.frame_focals)
    # pose files: every frame's focal in its own original units (one focal, the session's nominal one, goes from round to round)
    orig = lambda f: s.original_focals(f, ses.frel)
    render_dir = opt.results_folder / "renderings"                       # ace_zero_util.get_render_path
    render = None
    if opt.render_visualization:
        from .render import Visualizer

        def render(state_name, existing):
            return Visualizer(render_dir, opt.render_flipped_portrait, 100, state_file_name=state_name, marker_size=opt.render_marker_size,
                              every=opt.iterations_output, existing_state=existing, frame_rgb=rgb)
    res = ses.reconstruct(render=render)   # (seed trials one after the other: side by side is not faster here)
    if rank != 0:                                                       # every rank holds the same result; rank 0 writes it
        import torch.distributed as dist
        dist.barrier()
        return 0
    for h in res["history"]:                                            # the files ace_zero.py leaves behind (SURVEY 8b "process/file contract")
        write_pose_file(opt.results_folder / f"poses_{h['id']}.txt", files, h["poses"], h["confidence"], orig(h["focal"]))
        torch.save(h["head"], opt.results_folder / f"{h['id']}.pt")
        _logger.info(f"{h['id']}: registered {h['registration_rate'] * 100:.1f}% of the images")
    write_pose_file(opt.results_folder / "poses_final.txt", files, res["poses"], res["confidence"], orig(res["focal"]))
    if opt.export_point_cloud:
        from .pointcloud import point_colours, write_point_cloud
        xyz, src, sel = res["point_cloud"]
        write_point_cloud(opt.results_folder / "pc_final.ply", xyz, point_colours(ses, rgb, src, sel))
    if opt.render_visualization:
        _render_video(opt, render_dir)
    rates = [float((res["confidence"] > t).mean()) for t in (500, 1000, 2000, 4000)]
    _logger.info(f"Reconstructed in {res['seconds'] / 60:.1f} minutes, {res['iterations']} iterations; "
                 "registration rate @500/@1000/@2000/@4000: " + " ".join(f"{r * 100:.1f}%" for r in rates))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    return 0


def _render_video(opt, render_dir):
    """ace_zero.py:341-370: the final sweep over the last round's state, then ffmpeg if it is on PATH (else the command is logged and
    the PNG frames stay)."""
    import shlex
    import shutil
    import subprocess
    from .render import render_final_sweep_main
    _logger.info("Rendering final sweep.")
    if render_final_sweep_main([str(render_dir), "--render_marker_size", str(opt.render_marker_size)]) != 0:
        raise SystemExit("the final sweep found no registration state to render from")
    cmd = ["ffmpeg", "-y", "-framerate", "30", "-pattern_type", "glob", "-i", f"{render_dir}/*.png", "-c:v", "libx264", "-pix_fmt",
           "yuv420p", str(opt.results_folder / "reconstruction.mp4")]
    ffmpeg = shutil.which("ffmpeg")
    if ffmpeg is None:
        _logger.info("ffmpeg is not on PATH; the frames are in %s. To make the video run: %s", render_dir, shlex.join(cmd))
        return
    _logger.info("Converting to video.")
    subprocess.run([ffmpeg] + cmd[1:], check=True)


# ------------------------------------------------------------------------------------------------ export_point_cloud
def export_point_cloud_main(argv=None):
    """export_point_cloud.py: from a visualisation buffer (host only) or from network + pose file (encoder -> head -> filter on
    the device)."""
    import pickle
    import torch
    from .pointcloud import point_colours, write_point_cloud
    parser = with_ingest_flag(export_point_cloud_parser())
    opt = parser.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    if opt.visualization_buffer is None and (opt.network is None or opt.pose_file is None):
        parser.error("You must provide either a visualization buffer or network and pose file.")
    if opt.dense_point_cloud and opt.visualization_buffer is not None:
        parser.error("A dense cloud cannot be extracted from a visualization buffer. Please provide network and pose file.")
    if opt.visualization_buffer is not None:
        with open(opt.visualization_buffer, "rb") as f:
            state = pickle.load(f)
        xyz, clr = np.asarray(state["map_xyz"]).copy(), np.asarray(state["map_clr"])
        if opt.convention == "opencv":                                   # the buffer holds OpenGL coordinates (:104-107)
            xyz[:, 1], xyz[:, 2] = -xyz[:, 1], -xyz[:, 2]
    else:
        from .session import ReconstructionSession, default_options
        files, c2w, focals = read_ace_pose_file(opt.pose_file, opt.confidence_threshold)
        if not files:
            raise SystemExit("no pose above the confidence threshold")
        s = session_frames(_frame_loaders(opt)[1], None, opt.image_resolution, files=files, file_focals=focals, return_rgb=True)
        so = default_options(use_external_focal_length=s.focal, use_aug=False, registration_confidence=opt.confidence_threshold,
                             compute_dtype=opt.compute_dtype)
        ses = ReconstructionSession(torch.load(_default_encoder_path(opt.encoder_path), map_location="cpu"), s.frames, opt=so, focals=s.frame_focals)
        conf = np.full(len(s.files), np.inf)
        xyz, src, sel = ses.point_cloud(torch.load(opt.network, map_location="cpu"), c2w, conf, ses.focal0, dense=opt.dense_point_cloud,
                                        filter_depth=100, opengl=opt.convention == "opengl")
        clr = point_colours(ses, s.rgb, src, sel)
    write_point_cloud(opt.output_file, xyz, clr)
    _logger.info(f"Done. Wrote point cloud to: {opt.output_file}")
    return 0


# ------------------------------------------------------------------------------------------------------------ eval_poses
def eval_parser():
    """eval_poses.py:28-54: the same positional arguments, flags, defaults and help."""
    from .evaluate import DEFAULT_SEED
    p = argparse.ArgumentParser(description='Compute pose error metrics for an ACE pose file using (pseudo) ground truth pose files.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('ace_pose_file', type=Path, help='Path to an ACE pose file with one line per image.')
    p.add_argument('gt_pose_files', type=str,
                   help="Glob pattern for pose files, e.g. 'datasets/scene/*.txt', each file is assumed to "
                        "contain a 4x4 pose matrix, cam2world, correspondence with rgb files in the ACE pose "
                        "file is assumed by alphabetical order")
    p.add_argument('--estimate_alignment', type=_strtobool, default=True,
                   help='Estimate rigid body transformation between estimates and ground truth.')
    p.add_argument('--estimate_alignment_scale', type=_strtobool, default=True,
                   help='Estimate similarity transformation when estimating alignment')
    p.add_argument('--estimate_alignment_conf_threshold', type=float, default=500,
                   help='Only consider pose estimates with higher confidence when estimates the alignment.')
    p.add_argument('--pose_error_thresh_t', type=float, default=0.05, help='Pose threshold (translation) for evaluation and alignment')
    p.add_argument('--pose_error_thresh_r', type=float, default=5, help='Pose threshold (rotation) for evaluation and alignment')
    p.add_argument('--seed', type=int, default=DEFAULT_SEED,
                   help="[additive] key of the device's counter-based stream of RANSAC samples (the reference uses Python's random)")
    return p


def eval_poses_main(argv=None):
    """eval_poses.py: read the ACE pose file (every line) and the GT pose files, align, log per-frame errors, accuracy and medians."""
    import glob
    from .evaluate import evaluate_poses, log_lines, read_pose_pairs
    logging.basicConfig(level=logging.INFO)
    opt = eval_parser().parse_args(argv)
    log = logging.getLogger("eval_poses")
    log.info("Reading ACE pose file.")
    estimates, ground_truth, confidences, n_estimates = read_pose_pairs(opt.ace_pose_file, opt.gt_pose_files)
    log.info(f"Read {n_estimates} poses from: {opt.ace_pose_file}")
    log.info(f"Loaded {len(glob.glob(opt.gt_pose_files))} ground truth poses.")
    if not len(estimates):
        raise SystemExit("no (estimate, ground truth) pairs to evaluate")
    res = evaluate_poses(estimates, ground_truth, confidences,
                         estimate_alignment=opt.estimate_alignment, estimate_alignment_scale=opt.estimate_alignment_scale,
                         estimate_alignment_conf_threshold=opt.estimate_alignment_conf_threshold, pose_error_thresh_t=opt.pose_error_thresh_t,
                         pose_error_thresh_r=opt.pose_error_thresh_r, seed=opt.seed)
    if opt.estimate_alignment and res["T"] is None:
        log.info(f"Alignment requested but failed. Setting all pose errors to {math.inf}.")
    for r_err, t_err in zip(res["r_err"], res["t_err"]):
        log.info(f"Rotation Error: {r_err:.2f}deg, Translation Error: {t_err * 100:.1f}cm")
    total_frames = len(res["t_err"])
    assert total_frames == n_estimates
    log.info("===================================================")
    log.info("Test complete.")
    for line in log_lines(res):
        log.info(line)
    return 0


# ------------------------------------------------------------------------------------------------------ benchmark_poses
# benchmarks/benchmark_poses.py:12-27 ("required" in place of a default for the first three)
BENCHMARK_FLAGS = [
    (("--pose_file",), str, None, None, "Path to the poses file, in ACE0 format. Poses with confidence <1000 will be excluded from the "
                                        "training set."),
    (("--output_dir",), str, None, None, "Output directory where the benchmark results will be written"),
    (("--images_glob_pattern",), str, None, None, "Pattern relative to working directory to glob for images"),
    (("--split_json",), str, None, None, "Path to a JSON file containing splits; if not given, every 8 images will be test images"),
    (("--method",), str, "reproject", ["reproject", "nerfacto", "splatfacto"],
     "reproject [additive, the default here]: reprojection PSNR at 1/8 resolution on the GPU (acezero_amd.benchmark; NOT nerfacto PSNR); "
     "nerfacto / splatfacto: the reference's choices, accepted with --no_run_nerfstudio only (nerfstudio is not part of this package)"),
    (("--camera_optimizer",), str, "off", ["off", "SO3xR3", "SE3"], "Type of camera optimizer for nerfstudio; refused with --method reproject"),
    (("--max_resolution",), int, 640, None, "Maximum resolution of the images of the written data set"),
]


def benchmark_poses_parser():
    p = argparse.ArgumentParser(description="Benchmark some poses by view synthesis: writes the reference's nerfstudio data set and scores "
                                            "the held-out views by reprojection on the GPU (--method reproject).",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    for flags, typ, default, choices, hlp in BENCHMARK_FLAGS:
        kw = {"type": typ, "help": hlp}
        if choices is not None:
            kw["choices"] = choices
        if flags[0] in ("--pose_file", "--output_dir", "--images_glob_pattern"):
            kw["required"] = True
        elif flags[0] == "--split_json":
            kw["required"] = False
        else:
            kw["default"] = default
        p.add_argument(*flags, **kw)
    p.add_argument("--no_run_nerfstudio", action="store_true",
                   help="If given, the script will generate Nerfstudio input files and compute nothing")
    p.add_argument("--network", type=Path, default=None, help="[additive, reproject] head weights (.pt) of the scene, e.g. the last round's")
    p.add_argument("--encoder_path", type=Path, default="<path>", help="[additive, reproject] pre-trained encoder weights")
    p.add_argument("--image_resolution", type=int, default=480, help="[additive, reproject] short side of the frames the network sees")
    p.add_argument("--depth_band", type=float, default=0.05, help="[additive, reproject] points within this relative depth of a cell's "
                                                                  "nearest point colour the cell")
    p.add_argument("--use_half", type=_strtobool, default=True, help="[additive, reproject] 16-bit matrix arithmetic; False (fp32) is not "
                                                                     "implemented and is refused")
    _add_dtype(p)
    return p


def benchmark_poses_main(argv=None):
    """benchmark_poses.py: the reference's data set for nerfstudio, and (--method reproject) the reprojection score of the held-out views."""
    from . import benchmark
    opt = benchmark_poses_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    benchmark.check_method(opt.method, opt.no_run_nerfstudio, opt.camera_optimizer)
    if not opt.use_half:
        raise SystemExit("--use_half False (fp32 network arithmetic) is not implemented on this path; it is refused rather than silently "
                         "run in 16 bits. Use --use_half True [--compute_dtype fp16 for the reference's autocast precision].")
    benchmark.run(Path(opt.pose_file), opt.images_glob_pattern, Path(opt.output_dir), split_json=Path(opt.split_json) if opt.split_json else None,
                  no_run_nerfstudio=opt.no_run_nerfstudio, method=opt.method, camera_optimizer=opt.camera_optimizer,
                  max_resolution=opt.max_resolution, network=opt.network, encoder_path=opt.encoder_path,
                  image_resolution=opt.image_resolution, depth_band=opt.depth_band, compute_dtype=opt.compute_dtype)
    return 0


# ----------------------------------------------------------------------------------------------------------- fuse_depth
MAX_GRID_VOXELS = 2 ** 62                # --sparse True: the virtual grid is limited by its block grid, not by --max_voxels
MAX_SPARSE_GRID_BLOCKS = 2 ** 28         # one flag byte and one int32 table entry per block: 1.3 GB


def fuse_depth_parser():
    p = argparse.ArgumentParser(description="Fuse the depth maps of an RGB-D reconstruction along its estimated poses into a TSDF volume "
                                            "on the GPU and write the surface as a coloured triangle mesh (.ply).",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("pose_file", type=Path, help="ACE pose file of the reconstruction (file qw qx qy qz tx ty tz f conf)")
    p.add_argument("rgb_files", type=str, help="glob of the RGB files, e.g. 'scene/*.jpg'")
    p.add_argument("output_file", type=Path, help="mesh to write (.ply)")
    p.add_argument("--depth_files", type=str, required=True, help="glob of the depth maps (16 bit), one per image, in the sorted order of the "
                                                                  "images (the format ace_zero.py --depth_files reads)")
    p.add_argument("--voxel_size", type=float, default=0.02, help="voxel edge in metres")
    p.add_argument("--truncation", type=float, default=None, help="truncation distance in metres; default: 4 voxels")
    p.add_argument("--max_depth", type=float, default=4.0, help="depth beyond this many metres is not fused")
    p.add_argument("--min_weight", type=float, default=2, help="a voxel belongs to the surface once this many frames have observed it")
    p.add_argument("--confidence_threshold", type=float, default=1000, help="ignore pose-file entries below this confidence")
    p.add_argument("--depth_unit", type=float, default=0.001, help="metres per raw depth unit (0.001: millimetres)")
    p.add_argument("--max_voxels", type=int, default=2 ** 28, help="refuse a volume of more voxels than this")
    p.add_argument("--colour", type=_strtobool, default=True, help="colour the mesh from the RGB files")
    p.add_argument("--sparse", type=_strtobool, default=False, help="store only the 8^3-voxel blocks near a surface: the same mesh (rows in "
                                                                    "another order) for scenes whose dense volume does not fit; "
                                                                    "--max_voxels then limits the allocated voxels")
    _add_component_flags(p)
    p.add_argument("--simplify_cell", type=float, default=None, help="simplify the mesh before it is written: one vertex per grid cell of "
                                                                     "this edge in metres (after the component filter)")
    p.add_argument("--simplify_placement", type=str, default="quadric", choices=["quadric", "mean"],
                   help="with --simplify_cell: a cell's vertex minimises the plane quadrics of the faces around it, or is the mean of its vertices")
    p.add_argument("--refine_poses", type=int, default=0, metavar="ROUNDS",
                   help="refine the poses against the fused volume this many times (fuse, track every frame on the volume's SDF, fuse again) "
                        "before the mesh is extracted; 0: off")
    p.add_argument("--refine_iterations", type=int, default=10, help="with --refine_poses: Gauss-Newton iterations per frame and round at most")
    p.add_argument("--refine_min_weight", type=float, default=1.0, help="with --refine_poses: a depth pixel is used where all eight voxels "
                                                                       "around its point have been observed this many times")
    p.add_argument("--refined_pose_file", type=Path, default=None, help="with --refine_poses: write the refined poses here, in the pose "
                                                                        "file's format (frames whose tracking was degenerate keep their pose)")
    p.add_argument("--model_depth_dir", type=Path, default=None,
                   help="render the mesh that is written into every fused frame's camera (after the component filter and the "
                        "simplification, under the refined poses if --refine_poses ran) and write one 16-bit depth PNG per frame here, "
                        "named after the image, at the depth map's own size and --depth_unit")
    p.add_argument("--model_depth_compare", type=_strtobool, default=False,
                   help="with --model_depth_dir: log how the rendered depth agrees with the input depth, per frame and for the folder")
    p.add_argument("--model_depth_tolerance", type=float, default=0.01, help="with --model_depth_compare: metres up to which two depths agree")
    return p


def _simplify_cell(value, flag):
    """The cell edge of simplify.simplify_mesh from a flag's value."""
    if not (math.isfinite(value) and value > 0.0):
        raise SystemExit(f"{flag} must be positive and finite")
    return value


def _simplify_line(cell, placement, info):
    return (f"Simplified at a cell of {cell} m ({placement}): {info['vertices_in']} vertices, {info['faces_in']} faces ({info['invalid_faces']} invalid, {info['degenerate_faces']} degenerate, "
            f"{info['nonfinite_vertices']} vertices not finite) in {info['clusters']} cells; {info['collapsed_faces']} faces collapsed, "
            f"{info['duplicate_faces']} duplicates and {info['unused_clusters']} cells without a face dropped; {info['vertices_out']} vertices "
            f"({info['fallbacks']} placed at the mean for want of a usable quadric), {info['faces_out']} faces left.")


def _add_component_flags(p):
    """The three criteria of mesh.filter_components; a component must meet all that are given."""
    p.add_argument("--min_component_faces", type=int, default=0, help="drop the connected components of the mesh with fewer faces than this")
    p.add_argument("--min_component_ratio", type=float, default=0.0, help="drop the components with fewer faces than this fraction of the "
                                                                          "largest component's")
    p.add_argument("--keep_largest", type=int, default=None, help="keep only this many components, the ones with the most faces")


def _component_criteria(opt):
    """filter_components' keyword arguments from the flags, or None if every flag has its default (the filter is then not called)."""
    if opt.min_component_faces < 0 or not 0.0 <= opt.min_component_ratio <= 1.0 or (opt.keep_largest is not None and opt.keep_largest < 1):
        raise SystemExit("--min_component_faces must not be negative, --min_component_ratio must be in 0 .. 1, --keep_largest at least 1")
    if opt.min_component_faces == 0 and opt.min_component_ratio == 0.0 and opt.keep_largest is None:
        return None
    return dict(min_faces=opt.min_component_faces, min_ratio=opt.min_component_ratio, keep_largest=opt.keep_largest)


def _component_summary(info):
    h = info["size_histogram"]
    return (f"{info['components']} connected components, the largest of {info['largest_component_faces']} faces ({h[0]} of 1-9 faces, "
            f"{h[1]} of 10-99, {h[2]} of 100-999, {h[3]} of 1000-9999, {h[4]} of 10000 or more); kept "
            f"{info['components_kept']}, dropped {info['faces_dropped']} faces ({info['invalid_faces']} with an index out of range, "
            f"{info['degenerate_faces']} degenerate) and {info['vertices_dropped']} vertices")


def fuse_depth_main(argv=None):
    """fuse_depth.py: depth maps at their own resolution + pose file -> TSDF volume (HIP) -> surface-net mesh (HIP) -> .ply."""
    import glob
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from . import fusion
    parser = fuse_depth_parser()
    opt = parser.parse_args(argv)
    if opt.refined_pose_file is not None and opt.refine_poses == 0:
        parser.error("--refined_pose_file needs --refine_poses ROUNDS")
    if opt.model_depth_compare and opt.model_depth_dir is None:
        parser.error("--model_depth_compare needs --model_depth_dir DIR")
    logging.basicConfig(level=logging.INFO)
    log = logging.getLogger("fuse_depth")
    _require_ply(opt.output_file)
    if opt.voxel_size <= 0:
        raise SystemExit("--voxel_size must be positive")
    if opt.refine_poses < 0 or opt.refine_iterations < 1 or not opt.refine_min_weight > 0:
        raise SystemExit("--refine_poses must not be negative, --refine_iterations at least 1, --refine_min_weight positive")
    criteria = _component_criteria(opt)
    simplify_cell = None if opt.simplify_cell is None else _simplify_cell(opt.simplify_cell, "--simplify_cell")
    truncation = 4.0 * opt.voxel_size if opt.truncation is None else opt.truncation
    rgb_files, depth_files = sorted(glob.glob(opt.rgb_files)), sorted(glob.glob(opt.depth_files))
    if len(depth_files) != len(rgb_files):
        raise SystemExit(f"{len(depth_files)} depth files for {len(rgb_files)} images")
    try:
        c2w_all, focals_all, pose_row = read_posed_images(opt.pose_file, rgb_files, opt.confidence_threshold)
    except ValueError as e:
        raise SystemExit(str(e))
    # (rgb file, depth file, row of the pose file), in the folder's order
    pairs = [(r, d, k) for r, d, k in zip(rgb_files, depth_files, pose_row) if k is not None]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        depth = list(pool.map(read_depth_png, [p[1] for p in pairs]))
        image_h = [Image.open(p[0]).size[1] for p in pairs]
        c2w = np.stack([c2w_all[p[2]] for p in pairs])
        focals = np.array([focal_at_height(focals_all[p[2]], d.shape[0], ih) for p, d, ih in zip(pairs, depth, image_h)])
        origin, dims = fusion.bounds_from_frames(depth, c2w, focals, opt.voxel_size, truncation, depth_unit=opt.depth_unit,
                                                 max_depth=opt.max_depth, max_voxels=MAX_GRID_VOXELS if opt.sparse else opt.max_voxels)
        if opt.sparse:
            grid = fusion.block_grid(dims)
            if grid[0] * grid[1] * grid[2] > MAX_SPARSE_GRID_BLOCKS:
                raise SystemExit(f"the volume would have {grid[0]} x {grid[1]} x {grid[2]} = {grid[0] * grid[1] * grid[2]} blocks of 8^3 voxels, "
                                 f"more than 2^28: raise --voxel_size or lower --max_depth")
        rgb = None
        if opt.colour:
            def read_rgb(job):
                path, (h, w) = job
                return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB").resize((w, h), Image.NEAREST), np.uint8))
            rgb = list(pool.map(read_rgb, [(p[0], d.shape) for p, d in zip(pairs, depth)]))
    t_decode = time.perf_counter() - t0
    _require_gpu("fuse_depth", "TSDF fusion is a HIP kernel")
    t0 = time.perf_counter()
    def make_volume():
        if opt.sparse:
            return fusion.SparseTSDFVolume(origin, dims, opt.voxel_size, truncation, "cuda", max_blocks=opt.max_voxels // fusion.BLOCK_VOXELS)
        return fusion.TSDFVolume(origin, dims, opt.voxel_size, truncation, "cuda")
    rounds = []
    try:                                                     # mark, allocate, integrate: 64 frames a call
        if opt.refine_poses:
            vol, c2w, rounds = fusion.refine_poses(make_volume, depth, c2w, focals, rgb=rgb, rounds=opt.refine_poses, depth_unit=opt.depth_unit,
                                                   max_depth=opt.max_depth, min_weight=opt.refine_min_weight,
                                                   max_iterations=opt.refine_iterations)
        else:
            vol = fusion.fuse(make_volume, depth, c2w, focals, rgb=rgb, depth_unit=opt.depth_unit, max_depth=opt.max_depth)
    except fusion.TooManyBlocks as e:
        raise SystemExit(f"{e}: the volume would allocate more than --max_voxels {opt.max_voxels} voxels: raise --voxel_size, lower "
                         f"--max_depth or raise --max_voxels")
    n_blocks = vol.allocated_blocks if opt.sparse else None
    if opt.refined_pose_file is not None:
        write_poses_like(opt.refined_pose_file, opt.pose_file, opt.confidence_threshold, [p[2] for p in pairs], c2w)
    vertices, colours, faces = vol.extract_mesh(opt.min_weight)
    known = vol.known_voxels(opt.min_weight)
    dropped = None
    if criteria is not None:
        from . import mesh
        vertices, colours, faces, dropped = mesh.filter_components(vertices, colours, faces, **criteria)
    simplified = None
    if simplify_cell is not None:
        from . import simplify
        vertices, colours, faces, simplified = simplify.simplify_mesh(vertices, colours, faces, simplify_cell, opt.simplify_placement)
    model_lines = None
    if opt.model_depth_dir is not None:                      # the mesh as it is written, still on the device
        from . import meshrender
        stems = [os.path.splitext(os.path.basename(p[0]))[0] for p in pairs]
        if len(set(stems)) != len(stems):
            raise SystemExit("two images of the glob share a name: their model depth maps would overwrite each other")
        model_lines = meshrender.render_to_folder(vertices, faces, None, c2w, focals, [d.shape for d in depth], stems, opt.model_depth_dir,
                                                  min_depth=MODEL_MIN_DEPTH, max_depth=opt.max_depth, depth_unit=opt.depth_unit,
                                                  compare=depth if opt.model_depth_compare else None,
                                                  tolerance=opt.model_depth_tolerance)
    vertices, colours, faces = vertices.cpu(), colours.cpu(), faces.cpu()
    t_device = time.perf_counter() - t0
    t0 = time.perf_counter()
    if rgb is None:
        colours[:] = 200
    write_ply(opt.output_file, vertices, colours, faces)
    t_write = time.perf_counter() - t0
    log.info(f"Fused {len(pairs)} of {len(rgb_files)} frames into a volume of {dims[0]} x {dims[1]} x {dims[2]} voxels "
             f"({opt.voxel_size} m, truncation {truncation} m).")
    if opt.sparse:
        grid = fusion.block_grid(dims)
        n_grid, n_vox = grid[0] * grid[1] * grid[2], dims[0] * dims[1] * dims[2]
        log.info(f"Allocated blocks: {n_blocks} of {n_grid} ({100.0 * n_blocks / n_grid:.2f} % of the block grid), "
                 f"{n_blocks * fusion.BLOCK_VOXELS * 20 + n_grid * 5} bytes of volume storage where the dense volume would take {n_vox * 20}.")
    for k, r in enumerate(rounds):
        log.info(f"Pose refinement round {k + 1}: {r['converged']} frames converged, {r['degenerate']} degenerate, {r['out_of_iterations']} out "
                 f"of iterations; mean rms residual {1000.0 * r['rms_before']:.3f} -> {1000.0 * r['rms_after']:.3f} mm, mean pixels used "
                 f"{r['pixels']:.0f}.")
    if opt.refined_pose_file is not None:
        log.info(f"Wrote the refined poses to: {opt.refined_pose_file}")
    log.info(f"Known voxels: {known}. Mesh: {len(vertices)} vertices, {len(faces)} faces.")
    if dropped is not None:
        log.info(f"Extracted mesh: {_component_summary(dropped)}.")
    if simplified is not None:
        log.info(_simplify_line(simplify_cell, opt.simplify_placement, simplified))
    if model_lines is not None:
        for line in model_lines:
            log.info(line)
        log.info(f"Wrote {len(pairs)} model depth maps to: {opt.model_depth_dir}")
    log.info(f"Decode {t_decode:.2f} s, upload + kernels + download {t_device:.2f} s, write {t_write:.2f} s.")
    log.info(f"Done. Wrote mesh to: {opt.output_file}")
    return 0


# ---------------------------------------------------------------------------------------------------------- render_mesh
MODEL_MIN_DEPTH = 0.05                   # the near plane of the model depth maps, metres


def render_mesh_parser():
    p = argparse.ArgumentParser(description="Render a triangle mesh into the cameras of a reconstruction on the GPU: one 16-bit depth PNG "
                                            "per image, seen from that image's pose (and, on request, normal and colour images).",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("mesh_file", type=Path, help="mesh to render (.ply, binary little-endian or ASCII; world coordinates, OpenCV convention)")
    p.add_argument("pose_file", type=Path, help="ACE pose file of the reconstruction (file qw qx qy qz tx ty tz f conf)")
    p.add_argument("rgb_files", type=str, help="glob of the images, e.g. 'scene/*.jpg'")
    p.add_argument("output_dir", type=Path, help="folder for the maps: depth/NAME.png (and normals/, colour/) per image of the glob with a pose")
    p.add_argument("--image_resolution", type=int, default=None, help="short side of the rendered maps; default: the image's own size")
    p.add_argument("--depth_files", type=str, default=None, help="glob of depth maps, one per image in sorted order: every frame is rendered "
                                                                 "at its depth map's size (instead of --image_resolution)")
    p.add_argument("--depth_unit", type=float, default=0.001, help="metres per unit of the written depth maps (0.001: millimetres)")
    p.add_argument("--min_depth", type=float, default=MODEL_MIN_DEPTH, help="near plane in metres: triangles are clipped against it")
    p.add_argument("--max_depth", type=float, default=65.0, help="depth beyond this many metres is not written")
    p.add_argument("--confidence_threshold", type=float, default=1000, help="ignore pose-file entries below this confidence")
    p.add_argument("--write_normals", type=_strtobool, default=False, help="also write normals/NAME.png: 128 + 127 n of the camera-space normal")
    p.add_argument("--write_colour", type=_strtobool, default=False, help="also write colour/NAME.png: the mesh's vertex colours")
    p.add_argument("--compare_depth_files", type=str, default=None, help="glob of measured depth maps (one per image, sorted, of the rendered "
                                                                         "size and --depth_unit): log the agreement per frame and for the folder")
    p.add_argument("--compare_tolerance", type=float, default=0.01, help="with --compare_depth_files: metres up to which two depths agree")
    p.add_argument("--output_json", type=Path, default=None, help="with --compare_depth_files: write the agreement here")
    return p


def render_mesh_main(argv=None):
    """render_mesh.py: .ply + pose file -> rasterisation into every posed image's camera (HIP) -> 16-bit depth PNGs."""
    import glob
    import json
    from PIL import Image
    from . import meshrender
    parser = render_mesh_parser()
    opt = parser.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    log = logging.getLogger("render_mesh")
    if opt.image_resolution is not None and opt.depth_files is not None:
        parser.error("give at most one of --image_resolution and --depth_files")
    if opt.image_resolution is not None and opt.image_resolution < 1:
        raise SystemExit("--image_resolution must be positive")
    for name in ("depth_unit", "min_depth", "max_depth", "compare_tolerance"):
        if not 0 < getattr(opt, name) < math.inf:
            raise SystemExit(f"--{name} must be positive and finite")
    if opt.output_json is not None and opt.compare_depth_files is None:
        parser.error("--output_json needs --compare_depth_files")
    if not opt.mesh_file.is_file():
        raise SystemExit(f"{opt.mesh_file}: no such file")
    rgb_files = sorted(glob.glob(opt.rgb_files))
    if not rgb_files:
        raise SystemExit(f"no files match {opt.rgb_files!r}")
    per_image = {}
    for flag in ("depth_files", "compare_depth_files"):
        if getattr(opt, flag) is not None:
            per_image[flag] = sorted(glob.glob(getattr(opt, flag)))
            if len(per_image[flag]) != len(rgb_files):
                raise SystemExit(f"--{flag}: {len(per_image[flag])} depth files for {len(rgb_files)} images")
    try:
        c2w_all, focals_all, pose_row = read_posed_images(opt.pose_file, rgb_files, opt.confidence_threshold)
    except ValueError as e:
        raise SystemExit(str(e))
    keep = [f for f, k in enumerate(pose_row) if k is not None]
    stems = [os.path.splitext(os.path.basename(rgb_files[f]))[0] for f in keep]
    if len(set(stems)) != len(stems):
        raise SystemExit("two images of the glob share a name: their maps would overwrite each other")
    vertices, colours, faces = read_ply_mesh(opt.mesh_file)
    if opt.write_colour and colours is None:
        raise SystemExit(f"--write_colour: {opt.mesh_file} has no vertex colours")
    from .ingest import resized_size
    sizes, focals = [], []
    for f in keep:
        iw, ih = Image.open(rgb_files[f]).size
        if opt.depth_files is not None:
            w, h = Image.open(per_image["depth_files"][f]).size
        elif opt.image_resolution is not None:
            _, h, w = resized_size(iw, ih, opt.image_resolution)
        else:
            h, w = ih, iw
        sizes.append((h, w))
        focals.append(focal_at_height(focals_all[pose_row[f]], h, ih))
    measured = None
    if opt.compare_depth_files is not None:
        measured = [read_depth_png(per_image["compare_depth_files"][f]) for f in keep]
        for d, size, f in zip(measured, sizes, keep):
            if d.shape != size:
                raise SystemExit(f"{per_image['compare_depth_files'][f]}: {d.shape[1]} x {d.shape[0]} px, but the frame is rendered at "
                                 f"{size[1]} x {size[0]}: give the same files as --depth_files")
    _require_gpu("render_mesh", "the rasterisation is a HIP kernel")
    import torch
    t0 = time.perf_counter()
    device = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    report = {}
    lines = meshrender.render_to_folder(device(vertices), device(np.ascontiguousarray(faces, np.int32)), device(colours),
                                        np.stack([c2w_all[pose_row[f]] for f in keep]), np.array(focals), sizes, stems, opt.output_dir / "depth",
                                        min_depth=opt.min_depth, max_depth=opt.max_depth, depth_unit=opt.depth_unit,
                                        normals_dir=opt.output_dir / "normals" if opt.write_normals else None,
                                        colour_dir=opt.output_dir / "colour" if opt.write_colour else None, compare=measured,
                                        tolerance=opt.compare_tolerance, report=report)
    log.info(f"Rendered {len(faces)} faces into {len(keep)} of {len(rgb_files)} images in {time.perf_counter() - t0:.2f} s "
             f"(upload, kernels, download, write).")
    for line in lines:
        log.info(line)
    if opt.output_json is not None:
        with open(opt.output_json, "w") as fh:
            json.dump(report, fh, indent=1)
        log.info(f"Wrote the agreement to: {opt.output_json}")
    log.info(f"Done. Wrote the maps to: {opt.output_dir}")
    return 0


# ----------------------------------------------------------------------------------------------------------- clean_mesh
def clean_mesh_parser():
    p = argparse.ArgumentParser(description="Drop the floating fragments of a triangle mesh on the GPU: label its connected components "
                                            "and keep those that meet every given criterion. Faces with an index out of range or with "
                                            "two equal indices, and vertices that no kept face uses, are dropped in any case.",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("input_file", type=Path, help="mesh to clean (.ply, binary little-endian or ASCII)")
    p.add_argument("output_file", type=Path, help="mesh to write (.ply)")
    _add_component_flags(p)
    return p


def _mesh_command(name, opt, check, why, run):
    """clean_mesh.py and simplify_mesh.py: .ply -> the device -> one call -> .ply. check(opt) gives what the call takes from the options
    or refuses them; run(log, that, vertices, colours, faces) gives the new mesh on the device and the line that sums it up."""
    logging.basicConfig(level=logging.INFO)
    log = logging.getLogger(name)
    _require_ply(opt.output_file)
    options = check(opt)
    if not opt.input_file.is_file():
        raise SystemExit(f"{opt.input_file}: no such file")
    vertices, colours, faces = read_ply_mesh(opt.input_file)
    _require_gpu(name, why)
    import torch
    device = lambda a: None if a is None else torch.from_numpy(a).cuda()
    out_v, out_c, out_f, summary = run(log, options, device(vertices), device(colours), device(np.ascontiguousarray(faces, np.int32)))
    log.info(summary)
    if len(out_f) == 0:
        log.warning("Nothing is left of the mesh: writing an empty file.")
    out_c = np.full((len(out_v), 3), 200, np.uint8) if out_c is None else out_c.cpu().numpy()
    write_ply(opt.output_file, out_v.cpu().numpy(), out_c, out_f.cpu().numpy())
    log.info(f"Done. Wrote {len(out_v)} vertices, {len(out_f)} faces to: {opt.output_file}")
    return 0


def clean_mesh_main(argv=None):
    """clean_mesh.py: .ply -> connected components (HIP) -> the kept components' faces and vertices in their order (HIP) -> .ply."""
    def run(log, criteria, vertices, colours, faces):
        from . import mesh
        if criteria is None:
            log.info("No criterion given: only faces with an index out of range, degenerate faces and unreferenced vertices are dropped.")
        *out, info = mesh.filter_components(vertices, colours, faces, **(criteria or {}))
        return (*out, f"Read {len(vertices)} vertices, {len(faces)} faces: {_component_summary(info)}.")

    return _mesh_command("clean_mesh", clean_mesh_parser().parse_args(argv), _component_criteria, "the component labelling is a HIP kernel", run)


# -------------------------------------------------------------------------------------------------------- simplify_mesh
def simplify_mesh_parser():
    p = argparse.ArgumentParser(description="Simplify a triangle mesh on the GPU by vertex clustering: the vertices of one grid cell become "
                                            "one vertex, the faces that collapse and the duplicates are dropped. Faces with an index out "
                                            "of range, with two equal indices or with a vertex that is not finite are dropped in any case.",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("input_file", type=Path, help="mesh to simplify (.ply, binary little-endian or ASCII)")
    p.add_argument("output_file", type=Path, help="mesh to write (.ply)")
    p.add_argument("--cell", type=float, required=True, help="edge of the grid cells in metres")
    p.add_argument("--placement", type=str, default="quadric", choices=["quadric", "mean"],
                   help="a cell's vertex minimises the plane quadrics of the faces around it (walls stay flat, corners sharp), or is the "
                        "mean of its vertices")
    return p


def simplify_mesh_main(argv=None):
    """simplify_mesh.py: .ply -> clusters, per-cluster quadrics and their minimisers, surviving faces (HIP) -> .ply."""
    opt = simplify_mesh_parser().parse_args(argv)

    def run(log, cell, vertices, colours, faces):
        from . import simplify
        *out, info = simplify.simplify_mesh(vertices, colours, faces, cell, opt.placement)
        return (*out, _simplify_line(cell, opt.placement, info))

    return _mesh_command("simplify_mesh", opt, lambda o: _simplify_cell(o.cell, "--cell"), "the simplification is HIP kernels", run)


# -------------------------------------------------------------------------------------------------------- eval_geometry
def eval_geometry_parser():
    from .evaluate import DEFAULT_SEED
    p = argparse.ArgumentParser(description="Score a reconstructed point cloud or mesh (by its vertices, or with --sample_spacing by "
                                            "samples of its surface) against a ground-truth cloud on the GPU: precision, recall and "
                                            "F-score per distance threshold (the Tanks and Temples metric).",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("reconstruction", type=Path, help="reconstructed cloud or mesh (.ply, binary little-endian or ASCII)")
    p.add_argument("ground_truth", type=Path, help="ground-truth cloud (.ply)")
    p.add_argument("--thresholds", type=float, nargs="+", default=[0.01, 0.02, 0.05], help="distance thresholds in metres")
    p.add_argument("--voxel_size", type=float, default=None, help="downsample both clouds to one point (the mean) per voxel of this edge first")
    p.add_argument("--max_distance", type=float, default=None, help="search radius, and the value distances are clipped to in the means; "
                                                                    "default: the largest threshold")
    p.add_argument("--crop", type=_strtobool, default=True, help="drop reconstruction points outside the ground truth's bounding box "
                                                                 "enlarged by the search radius")
    p.add_argument("--transform", type=Path, default=None, help="text file with a 4x4 similarity, reconstruction -> ground-truth frame")
    p.add_argument("--ace_pose_file", type=Path, default=None, help="ACE pose file of the reconstruction; with --gt_pose_files the "
                                                                    "similarity is estimated from the two sets of poses as eval_poses.py does")
    p.add_argument("--gt_pose_files", type=str, default=None, help="glob of ground-truth pose files (4x4 cam2world, one per image, matched "
                                                                   "to the pose file's images by alphabetical order)")
    p.add_argument("--estimate_alignment_conf_threshold", type=float, default=500, help="only poses above this confidence enter the alignment")
    p.add_argument("--seed", type=int, default=DEFAULT_SEED, help="key of the alignment's stream of RANSAC samples")
    p.add_argument("--icp", type=_strtobool, default=False, help="refine the alignment (--transform, the pose pair, or the identity) by "
                                                                 "ICP on the GPU before scoring, coarse to fine")
    p.add_argument("--icp_distances", type=float, nargs="+", default=None, help="correspondence radius of every ICP stage in metres; "
                                                                                "default: 4, 2 and 1 times the search radius")
    p.add_argument("--icp_voxel_sizes", type=float, nargs="+", default=None, help="downsample both clouds to this voxel edge in every ICP "
                                                                                  "stage: one value per stage")
    p.add_argument("--icp_max_iterations", type=int, default=30, help="iterations per ICP stage")
    p.add_argument("--icp_scale", type=_strtobool, default=False, help="let ICP estimate a scale factor as well")
    p.add_argument("--sample_spacing", type=float, default=None, help="score the reconstruction, a mesh, by its surface instead of its "
                                                                      "vertices: samples of its faces on the GPU, about this many metres "
                                                                      "(of the ground truth's frame) apart")
    p.add_argument("--gt_sample_spacing", type=float, default=None, help="the same for a ground truth that is a mesh")
    p.add_argument("--sample_seed", type=int, default=0, help="key of the samples' random stream")
    p.add_argument("--write_samples", type=Path, default=None, help="write the reconstruction's samples as they are scored to this .ply")
    p.add_argument("--crop_file", type=Path, default=None, help="Tanks and Temples crop file (.json: a polygon swept along an axis, in the "
                                                                "ground truth's frame): reconstruction points outside it are dropped "
                                                                "before ICP and before scoring")
    p.add_argument("--crop_file_ground_truth", type=_strtobool, default=False, help="apply --crop_file to the ground truth as well")
    p.add_argument("--output_json", type=Path, default=None, help="write the numbers to this file")
    return p


def eval_geometry_main(argv=None):
    """eval_geometry.py: two .ply files (+ an alignment) -> nearest-neighbour distances both ways (HIP) -> precision / recall / F-score."""
    import json
    from . import geometry
    opt = eval_geometry_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    log = logging.getLogger("eval_geometry")
    if opt.transform is not None and (opt.ace_pose_file is not None or opt.gt_pose_files is not None):
        raise SystemExit("give either --transform or the pair --ace_pose_file / --gt_pose_files, not both")
    if (opt.ace_pose_file is None) != (opt.gt_pose_files is None):
        raise SystemExit("--ace_pose_file and --gt_pose_files go together")
    for path in (opt.reconstruction, opt.ground_truth, opt.transform, opt.ace_pose_file):
        if path is not None and not os.path.isfile(path):
            raise SystemExit(f"{path}: no such file")
    if any(not (math.isfinite(t) and t > 0) for t in opt.thresholds):
        raise SystemExit("--thresholds must be positive")
    for name in ("voxel_size", "max_distance"):
        value = getattr(opt, name)
        if value is not None and not (math.isfinite(value) and value > 0):
            raise SystemExit(f"--{name} must be positive")
    icp_distances = None
    if opt.icp:
        radius = max(opt.thresholds) if opt.max_distance is None else opt.max_distance
        icp_distances = [4 * radius, 2 * radius, radius] if opt.icp_distances is None else opt.icp_distances
        if any(not (math.isfinite(d) and d > 0) for d in icp_distances):
            raise SystemExit("--icp_distances must be positive")
        if opt.icp_voxel_sizes is not None and len(opt.icp_voxel_sizes) != len(icp_distances):
            raise SystemExit(f"--icp_voxel_sizes has {len(opt.icp_voxel_sizes)} values for {len(icp_distances)} ICP stages: give one per stage")
        if opt.icp_voxel_sizes is not None and any(not (math.isfinite(v) and v > 0) for v in opt.icp_voxel_sizes):
            raise SystemExit("--icp_voxel_sizes must be positive")
        if opt.icp_max_iterations < 1:
            raise SystemExit("--icp_max_iterations must be at least 1")
    for name in ("sample_spacing", "gt_sample_spacing"):
        value = getattr(opt, name)
        try:
            if value is not None:
                geometry.sample_density(value)
        except ValueError:
            raise SystemExit(f"--{name} must be positive (and its square within float64's range)")
    if opt.write_samples is not None and opt.sample_spacing is None:
        raise SystemExit("--write_samples needs --sample_spacing: without it the reconstruction is scored by its vertices")
    if opt.crop_file_ground_truth and opt.crop_file is None:
        raise SystemExit("--crop_file_ground_truth needs --crop_file")
    if opt.crop_file is not None and not os.path.isfile(opt.crop_file):
        raise SystemExit(f"{opt.crop_file}: no such file")
    crop_volume = None if opt.crop_file is None else read_crop_file(opt.crop_file)
    rec_colours = rec_faces = gt_faces = None
    if opt.sample_spacing is not None:
        rec, rec_colours, rec_faces = read_ply_mesh(opt.reconstruction)
        if len(rec_faces) == 0:
            raise SystemExit(f"{opt.reconstruction}: --sample_spacing needs a mesh, and this file has no faces")
    else:
        rec = read_ply_points(opt.reconstruction)
    if opt.gt_sample_spacing is not None:
        gt, _, gt_faces = read_ply_mesh(opt.ground_truth)
        if len(gt_faces) == 0:
            raise SystemExit(f"{opt.ground_truth}: --gt_sample_spacing needs a mesh, and this file has no faces")
    else:
        gt = read_ply_points(opt.ground_truth)
    log.info(f"Read {len(rec)} points from {opt.reconstruction} and {len(gt)} from {opt.ground_truth}.")
    _require_gpu("eval_geometry", "the cloud distances are HIP kernels")
    import torch
    transform = None
    if opt.transform is not None:
        try:
            transform = np.loadtxt(opt.transform, dtype=np.float64).reshape(4, 4)
        except ValueError:
            raise SystemExit(f"{opt.transform}: expected 16 numbers, a 4x4 matrix")
    elif opt.ace_pose_file is not None:
        from .evaluate import evaluate_poses, read_pose_pairs
        estimates, ground_truth, confidences, _ = read_pose_pairs(opt.ace_pose_file, opt.gt_pose_files)
        if not len(estimates):
            raise SystemExit("no (estimate, ground truth) pose pairs to align with")
        res = evaluate_poses(estimates, ground_truth, confidences, estimate_alignment_conf_threshold=opt.estimate_alignment_conf_threshold,
                             seed=opt.seed)
        if res["T"] is None:
            raise SystemExit("the alignment of the estimated poses to the ground-truth poses failed: too few confident poses, or no "
                             "consistent similarity")
        transform = np.linalg.inv(res["T"])                       # T maps ground truth -> estimates (its rotation part carries the scale)
        log.info(f"Aligned on {len(estimates)} pose pairs: scale {res['scale']:.6f} (ground truth -> reconstruction), median pose error "
                 f"{res['median_r_deg']:.2f}deg, {res['median_t_cm']:.1f}cm.")
    t0 = time.perf_counter()
    device = lambda a: None if a is None else torch.from_numpy(a).cuda()
    try:
        res, scored, colours = geometry.score_reconstruction(
            device(rec), device(gt), opt.thresholds, rec_faces=device(rec_faces), rec_colours=device(rec_colours), gt_faces=device(gt_faces),
            transform=transform, sample_spacing=opt.sample_spacing, gt_sample_spacing=opt.gt_sample_spacing, sample_seed=opt.sample_seed,
            crop_volume=crop_volume, crop_ground_truth=opt.crop_file_ground_truth, icp_distances=icp_distances,
            icp_voxels=opt.icp_voxel_sizes, icp_max_iterations=opt.icp_max_iterations, icp_scale=opt.icp_scale, voxel=opt.voxel_size,
            crop=opt.crop, max_distance=opt.max_distance)
    except ValueError as e:
        raise SystemExit(str(e))
    for gt_, what in (("", "reconstruction"), ("gt_", "ground truth")):
        info = res.get("sampling", {})
        if gt_ + "spacing" in info:
            log.info(f"Sampled {info[gt_ + 'samples']} points, {info[gt_ + 'spacing']} m apart, from the {info[gt_ + 'faces']} faces of the "
                     f"{what} ({info[gt_ + 'area']:.4f} m^2; {info[gt_ + 'faces_invalid']} faces invalid).")
    if crop_volume is not None:
        info = res["crop_file"]
        log.info(f"Crop file {opt.crop_file}: {info['corners']} corners along {info['orthogonal_axis']}, "
                 f"{info['dropped']} reconstruction points dropped, {res['rec_points_read']} kept"
                 + (f"; {info['gt_dropped']} ground-truth points dropped" if opt.crop_file_ground_truth else "") + ".")
        res["crop_file"] = {"file": str(opt.crop_file), **info}
    for stage in res.get("icp", []):
        log.info(f"ICP stage at {stage['distance']} m: {stage['iterations']} iterations, {stage['status']}"
                 + (", the alignment before it kept" if stage["kept_previous"] else "")
                 + (f", fitness {stage['fitness'][-1] * 100:.2f}%, rmse {stage['rmse'][-1] * 1000:.3f} mm" if stage["iterations"] else ""))
    if opt.write_samples is not None:                             # as they are scored: cropped by the polygon, under the final alignment
        write_ply(opt.write_samples, scored.cpu().numpy(), np.full((scored.shape[0], 3), 200, np.uint8) if colours is None
                  else colours.cpu().numpy())
        log.info(f"Wrote {scored.shape[0]} samples to {opt.write_samples}.")
    t_device = time.perf_counter() - t0
    for line in geometry.log_lines(res):
        log.info(line)
    log.info(f"Upload + kernels + download {t_device:.2f} s.")
    if opt.output_json is not None:
        if opt.icp:
            # a stage without correspondences has rmse = sqrt(0 / 0): null in the file, which stays strict JSON
            res["icp"] = [{k: [x if math.isfinite(x) else None for x in v] if isinstance(v, list) else v for k, v in stage.items()}
                          for stage in res["icp"]]
        with open(opt.output_json, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


# ------------------------------------------------------------------------------------------------------- estimate_depth
def estimate_depth_parser():
    p = argparse.ArgumentParser(description="Estimate a depth map per image of an RGB reconstruction by plane-sweep stereo over "
                                            "neighbouring frames on the GPU and write them as 16-bit PNGs, the input of fuse_depth.py.",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("pose_file", type=Path, help="ACE pose file of the reconstruction (file qw qx qy qz tx ty tz f conf)")
    p.add_argument("rgb_files", type=str, help="glob of the RGB files, e.g. 'scene/*.jpg'")
    p.add_argument("output_dir", type=Path, help="folder for the depth maps: one 16-bit PNG per image of the glob, named after it")
    p.add_argument("--image_resolution", type=int, default=240, help="short side of the working images and of the depth maps")
    p.add_argument("--point_cloud", type=Path, default=None, help="the reconstruction's point cloud (.ply of ace_zero.py "
                                                                  "--export_point_cloud True or of export_point_cloud.py): gives every "
                                                                  "frame its depth range")
    p.add_argument("--cloud_convention", type=str, default="opencv", choices=["opengl", "opencv"],
                   help="coordinate convention of --point_cloud: ace_zero.py --export_point_cloud True writes OpenCV (pc_final.ply), "
                        "export_point_cloud.py OpenGL unless it is given --convention opencv")
    p.add_argument("--depth_range", type=float, nargs=2, default=None, metavar=("NEAR", "FAR"), help="one depth range in metres for all frames, "
                                                                                                   "instead of --point_cloud")
    p.add_argument("--planes", type=int, default=128, help="depth planes, uniform in inverse depth")
    p.add_argument("--sources", type=int, default=4, help="neighbouring frames to match each frame against (1 .. 8)")
    p.add_argument("--keep", type=int, default=None, help="the plane cost sums the KEEP best sources; default: half of them, rounded up")
    p.add_argument("--window", type=int, default=2, help="matching window radius in pixels (0 .. 4)")
    p.add_argument("--uniqueness", type=int, default=5, help="the best plane must beat every plane outside its neighbourhood by this many percent")
    p.add_argument("--tolerance", type=float, default=0.01, help="relative depth difference up to which a source's depth map agrees")
    p.add_argument("--min_consistent", type=int, default=2, help="a depth is kept if this many sources agree with it")
    p.add_argument("--confidence_threshold", type=float, default=1000, help="ignore pose-file entries below this confidence")
    p.add_argument("--depth_unit", type=float, default=0.001, help="metres per unit of the written depth maps (0.001: millimetres)")
    p.add_argument("--aggregation", type=str, default="none", choices=["none", "sgm"],
                   help="sgm: smooth the plane costs along scanlines before a plane is chosen (semi-global matching), so that textureless "
                        "walls inherit the depth of the texture around them instead of coming out empty")
    p.add_argument("--sgm_paths", type=int, default=None, choices=[4, 8], help="scanline directions of --aggregation sgm; default: 4")
    p.add_argument("--sgm_p1", type=int, default=None, help="penalty for moving one plane; default: 1.6 per sample of a cost "
                                                            "(KEEP * (2 WINDOW + 1)^2 samples)")
    p.add_argument("--sgm_p2", type=int, default=None, help="penalty for a jump of more than one plane; default: 12.8 per sample")
    return p


def estimate_depth_main(argv=None):
    """estimate_depth.py: images + pose file (+ point cloud) -> prefilter, plane sweep, consistency check (HIP) -> 16-bit depth PNGs."""
    import glob
    from concurrent.futures import ThreadPoolExecutor
    from . import mvs
    opt = estimate_depth_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    log = logging.getLogger("estimate_depth")
    if (opt.point_cloud is None) == (opt.depth_range is None):
        raise SystemExit("give exactly one of --point_cloud and --depth_range")
    if opt.depth_range is not None and not 0 < opt.depth_range[0] < opt.depth_range[1] < math.inf:
        raise SystemExit("--depth_range needs 0 < NEAR < FAR")
    if opt.image_resolution < 16:
        raise SystemExit("--image_resolution must be at least 16")
    if not 2 <= opt.planes <= 1024:
        raise SystemExit("--planes must be in 2 .. 1024")
    if not 1 <= opt.sources <= 8:
        raise SystemExit("--sources must be in 1 .. 8")
    if opt.keep is not None and not 1 <= opt.keep <= opt.sources:
        raise SystemExit("--keep must be in 1 .. --sources")
    if not 0 <= opt.window <= 4:
        raise SystemExit("--window must be in 0 .. 4")
    if not 0 <= opt.uniqueness <= 100:
        raise SystemExit("--uniqueness is a percentage (0 .. 100)")
    if not 0 <= opt.tolerance < math.inf:
        raise SystemExit("--tolerance must not be negative")
    if opt.min_consistent < 0:
        raise SystemExit("--min_consistent must not be negative")
    if not 0 < opt.depth_unit < math.inf:
        raise SystemExit("--depth_unit must be positive")
    sgm = opt.aggregation == "sgm"
    if not sgm and (opt.sgm_paths is not None or opt.sgm_p1 is not None or opt.sgm_p2 is not None):
        raise SystemExit("--sgm_paths, --sgm_p1 and --sgm_p2 need --aggregation sgm")
    if sgm:
        keep_most = opt.keep if opt.keep is not None else -(-opt.sources // 2)
        p1, p2 = mvs.sgm_penalties(keep_most, opt.window, opt.sgm_p1, opt.sgm_p2)
        if not 1 <= p1 <= p2 <= 32767:
            raise SystemExit("--sgm_p1 and --sgm_p2 need 1 <= P1 <= P2 <= 32767")
    rgb_files = sorted(glob.glob(opt.rgb_files))
    if not rgb_files:
        raise SystemExit(f"no files match {opt.rgb_files!r}")
    stems = [os.path.splitext(os.path.basename(f))[0] for f in rgb_files]
    if len(set(stems)) != len(stems):
        raise SystemExit("two images of the glob share a name: their depth maps would overwrite each other")
    try:
        c2w_all, focals_all, pose_row = read_posed_images(opt.pose_file, rgb_files, opt.confidence_threshold)
    except ValueError as e:
        raise SystemExit(str(e))
    cloud = None
    if opt.point_cloud is not None:
        cloud = read_ply_vertices(opt.point_cloud).astype(np.float64)
        if opt.cloud_convention == "opengl":
            cloud[:, 1], cloud[:, 2] = -cloud[:, 1], -cloud[:, 2]
    _require_gpu("estimate_depth", "plane-sweep stereo is a HIP kernel")
    t0 = time.perf_counter()
    grey, image_h = mvs.load_grey_frames(rgb_files, opt.image_resolution)
    t_decode = time.perf_counter() - t0
    n = len(rgb_files)
    c2w = np.full((n, 4, 4), np.nan)
    focals = np.ones(n)
    ranges = [None] * n
    for f, k in enumerate(pose_row):
        if k is None:
            continue
        h, w = grey[f].shape
        c2w[f] = c2w_all[k]
        focals[f] = focal_at_height(focals_all[k], h, image_h[f])
        if cloud is None:
            ranges[f] = tuple(opt.depth_range)
        else:
            ranges[f] = mvs.depth_range_from_cloud(cloud, np.linalg.inv(c2w[f]), focals[f], w / 2.0, h / 2.0, h, w)
    scene_depth = np.array([math.sqrt(r[0] * r[1]) if r is not None else np.nan for r in ranges])
    sources = mvs.select_sources(c2w, focals, [g.shape for g in grey], scene_depth, opt.sources)
    sources = [s if r is not None else [] for s, r in zip(sources, ranges)]
    t0 = time.perf_counter()
    info = {}
    maps = mvs.estimate_depth_maps(grey, cam_to_world=np.where(np.isfinite(c2w), c2w, np.eye(4)), focals=focals, sources=sources, ranges=ranges,
                                   planes=opt.planes, window=opt.window, keep=opt.keep, uniqueness=opt.uniqueness, tolerance=opt.tolerance,
                                   min_consistent=opt.min_consistent, depth_unit=opt.depth_unit, aggregation=opt.aggregation if sgm else None,
                                   sgm_paths=opt.sgm_paths, sgm_p1=opt.sgm_p1, sgm_p2=opt.sgm_p2, info=info)
    t_device = time.perf_counter() - t0
    t0 = time.perf_counter()
    os.makedirs(opt.output_dir, exist_ok=True)
    with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as pool:
        list(pool.map(write_depth_png, [os.path.join(opt.output_dir, s + ".png") for s in stems], maps))
    t_write = time.perf_counter() - t0
    estimated = sum(1 for s in sources if s)
    filled = float(np.mean([float((m > 0).mean()) for m, s in zip(maps, sources) if s])) if estimated else 0.0
    log.info(f"Estimated {estimated} of {n} depth maps ({opt.planes} planes, up to {opt.sources} sources, window radius {opt.window}); "
             f"{n - estimated} frames without a usable pose, range or neighbour got an empty map.")
    if sgm:
        log.info(f"Aggregation: sgm, {opt.sgm_paths or mvs.SGM_PATHS} paths, P1 / P2 = {p1} / {p2} at KEEP = {keep_most}; scratch (cost volume and "
                 f"aggregated costs, one pair per stream) {info.get('sgm_scratch_bytes', 0) / 2 ** 20:.1f} MiB.")
    else:
        log.info("Aggregation: none (each pixel's best plane on its own).")
    log.info(f"Pixels with a depth in the estimated maps: {100.0 * filled:.1f} %.")
    log.info(f"Decode {t_decode:.2f} s, upload + kernels + download {t_device:.2f} s, write {t_write:.2f} s.")
    log.info(f"Done. Wrote depth maps to: {opt.output_dir}")
    return 0
