"""Pose evaluation against ground truth on the MI355X: eval_poses_util.py / eval_poses.py of the reference.

    from acezero_amd.evaluate import TestEstimate, estimate_alignment, evaluate_poses
    T, scale = estimate_alignment(estimates, confidence_threshold=500, estimate_scale=True)     # (None, 1) if it failed
    res = evaluate_poses(poses_est_c2w, poses_gt_c2w, confidences)                           # accuracy, medians, per-frame errors

The RANSAC over similarity transforms, the refinement and the per-frame errors run in libacez.so (align_api.hip, fp64). The
sample triples come from a counter-based stream keyed by `seed` (the reference draws them with Python's `random.sample`);
pass `samples` (int [ransac_iterations][3], indices into the confident frames in frame order) to replay a given set of draws.
There is no CPU path: without a GPU the calls raise."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _native as N
from .formats import read_pose_file

# eval_poses_util.py:11-17
TestEstimate = namedtuple("TestEstimate", ["pose_est", "pose_gt", "focal_length", "confidence", "image_file"])

DEFAULT_SEED = 0x5EED_A11C

_ctx = {}


def _context(n, h):
    """One device context per process, regrown when a call needs more frames or hypotheses."""
    c = _ctx.get("c")
    if c is not None and c[1] >= n and c[2] >= h:
        return c[0]
    lib = N.lib()
    if c is not None:
        lib.acez_align_destroy(c[0])
        _ctx.pop("c")
    n2, h2 = max(n, 16), max(h, 1)
    handle = C.c_void_p()
    N.check(lib.acez_align_create(C.byref(handle), n2, h2, -1))
    _ctx["c"] = (handle, n2, h2)
    return handle


def _run(poses_est, poses_gt, confidences, *, confidence_threshold, estimate_alignment, estimate_scale, min_confident_estimates,
         threshold_t, threshold_r, ransac_iterations, refinement_max_hyp, refinement_max_it, seed, samples, want_scores=False):
    est = np.ascontiguousarray(np.asarray(poses_est, np.float64).reshape(-1, 4, 4))
    gt = np.ascontiguousarray(np.asarray(poses_gt, np.float64).reshape(-1, 4, 4))
    conf = np.ascontiguousarray(np.asarray(confidences, np.float64).reshape(-1))
    n = len(est)
    if not (len(gt) == n == len(conf)) or n == 0:
        raise ValueError(f"need one GT pose and one confidence per estimate (got {len(est)}, {len(gt)}, {len(conf)})")
    H = int(ransac_iterations)
    tab = None
    if samples is not None:
        tab = np.ascontiguousarray(np.asarray(samples).astype(np.int32).reshape(-1, 3))
        if len(tab) != H:
            raise ValueError(f"samples has {len(tab)} rows, ransac_iterations is {H}")
    prm = N.AlignParams(float(threshold_t), float(threshold_r), float(confidence_threshold), int(bool(estimate_alignment)),
                        int(bool(estimate_scale)), int(min_confident_estimates), H, int(refinement_max_hyp), int(refinement_max_it),
                        int(seed) & (2 ** 64 - 1))
    ctx = _context(n, H)
    T = np.zeros(16, np.float64)
    scale = C.c_double()
    status = C.c_int32()
    acc = C.c_int32()
    t_err = np.zeros(n, np.float64)
    r_err = np.zeros(n, np.float64)
    scores = np.zeros(H, np.int32) if want_scores else None
    valid = np.zeros(H, np.int32) if want_scores else None
    rc = N.lib().acez_align_evaluate(ctx, gt.ctypes.data, est.ctypes.data, conf.ctypes.data, n, C.byref(prm),
                                     tab.ctypes.data if tab is not None else None, T.ctypes.data, C.byref(scale), C.byref(status),
                                     scores.ctypes.data if want_scores else None, valid.ctypes.data if want_scores else None,
                                     t_err.ctypes.data, r_err.ctypes.data, C.byref(acc))
    N.check(rc)
    out = {"T": T.reshape(4, 4) if status.value == 0 else None, "scale": scale.value if status.value == 0 else 1,
           "t_err": t_err, "r_err": r_err, "accurate": acc.value}
    if want_scores:
        out["scores"], out["valid"] = scores, valid.astype(bool)
    return out


def estimate_alignment(estimates, confidence_threshold, min_cofident_estimates=10, inlier_threshold_t=0.05, inlier_threshold_r=5,
                       ransac_iterations=10000, refinement_max_hyp=12, refinement_max_it=8, estimate_scale=False, *,
                       seed=DEFAULT_SEED, samples=None):
    """eval_poses_util.estimate_alignment (same signature, same misspelt keyword): the similarity (estimate_scale) or rigid
    transform T that maps GT cam->world poses onto the estimates, and its scale; (None, 1) with fewer than
    min_cofident_estimates confident frames (confidence strictly above the threshold, finite GT) or when no hypothesis survives."""
    est = [e.pose_est for e in estimates]
    if not est:
        return None, 1
    r = _run(est, [e.pose_gt for e in estimates], [e.confidence for e in estimates], confidence_threshold=confidence_threshold,
             estimate_alignment=True, estimate_scale=estimate_scale, min_confident_estimates=min_cofident_estimates,
             threshold_t=inlier_threshold_t, threshold_r=inlier_threshold_r, ransac_iterations=ransac_iterations,
             refinement_max_hyp=refinement_max_hyp, refinement_max_it=refinement_max_it, seed=seed, samples=samples)
    return r["T"], r["scale"]


def median_of_sorted(values):
    """eval_poses.py:172-177: the element at index n // 2 of list.sort()'s order (Python floats, so NaN behaves as it does there)."""
    v = [float(x) for x in values]
    v.sort()
    return v[len(v) // 2]


def evaluate_poses(poses_est, poses_gt, confidences, *, estimate_alignment=True, estimate_alignment_scale=True,
                   estimate_alignment_conf_threshold=500, pose_error_thresh_t=0.05, pose_error_thresh_r=5, min_cofident_estimates=10,
                   ransac_iterations=10000, refinement_max_hyp=12, refinement_max_it=8, seed=DEFAULT_SEED, samples=None,
                   return_scores=False):
    """eval_poses.py:108-190 on arrays (cam->world 4x4 estimates and GT, one confidence per frame). Returns a dict:
    accuracy (percent), median_r_deg, median_t_cm, accurate (count), t_err (metres), r_err (degrees), T (None if the alignment
    failed), scale; with return_scores also the per-hypothesis scores and sample-test flags."""
    r = _run(poses_est, poses_gt, confidences, confidence_threshold=estimate_alignment_conf_threshold,
             estimate_alignment=estimate_alignment, estimate_scale=estimate_alignment_scale, min_confident_estimates=min_cofident_estimates,
             threshold_t=pose_error_thresh_t, threshold_r=pose_error_thresh_r, ransac_iterations=ransac_iterations,
             refinement_max_hyp=refinement_max_hyp, refinement_max_it=refinement_max_it, seed=seed, samples=samples,
             want_scores=return_scores)
    n = len(r["t_err"])
    r["median_r_deg"] = median_of_sorted(r["r_err"])
    r["median_t_cm"] = median_of_sorted(r["t_err"] * 100)
    r["accuracy"] = r["accurate"] / n * 100
    return r


def read_pose_file_with_confidence(path):
    """eval_poses.py:60-88: every line of an ACE pose file -> {file name: (cam->world 4x4 float64, confidence)}; a later line of the
    same name replaces an earlier one (formats.read_ace_pose_file instead drops low-confidence lines)."""
    return {e.file: (np.linalg.inv(e.w2c), e.confidence) for e in read_pose_file(path)}


def load_gt_pose_files(pattern):
    """dataset_io.load_pose_files: sorted glob, np.loadtxt, then .float() (the reference converts GT to float32 before it evaluates)."""
    import glob
    return [np.loadtxt(p).astype(np.float32).astype(np.float64) for p in sorted(glob.glob(pattern))]


def read_pose_pairs(ace_pose_file, gt_glob):
    """What eval_poses.py and eval_geometry.py align on: the pose file's estimates in the sorted order of their names, zipped with
    the sorted ground-truth files (the shorter list decides). Returns (estimates [n,4,4], ground truth [n,4,4], confidences [n],
    number of estimates read); n may be 0."""
    estimates = read_pose_file_with_confidence(ace_pose_file)
    pairs = list(zip([estimates[key] for key in sorted(estimates.keys())], load_gt_pose_files(gt_glob)))
    stack = lambda rows: np.stack(rows) if rows else np.zeros((0, 4, 4))
    return stack([p[0][0] for p in pairs]), stack([p[1] for p in pairs]), np.array([p[0][1] for p in pairs]), len(estimates)


def log_lines(res):
    """The two summary lines eval_poses.py logs at the end."""
    return [f"Accuracy: {res['accuracy']:.1f}%", f"Median Error: {res['median_r_deg']:.1f}deg, {res['median_t_cm']:.1f}cm"]


__all__ = ["TestEstimate", "estimate_alignment", "evaluate_poses", "median_of_sorted", "read_pose_file_with_confidence",
           "load_gt_pose_files", "read_pose_pairs", "log_lines", "DEFAULT_SEED"]
