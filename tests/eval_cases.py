"""Inputs of the pose-evaluation fixtures (tests/golden/eval_*.npz, tests/golden/make_eval_golden.py): 7-Scenes-like camera
trajectories with a known similarity between ground truth and estimates, noise and gross outliers, plus the edge cases.
GT poses are float32 values (the reference loads GT files as float32 tensors); estimates are float64."""
import os

import numpy as np
from scipy.spatial.transform import Rotation

# name -> spec.  scales: the estimate_scale settings recorded.  well: the settings on which RANSAC + refinement reach the same
# inlier set from any stream of samples (the own-stream GPU tests use only these).
CASES = {
    "traj_n12": dict(n=12, seed=11, s=1.7, outliers=0.3, scales=(True, False), well=(True,)),
    "traj_n500": dict(n=500, seed=12, s=1.7, outliers=0.3, scales=(True, False), well=(True,), script=True),
    "traj_n3000": dict(n=3000, seed=13, s=1.0, outliers=0.3, scales=(True, False), well=(True, False)),
    "lowconf_nan": dict(n=300, seed=14, s=1.3, outliers=0.3, low_conf=0.25, nan_rows=5, inf_rows=3, scales=(True,), well=(True,)),
    "static": dict(n=200, seed=15, s=0.8, outliers=0.2, static_runs=10, scales=(False, True), well=()),
    "fewconf": dict(n=50, seed=16, s=1.0, outliers=0.0, n_confident=9, scales=(True,), well=(True,)),
    "nosurvive": dict(n=100, seed=17, s=1.0, outliers=1.0, scales=(True,), well=(True,)),
    "noalign": dict(n=100, seed=18, s=1.0, outliers=0.3, scales=(True,), well=(True,), align=False),
}


def _look_at(c, target, up=np.array([0.0, 1.0, 0.0])):
    z = target - c
    z = z / np.linalg.norm(z)
    x = np.cross(up, z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z], axis=1)    # cam -> world rotation (columns: camera axes in the world)


def make_inputs(spec):
    """(est [n,4,4] float64, gt [n,4,4] float64 holding float32 values, confidence [n] float64) cam -> world."""
    rng = np.random.RandomState(spec["seed"])
    n = spec["n"]
    th = np.linspace(0.0, 1.5 * np.pi, n)
    centres = np.stack([1.5 * np.cos(th), 0.3 * np.sin(2 * th) + 1.2, 1.5 * np.sin(th)], 1) + rng.normal(0, 0.01, (n, 3))
    if spec.get("static_runs"):
        run = spec["static_runs"]
        for s in range(0, n, 2 * run):                    # every other block of `run` frames: the camera stands still
            centres[s:s + run] = centres[s]
    gt = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        roll = Rotation.from_rotvec([0, 0, rng.normal(0, 0.05)]).as_matrix()
        gt[i, :3, :3] = _look_at(centres[i], np.array([0.0, 1.0, 0.0]) + rng.normal(0, 0.2, 3)) @ roll
        gt[i, :3, 3] = centres[i]
    gt = gt.astype(np.float32).astype(np.float64)
    R = Rotation.random(random_state=rng).as_matrix()
    t = rng.normal(0, 2.0, 3)
    s = spec["s"]
    est = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        noise = Rotation.from_rotvec(rng.normal(0, np.radians(0.3), 3)).as_matrix()
        est[i, :3, :3] = R @ gt[i, :3, :3] @ noise
        est[i, :3, 3] = s * (R @ gt[i, :3, 3]) + t + rng.normal(0, 0.005 * s, 3)
    n_out = int(round(spec["outliers"] * n))
    for i in rng.choice(n, n_out, replace=False):
        est[i, :3, :3] = Rotation.random(random_state=rng).as_matrix()
        est[i, :3, 3] = rng.uniform(-3, 3, 3) * s + t
    conf = rng.randint(1000, 5000, n).astype(np.float64)
    if spec.get("low_conf"):
        low = rng.choice(n, int(spec["low_conf"] * n), replace=False)
        conf[low] = rng.randint(0, 501, len(low))
        conf[low[:5]] = 500.0                               # at the threshold: not confident (strictly greater)
    if spec.get("n_confident") is not None:
        conf[:] = 100.0
        conf[rng.choice(n, spec["n_confident"], replace=False)] = 2000.0
    bad = rng.choice(n, spec.get("nan_rows", 0) + spec.get("inf_rows", 0), replace=False)
    for j, i in enumerate(bad):
        gt[i, rng.randint(3), rng.randint(4)] = np.nan if j < spec.get("nan_rows", 0) else np.inf
    return est, gt, conf


def write_case_files(d, est, gt, conf, focal=525.0):
    """An ACE pose file (the project's writer, world -> camera, integer confidences) and one GT .txt per frame (4x4 cam -> world).
    Returns (pose file path, GT glob pattern)."""
    from acezero_amd.cli import write_pose_line
    pose_file = os.path.join(d, "poses.txt")
    with open(pose_file, "w") as f:
        for i in range(len(est)):
            write_pose_line(f, f"seq/frame-{i:06d}.color.png", np.linalg.inv(est[i]), int(conf[i]), focal)
    os.makedirs(os.path.join(d, "gt"), exist_ok=True)
    for i in range(len(gt)):
        np.savetxt(os.path.join(d, "gt", f"frame-{i:06d}.pose.txt"), gt[i])
    return pose_file, os.path.join(d, "gt", "*.txt")
