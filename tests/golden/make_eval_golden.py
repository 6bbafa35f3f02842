"""Pose-evaluation fixtures from the REFERENCE's eval_poses_util.estimate_alignment and eval_poses.py -> tests/golden/eval_*.npz and
tests/golden/eval_flags.json.  Build container only (needs /root/reference; scipy 1.15.3; cv2 is not installed and is stubbed).

For every case the reference runs under random.seed(CASE_SEED) with random.sample wrapped, so the fixture holds the triples it drew.
Recorded per hypothesis: the score, the sample test (inliers[samples].sum() >= 3), a boundary flag (some frame's translation or
rotation error within 1e-9 of its threshold), a degenerate flag (second singular value of the sample covariance < 1e-12 x the
first).  Recorded per case: the final T / scale (or failed), and the per-frame errors of eval_poses.py:140-170.

Two restatements, both declared in DESIGN.md section 4d:
* cv2.Rodrigues (eval_poses.py:160) is replaced by scipy's magnitude of the SVD-orthonormalised matrix (R <- U V^T), which is what
  cv2.Rodrigues does first; UNPINNED here (no OpenCV in this image).
* scipy 1.15 raises inside get_inliers when a hypothesis is not finite (e.g. three coincident centres with estimate_scale: 0/0) or
  its rotation block is singular; the wrapper then marks every frame as an outlier (the device's rule). `guarded` counts those calls;
  on every case without such hypotheses the reference runs unmodified.

    python tests/golden/make_eval_golden.py [--flags-only]   # ~2-3 min, most of it the 3000-frame cases (prints the reference's CPU time)
"""
import argparse
import json
import math
import os
import random
import runpy
import sys
import tempfile
import time
from unittest.mock import MagicMock

import numpy as np
from scipy.spatial.transform import Rotation

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for name in ["torchvision", "torchvision.transforms", "torchvision.transforms.functional", "cv2"]:
    sys.modules.setdefault(name, MagicMock())
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)          # ahead of the repository root: `eval_poses_util` is the reference's, not the shim
import eval_poses_util as tutil  # noqa: E402  (the reference's)

from tests.eval_cases import CASES, make_inputs  # noqa: E402

BOUNDARY = 1e-9
_orig_get_inliers = tutil.get_inliers
_orig_kabsch = tutil.kabsch


def rodrigues_angle_deg(M):
    """Unpinned restatement of np.linalg.norm(cv2.Rodrigues(M)[0]) * 180 / pi: orthonormalise by SVD, then the angle (scipy)."""
    if not np.all(np.isfinite(M)):
        return math.nan
    U, _, Vt = np.linalg.svd(M)
    Q = U @ Vt
    if np.linalg.det(Q) <= 0:
        return math.nan
    return float(np.linalg.norm(Rotation.from_matrix(Q).as_rotvec()) * 180 / math.pi)


class Recorder:
    def __init__(self):
        self.triples, self.scores, self.valid, self.boundary, self.degenerate = [], [], [], [], []
        self.guarded = 0
        self.pending = None

    def sample(self, population, k):
        s = self._sample(population, k)
        self.triples.append(list(s))
        self.pending = list(s)
        return s

    def kabsch(self, pts1, pts2, estimate_scale=False):
        if self.pending is not None:
            c1 = pts1 - pts1.mean(axis=0)
            c2 = pts2 - pts2.mean(axis=0)
            S = np.linalg.svd(c1.T @ c2 / c1.shape[0], compute_uv=False)
            self.degenerate.append(bool(S[0] == 0 or S[1] < 1e-12 * S[0]))
        return _orig_kabsch(pts1, pts2, estimate_scale)

    def get_inliers(self, h_T, poses_gt, poses_est, thr_t, thr_r):
        if not np.all(np.isfinite(h_T)):
            inl = np.zeros(len(poses_gt), bool)
            self.guarded += 1
        else:
            try:
                inl = _orig_get_inliers(h_T, poses_gt, poses_est, thr_t, thr_r)
            except (ValueError, np.linalg.LinAlgError):
                inl = np.zeros(len(poses_gt), bool)
                self.guarded += 1
        if self.pending is not None:
            s = self.pending
            self.pending = None
            self.scores.append(int(inl.sum()))
            self.valid.append(bool(inl[s].sum() >= 3))
            self.boundary.append(self._boundary(h_T, poses_gt, poses_est, thr_t, thr_r))
        return inl

    @staticmethod
    def _boundary(h_T, poses_gt, poses_est, thr_t, thr_r):
        if not np.all(np.isfinite(h_T)):
            return False
        G = h_T @ poses_gt
        dt = np.linalg.norm(G[:, :3, 3] - poses_est[:, :3, 3], axis=1)
        if np.any(np.abs(dt - thr_t) <= BOUNDARY):
            return True
        near = dt < thr_t + BOUNDARY
        if not near.any():
            return False
        M = G[near, :3, :3] @ poses_est[near, :3, :3].transpose([0, 2, 1])
        try:
            mag = Rotation.from_matrix(M).magnitude()
        except (ValueError, np.linalg.LinAlgError):
            return False
        return bool(np.any(np.abs(mag - thr_r / 180 * math.pi) <= BOUNDARY))


def run_reference(est, gt, conf, estimate_scale, seed, thr_t=0.05, thr_r=5, conf_thr=500, align=True):
    rec = Recorder()
    rec._sample = random.sample
    random.seed(seed)
    ests = [tutil.TestEstimate(pose_est=est[i], pose_gt=gt[i], confidence=conf[i], image_file=None, focal_length=None) for i in range(len(est))]
    tutil.random.sample, tutil.kabsch, tutil.get_inliers = rec.sample, rec.kabsch, rec.get_inliers
    t0 = time.perf_counter()
    try:
        if align:
            T, scale = tutil.estimate_alignment(ests, confidence_threshold=conf_thr, estimate_scale=estimate_scale, inlier_threshold_t=thr_t,
                                                inlier_threshold_r=thr_r)
        else:
            T, scale = np.eye(4), 1.
    finally:
        tutil.random.sample, tutil.kabsch, tutil.get_inliers = rec._sample, _orig_kabsch, _orig_get_inliers
    secs = time.perf_counter() - t0
    # eval_poses.py:140-170
    t_err, r_err, acc = [], [], 0
    for i in range(len(est)):
        if T is not None:
            g = T @ gt[i]
            te = float(np.linalg.norm(g[0:3, 3] - est[i][0:3, 3])) / scale
            re = rodrigues_angle_deg(est[i][:3, :3] @ g[:3, :3].T)
        else:
            te, re = math.inf, math.inf
        t_err.append(te)
        r_err.append(re)
        acc += (re < thr_r and te < thr_t)
    tcm = [x * 100 for x in t_err]
    ts, rs = sorted(tcm), sorted(r_err)
    out = dict(failed=T is None, T=np.eye(4) * 0 if T is None else np.asarray(T), scale=float(scale), t_err=np.array(t_err),
               r_err=np.array(r_err), accurate=acc, median_t_cm=ts[len(ts) // 2], median_r_deg=rs[len(rs) // 2], guarded=rec.guarded)
    H = len(rec.triples)
    small = len(est) < 32768
    out.update(triples=np.array(rec.triples, np.int16 if small else np.int32).reshape(H, 3),
               scores=np.array(rec.scores, np.int16 if small else np.int32), valid=np.array(rec.valid, bool),
               boundary=np.array(rec.boundary, bool), degenerate=np.array(rec.degenerate, bool))
    return out, secs


def reference_script_lines(est, gt, conf, focal=525.0):
    """Run the reference's eval_poses.py (cv2 stubbed with the restated angle) on files written with the project's pose-file writer;
    return its log lines 'Accuracy: ...' and 'Median Error: ...'."""
    from tests.eval_cases import write_case_files
    import logging
    cv2 = sys.modules["cv2"]
    cv2.Rodrigues = lambda M: (np.array([rodrigues_angle_deg(M) * math.pi / 180, 0.0, 0.0]), None)
    sys.modules.setdefault("dataset_io", __import__("dataset_io"))
    lines = []

    class H(logging.Handler):
        def emit(self, r):
            lines.append(r.getMessage())
    with tempfile.TemporaryDirectory() as d:
        pose_file, pattern = write_case_files(d, est, gt, conf, focal)
        h = H()
        root = logging.getLogger()
        root.addHandler(h)
        root.setLevel(logging.INFO)      # the script's basicConfig(level=INFO) is a no-op once a handler exists
        argv = sys.argv
        sys.argv = ["eval_poses.py", pose_file, pattern]
        random.seed(0)
        try:
            runpy.run_path(os.path.join(REF, "eval_poses.py"), run_name="__main__")
        finally:
            sys.argv = argv
            logging.getLogger().removeHandler(h)
    return [x for x in lines if x.startswith("Accuracy:") or x.startswith("Median Error:")]


def flag_table():
    """The reference parser's surface (eval_poses.py:28-54), captured by making parse_args raise after construction."""
    box = {}

    class Captured(Exception):
        pass

    def fake_parse(self, *a, **k):
        box["p"] = self
        raise Captured()
    orig = argparse.ArgumentParser.parse_args
    argparse.ArgumentParser.parse_args = fake_parse
    sys.modules.setdefault("dataset_io", MagicMock())
    try:
        runpy.run_path(os.path.join(REF, "eval_poses.py"), run_name="__main__")
    except Captured:
        pass
    finally:
        argparse.ArgumentParser.parse_args = orig
    out = {}
    for act in box["p"]._actions:
        if act.dest == "help":
            continue
        out[act.dest] = {"flags": list(act.option_strings), "default": act.default, "help": act.help, "positional": not act.option_strings}
    return out


def api_table():
    """The reference parser's flags plus the public names eval_poses.py uses from eval_poses_util."""
    import inspect
    sig = inspect.signature(tutil.estimate_alignment)
    return {"eval_poses": flag_table(),
            "estimate_alignment": [[p.name, None if p.default is inspect.Parameter.empty else p.default] for p in sig.parameters.values()],
            "TestEstimate": list(tutil.TestEstimate._fields)}


def make_cases():
    timings = {}
    for name, spec in CASES.items():
        est, gt, conf = make_inputs(spec)
        arrays = dict(est=est, gt=gt, conf=conf)
        for scale in spec["scales"]:
            res, secs = run_reference(est, gt, conf, scale, spec["seed"], align=spec.get("align", True))
            timings[f"{name}/scale{int(scale)}"] = round(secs, 2)
            for k, v in res.items():
                arrays[f"s{int(scale)}_{k}"] = np.asarray(v)
        if spec.get("script"):
            arrays["script_lines"] = np.array(reference_script_lines(est, gt, conf))
        np.savez_compressed(os.path.join(HERE, f"eval_{name}.npz"), **arrays)
        print(name, {k: v for k, v in timings.items() if k.startswith(name + "/")}, flush=True)
    print("reference estimate_alignment CPU seconds:", json.dumps(timings))


if __name__ == "__main__":
    if "--flags-only" not in sys.argv:
        make_cases()
    with open(os.path.join(HERE, "eval_flags.json"), "w") as f:
        json.dump(api_table(), f, indent=1, sort_keys=True)
