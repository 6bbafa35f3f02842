"""GPU: pose evaluation on the MI355X (acezero_amd.evaluate, align_api.hip) against the reference's recorded runs
(tests/golden/eval_*.npz, tests/golden/make_eval_golden.py): replayed samples, the device's own sample stream, edge cases, the
eval_poses.py script on files, and a reconstruction of the synthetic room scored end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
from tests.eval_cases import CASES, write_case_files  # noqa: E402

# own stream vs the reference's draws (spread measured over three other sample streams with tests/eval_restated.py on traj_n12,
# traj_n500 and lowconf_nan: T entries <= 3.1e-2, scale <= 0.6 %, medians <= 0.6 cm / 0.14 deg)
OWN_STREAM_T_ATOL = 5e-2
OWN_STREAM_SCALE_RTOL = 1e-2
OWN_STREAM_MEDIAN_CM = 1.0
OWN_STREAM_MEDIAN_DEG = 0.25
RUNS = [(c, int(s)) for c, spec in CASES.items() for s in spec["scales"]]
WELL = [(c, int(s)) for c, spec in CASES.items() for s in spec["well"] if spec.get("align", True)]


def _gold(case):
    return np.load(os.path.join(GOLD, f"eval_{case}.npz"))


def _spec(case):
    return CASES[case]


def _evaluate(case, scale, **kw):
    from acezero_amd.evaluate import evaluate_poses
    z = _gold(case)
    return z, evaluate_poses(z["est"], z["gt"], z["conf"], estimate_alignment_scale=bool(scale),
                             estimate_alignment=_spec(case).get("align", True), **kw)


def _shortlist_degenerate(z, p):
    """True if a degenerate sample is among the reference's 12 shortlisted hypotheses (its rotation is not unique: declared
    deviation 2), so the final alignment is not compared exactly."""
    from tests.eval_restated import stable_order
    order = stable_order(z[p + "scores"], z[p + "valid"])[:12]
    return bool(z[p + "degenerate"][order].any()) if len(order) else False


def _assert_same_outcome(z, p, r, exact_errors):
    assert (r["T"] is None) == bool(z[p + "failed"])
    if exact_errors:
        if r["T"] is not None:
            Tg = z[p + "T"]
            np.testing.assert_allclose(r["T"], Tg, rtol=1e-9, atol=1e-9 * np.abs(Tg).max())
            assert abs(r["scale"] - float(z[p + "scale"])) <= 1e-9 * abs(float(z[p + "scale"]))
        fin = np.isfinite(z[p + "t_err"])
        assert np.array_equal(fin, np.isfinite(r["t_err"]))
        np.testing.assert_allclose(r["t_err"][fin], z[p + "t_err"][fin], rtol=1e-9, atol=1e-9)
        fin = np.isfinite(z[p + "r_err"])
        assert np.array_equal(fin, np.isfinite(r["r_err"]))
        np.testing.assert_allclose(r["r_err"][fin], z[p + "r_err"][fin], rtol=1e-9, atol=1e-9)
    assert r["accurate"] == int(z[p + "accurate"])
    assert r["median_t_cm"] == pytest.approx(float(z[p + "median_t_cm"]), rel=1e-9, abs=1e-9) or \
        (np.isinf(r["median_t_cm"]) and np.isinf(float(z[p + "median_t_cm"])))
    assert r["median_r_deg"] == pytest.approx(float(z[p + "median_r_deg"]), rel=1e-9, abs=1e-9) or \
        (np.isinf(r["median_r_deg"]) and np.isinf(float(z[p + "median_r_deg"])))


@pytest.mark.parametrize("case,scale", RUNS)
def test_replayed_samples_match_reference(case, scale):
    """The reference's own random.sample draws, replayed: per-hypothesis scores and sample tests, the alignment and the errors."""
    z = _gold(case)
    p = f"s{scale}_"
    tri = z[p + "triples"]
    align = _spec(case).get("align", True)
    _, r = _evaluate(case, scale, samples=tri if len(tri) else None, return_scores=True,
                     ransac_iterations=len(tri) if len(tri) else 10000)
    if len(tri) and r.get("scores") is not None and r["scores"].any():
        cmp = ~z[p + "boundary"] & ~z[p + "degenerate"]
        assert np.array_equal(r["scores"][cmp], z[p + "scores"][cmp].astype(np.int32))
        assert np.array_equal(r["valid"][cmp], z[p + "valid"][cmp])
    _assert_same_outcome(z, p, r, exact_errors=not align or not _shortlist_degenerate(z, p))


@pytest.mark.parametrize("case,scale", WELL)
def test_own_stream_reaches_reference_outcome(case, scale):
    """Counter-based samples instead of the reference's: the same outcome and accuracy count, the alignment and medians close (not
    equal: the reference's refinement returns the transform solved on the previous inlier set, so the final T depends on the hypothesis
    that heads the shortlist -- the reference's own eval_poses.py, which never seeds `random`, varies the same way from run to run).
    Two runs are bitwise identical; another seed gives the same accuracy."""
    z, a = _evaluate(case, scale)
    p = f"s{scale}_"
    assert (a["T"] is None) == bool(z[p + "failed"])
    assert a["accurate"] == int(z[p + "accurate"])
    if a["T"] is not None:
        np.testing.assert_allclose(a["T"], z[p + "T"], atol=OWN_STREAM_T_ATOL * max(1.0, float(z[p + "scale"])))
        assert abs(a["scale"] / float(z[p + "scale"]) - 1) < OWN_STREAM_SCALE_RTOL
        if np.all(np.isfinite(z[p + "t_err"])):   # with NaN errors, list.sort()'s order (and so the "median") depends on every value
            assert abs(a["median_t_cm"] - float(z[p + "median_t_cm"])) < OWN_STREAM_MEDIAN_CM
            assert abs(a["median_r_deg"] - float(z[p + "median_r_deg"])) < OWN_STREAM_MEDIAN_DEG
    _, b = _evaluate(case, scale)
    assert (a["T"] is None) == (b["T"] is None)
    if a["T"] is not None:
        assert np.array_equal(a["T"].view(np.uint64), b["T"].view(np.uint64)) and a["scale"] == b["scale"]
    assert np.array_equal(a["t_err"].view(np.uint64), b["t_err"].view(np.uint64))
    assert np.array_equal(a["r_err"].view(np.uint64), b["r_err"].view(np.uint64))
    _, c = _evaluate(case, scale, seed=12345)
    assert c["accurate"] == a["accurate"]


def test_edge_cases_give_reference_outcomes():
    from acezero_amd.evaluate import TestEstimate, estimate_alignment
    # too few confident frames, and no surviving hypothesis: (None, 1), every error inf, accuracy 0
    for case in ("fewconf", "nosurvive"):
        z, r = _evaluate(case, 1)
        assert bool(z["s1_failed"]) and r["T"] is None and r["scale"] == 1
        assert np.all(np.isinf(r["t_err"])) and np.all(np.isinf(r["r_err"])) and r["accuracy"] == 0.0
        ests = [TestEstimate(z["est"][i], z["gt"][i], None, z["conf"][i], None) for i in range(len(z["est"]))]
        assert estimate_alignment(ests, 500, estimate_scale=True) == (None, 1)
    # static-camera runs, NaN / inf GT rows with low-confidence rows
    for case, scale in (("static", 0), ("static", 1), ("lowconf_nan", 1)):
        z, r = _evaluate(case, scale)
        p = f"s{scale}_"
        assert (r["T"] is None) == bool(z[p + "failed"])
        assert r["accurate"] == int(z[p + "accurate"])
    z, r = _evaluate("lowconf_nan", 1)
    bad = ~np.all(np.isfinite(z["gt"]), axis=(1, 2))
    nan = np.isnan(r["t_err"]) | np.isnan(r["r_err"])             # a NaN in the rotation block reaches r_err only
    assert bad.sum() == 8 and np.array_equal(nan, bad)
    assert np.array_equal(np.isnan(r["t_err"]), np.isnan(z["s1_t_err"])) and np.array_equal(np.isnan(r["r_err"]), np.isnan(z["s1_r_err"]))
    # --estimate_alignment False: T = I, scale 1
    z, r = _evaluate("noalign", 1)
    assert np.array_equal(r["T"], np.eye(4)) and r["scale"] == 1.0
    _assert_same_outcome(z, "s1_", r, exact_errors=True)


def test_eval_poses_script_on_files(tmp_path):
    """eval_poses.py on files: the accuracy line equals the reference's; the median line agrees within the spread between sample
    streams (the reference draws from an unseeded `random`)."""
    z = _gold("traj_n500")
    pose_file, pattern = write_case_files(str(tmp_path), z["est"], z["gt"], z["conf"])
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "eval_poses.py"), pose_file, pattern],
                         cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln.split(":", 2)[-1] for ln in out.stderr.splitlines()]
    acc = [ln for ln in lines if ln.startswith("Accuracy:")]
    med = [ln for ln in lines if ln.startswith("Median Error:")]
    ref = list(z["script_lines"])
    assert acc == [ref[0]], (acc, ref)
    assert len(med) == 1 and sum(ln.startswith("Rotation Error:") for ln in lines) == 500

    def parse(ln):
        r, t = ln[len("Median Error: "):].split(", ")
        return float(r[:-3]), float(t[:-2])
    (r1, t1), (r0, t0) = parse(med[0]), parse(ref[1])
    assert abs(r1 - r0) <= OWN_STREAM_MEDIAN_DEG + 0.05 and abs(t1 - t0) <= OWN_STREAM_MEDIAN_CM + 0.05, (med, ref)


def test_reconstruction_of_synthetic_room_scores_within_bounds(tmp_path):
    """ace_zero's loop on the synthetic room, poses_final.txt scored with evaluate_poses against the rendered cameras: no more than
    tests/test_session_gpu.py already establishes (centres within 5 cm after alignment, metric scale from the seed's depth)."""
    import torch
    from acezero_amd import synth
    from acezero_amd.evaluate import evaluate_poses, read_pose_file_with_confidence
    from acezero_amd.session import ReconstructionSession, default_options, write_pose_file
    seq = synth.render_room_sequence(seed=2089, n_frames=72, arc_deg=36.0, device="cuda")
    esd = {k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}
    it = 3000
    opt = default_options(use_external_focal_length=seq["focal"], try_seeds=2, seed_iterations=it, iterations=it, refit_iterations=it,
                          iterations_max=8, final_refit_posewait=it // 5, learning_rate_warmup_iterations=it // 5,
                          cooldown_iterations=it // 5, aug_rotation=2, aug_scale=1.06, aug_black_white=0.02)
    res = ReconstructionSession(esd, seq["images"], opt=opt, depth=seq["depth"]).reconstruct()
    n = seq["images"].shape[0]
    names = [f"frame_{i:04d}.png" for i in range(n)]
    write_pose_file(str(tmp_path / "poses_final.txt"), names, res["poses"], res["confidence"], res["focal"])
    est = read_pose_file_with_confidence(str(tmp_path / "poses_final.txt"))
    est_poses = np.stack([est[k][0] for k in sorted(est)])
    conf = np.array([est[k][1] for k in sorted(est)])
    gt = seq["poses"].cpu().numpy().astype(np.float64)
    r = evaluate_poses(est_poses, gt, conf, estimate_alignment_conf_threshold=opt.registration_confidence)
    assert r["T"] is not None
    assert 0.8 < r["scale"] < 1.25, r["scale"]
    assert r["median_t_cm"] < 5.0, r["median_t_cm"]
