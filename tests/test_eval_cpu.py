"""CPU: pose evaluation (eval_poses.py / acezero_amd.evaluate) -- the command-line surface and API against the reference's, the ABI
without a device, and the numpy restatement of the device algorithm (tests/eval_restated.py) against the reference's fixtures."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest
import torch

from acezero_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _ref_api():
    with open(os.path.join(GOLD, "eval_flags.json")) as f:
        return json.load(f)


def test_eval_poses_parser_matches_reference_flags():
    from acezero_amd.cli import eval_parser
    ref = _ref_api()["eval_poses"]
    ours = {a.dest: a for a in eval_parser()._actions if a.dest != "help"}
    for dest, r in ref.items():
        a = ours[dest]
        assert list(a.option_strings) == r["flags"], dest
        assert a.default == r["default"], dest
        assert a.help == r["help"], dest
    for dest in set(ours) - set(ref):
        assert ours[dest].help.startswith("[additive]"), dest
    opt = eval_parser().parse_args(["p.txt", "gt/*.txt", "--estimate_alignment", "False", "--estimate_alignment_scale", "no"])
    assert opt.estimate_alignment is False and opt.estimate_alignment_scale is False and opt.pose_error_thresh_t == 0.05


def test_evaluate_module_signature_matches_reference():
    import eval_poses_util
    from acezero_amd import evaluate
    api = _ref_api()
    params = inspect.signature(evaluate.estimate_alignment).parameters
    pos = [(p.name, None if p.default is inspect.Parameter.empty else p.default) for p in params.values()
           if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert [list(x) for x in pos] == api["estimate_alignment"]
    assert list(evaluate.TestEstimate._fields) == api["TestEstimate"]
    assert eval_poses_util.estimate_alignment is evaluate.estimate_alignment
    assert eval_poses_util.TestEstimate is evaluate.TestEstimate


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_align_entry_points_fail_without_device():
    lib = N.lib()
    h = C.c_void_p()
    assert lib.acez_align_create(C.byref(h), 100, 100, -1) == -3
    assert b"no HIP device" in lib.acez_last_error()
    from acezero_amd import evaluate
    P = np.tile(np.eye(4), (12, 1, 1))
    with pytest.raises(RuntimeError):
        evaluate.evaluate_poses(P, P, np.full(12, 1000.0))
    with pytest.raises(RuntimeError):
        evaluate.estimate_alignment([evaluate.TestEstimate(P[i], P[i], None, 1000.0, None) for i in range(12)], 500)


def test_stable_shortlist_keeps_ascending_index_on_ties():
    from tests.eval_restated import stable_order
    scores = np.array([5, 7, 7, 3, 7, 5, 9])
    valid = np.array([1, 1, 0, 1, 1, 1, 0], bool)
    ref = sorted([dict(i=i, score=s) for i, s in enumerate(scores) if valid[i]], key=lambda x: x["score"], reverse=True)
    assert list(stable_order(scores, valid)) == [x["i"] for x in ref] == [1, 4, 0, 5, 3]


def test_median_is_element_n_half_of_sorted_list():
    from acezero_amd.evaluate import median_of_sorted
    assert median_of_sorted([3.0, 1.0, 2.0, 4.0]) == 3.0
    assert median_of_sorted([5.0]) == 5.0


# the restatement against the reference's recorded runs (the 3000-frame case takes a minute on a CPU: tools/eval_timing.py)
RESTATED = [("traj_n12", 1), ("traj_n12", 0), ("traj_n500", 1), ("traj_n500", 0), ("lowconf_nan", 1), ("static", 0), ("static", 1),
            ("fewconf", 1), ("nosurvive", 1)]


@pytest.mark.parametrize("case,scale", RESTATED)
def test_restatement_reproduces_reference_scores_and_alignment(case, scale):
    from tests.eval_restated import estimate_alignment
    z = np.load(os.path.join(GOLD, f"eval_{case}.npz"))
    p = f"s{scale}_"
    r = estimate_alignment(z["gt"], z["est"], z["conf"], z[p + "triples"], estimate_scale=bool(scale))
    if bool(z[p + "failed"]):
        assert r["T"] is None and r["scale"] == 1
        return
    cmp = ~z[p + "boundary"] & ~z[p + "degenerate"]
    assert cmp.sum() > 0.5 * len(cmp)
    assert np.array_equal(r["scores"][cmp], z[p + "scores"][cmp])
    assert np.array_equal(r["valid"][cmp], z[p + "valid"][cmp])
    assert r["T"] is not None
    np.testing.assert_allclose(r["T"], z[p + "T"], rtol=1e-9, atol=1e-9 * np.abs(z[p + "T"]).max())
    assert abs(r["scale"] - float(z[p + "scale"])) <= 1e-9 * abs(float(z[p + "scale"]))
