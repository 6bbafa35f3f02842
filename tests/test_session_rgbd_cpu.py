"""CPU: host logic of the RGB-D mode of the reconstruction loop: the command-line flag, the option, the
up-front refusals, the centimetre reading of the RANSAC thresholds, and the scripted loop scenarios of tests/test_session_cpu.py
re-done with rgbd=True (every map depth-supervised, every registration the RGB-D estimator, the decisions unchanged)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from acezero_amd import cli, dsacstar, session


# ------------------------------------------------------------------------------------------------------------ command line, option
def test_parser_takes_rgbd_and_names_the_centimetre_convention(tmp_path):
    p = cli.ace_zero_cli_parser()
    base = ["scene/*.png", str(tmp_path / "out")]
    assert p.parse_args(base).rgbd is False                                      # additive: off by default
    assert p.parse_args(base + ["--rgbd", "True"]).rgbd is True
    assert p.parse_args(base + ["--rgbd", "False"]).rgbd is False
    hlp = " ".join(p.format_help().split())
    assert "--rgbd" in hlp and "CENTIMETRES" in hlp and "--depth_files" in hlp
    # every reference flag is still there, with its default
    ref, mine = vars(cli.ace_zero_parser().parse_args(base)), vars(p.parse_args(base))
    assert set(mine) - set(ref) == {"rgbd"} and all(mine[k] == v for k, v in ref.items())


def test_command_line_refuses_rgbd_without_depth_files_before_reading_any_frame(tmp_path):
    out = tmp_path / "out"
    with pytest.raises(SystemExit, match="--rgbd True needs --depth_files"):
        cli.ace_zero_main([str(tmp_path / "no_such_*.png"), str(out), "--rgbd", "True"])
    assert not out.exists()                                                       # nothing was started


def test_command_line_refuses_rgbd_under_torchrun(tmp_path, monkeypatch):
    import torch.distributed as dist
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(torch.cuda, "set_device", lambda *_: None)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    with pytest.raises(SystemExit, match="--rgbd True runs on one GPU"):
        cli.ace_zero_main([str(tmp_path / "rgb_*.png"), str(tmp_path / "out"), "--rgbd", "True", "--depth_files", str(tmp_path / "d_*.png")])


def test_default_options_has_rgbd_off_by_default():
    assert session.default_options().rgbd is False
    assert session.default_options(rgbd=True).rgbd is True
    assert "rgbd" in vars(session.default_options())                              # ace_zero_main hands every known option over by name


# -------------------------------------------------------------------------------------------------------------- up-front refusals
def test_session_in_rgbd_mode_without_full_depth_is_refused_before_encoding():
    """The refusal is taken on the arguments alone: an empty encoder state dict and no device are enough to see it."""
    opt = session.default_options(rgbd=True)
    img = torch.zeros(3, 1, 64, 96)                                               # 8 x 12 cells
    why = "depth map for every frame"
    with pytest.raises(RuntimeError, match=why):
        session.ReconstructionSession({}, img, opt=opt, depth=None)
    with pytest.raises(RuntimeError, match=why + ".*2 depth maps for 3 frames"):
        session.ReconstructionSession({}, img, opt=opt, depth=torch.ones(2, 8, 12))
    with pytest.raises(RuntimeError, match=why + ".*frame 1 has none"):
        session.ReconstructionSession({}, img, opt=opt, depth=[torch.ones(8, 12), None, torch.ones(8, 12)])
    with pytest.raises(RuntimeError, match=why + ".*frame 0's has .* cells for 8 x 12"):
        session.ReconstructionSession({}, img, opt=opt, depth=torch.ones(3, 6, 8))
    # every size class: frames 0, 2 are 64 x 96, frame 1 is 96 x 64; the portrait frame's map is missing, then of the wrong shape
    mixed = [([0, 2], torch.zeros(2, 1, 64, 96)), ([1], torch.zeros(1, 1, 96, 64))]
    with pytest.raises(RuntimeError, match=why + ".*frame 1 has none"):
        session.ReconstructionSession({}, mixed, opt=opt, depth=[torch.ones(8, 12), None, torch.ones(8, 12)])
    with pytest.raises(RuntimeError, match=why + ".*frame 1's has"):
        session.ReconstructionSession({}, mixed, opt=opt, depth=[torch.ones(8, 12)] * 3)
    session.check_rgbd_mode(mixed, [torch.ones(8, 12), torch.ones(12, 8), torch.ones(8, 12)])      # complete: accepted
    session.check_rgbd_mode(img, torch.ones(3, 8, 12))
    with pytest.raises(RuntimeError, match="--rgbd True runs on one GPU"):        # multi-rank: refused, not silently run unsharded
        session.check_rgbd_mode(img, torch.ones(3, 8, 12), world=2)


def test_rgb_mode_does_not_ask_for_depth():
    """rgbd off: the constructor's first complaint is what it always was (no GPU here, or the empty encoder on a GPU box) -- never depth."""
    with pytest.raises(Exception) as e:
        session.ReconstructionSession({}, torch.zeros(1, 1, 64, 96), opt=session.default_options(), depth=None)
    assert "depth map for every frame" not in str(e.value)


# ------------------------------------------------------------------------------------------------------- thresholds in centimetres
def test_ransac_params_names_the_unit_and_keeps_the_numbers():
    o = session.default_options(ransac_threshold=7.5, maxpixelerror=60.0, ransac_iterations=48)
    rgb, rgbd = session.ransac_params(o, use_depth=False), session.ransac_params(o, use_depth=True, max_tries=5)
    assert rgb["unit"] == "px" and rgbd["unit"] == "cm"
    assert rgbd["thr"] == 7.5 and rgbd["max_reproj"] == 60.0 and rgbd["hyps"] == 48 and rgbd["max_tries"] == 5
    assert {k: v for k, v in rgb.items() if k != "unit"} == {**{k: v for k, v in rgbd.items() if k != "unit"}, "max_tries": 16}
    d = session.ransac_params(session.default_options(rgbd=True), use_depth=True)
    assert d["thr"] == 10.0 and d["max_reproj"] == 100.0                          # 10 cm, distance errors clamped at 100 cm


class _RegisterOnly(session.ReconstructionSession):
    """register() of the product on a host-only skeleton: the head and both estimators are replaced by recorders."""

    def __init__(self, opt, n=5, oh=6, ow=8):
        self.opt, self.n, self.world, self.rank, self.group = opt, n, 1, 0, None
        self.dev = torch.device("cpu")
        self.classes = [SimpleNamespace(ids=np.arange(n), oh=oh, ow=ow, hw=oh * ow, ppx=ow * 4.0, ppy=oh * 4.0)]
        self.frame_class, self.frel = np.zeros(n, np.int64), np.ones(n)
        self.depth = torch.full((n, oh, ow), 2.0)
        self.timings = {"register_s": 0.0}

    def scene_coordinates(self, head_sd, frame_ids=None):
        return torch.zeros(len(frame_ids), 3, self.classes[0].oh, self.classes[0].ow)


def test_centimetre_thresholds_reach_the_rgbd_kernel_parameters(monkeypatch):
    seen = {}

    def fake_cc(depth, focal, ppx, ppy, stride=8):
        seen["cc"] = (tuple(depth.shape), [float(f) for f in focal], ppx, ppy)
        return torch.zeros(depth.shape[0], 3, *depth.shape[1:])

    def fake_rgbd(sc, cc, params, seed, frame_ids=None, want_masks=True):
        seen["rgbd"] = (dsacstar._as_params(params, dsacstar._RGBD_DEFAULTS), seed, list(frame_ids))
        return torch.eye(4).repeat(len(sc), 1, 1), torch.full((len(sc),), 777, dtype=torch.int32), None

    def fake_rgb(sc, intrinsics, params, seed, frame_ids=None, want_masks=True):
        seen["rgb"] = (dsacstar._as_params(params), seed, list(frame_ids))
        return torch.eye(4).repeat(len(sc), 1, 1), torch.full((len(sc),), 333, dtype=torch.int32), None
    monkeypatch.setattr(dsacstar, "camera_coordinates_device", fake_cc)
    monkeypatch.setattr(dsacstar, "register_batch_rgbd", fake_rgbd)
    monkeypatch.setattr(dsacstar, "register_batch", fake_rgb)
    ses = _RegisterOnly(session.default_options(rgbd=True, ransac_threshold=12.0, maxpixelerror=80.0, ransac_iterations=40))
    _, inl = ses.register({}, 500.0, use_depth=True)
    prm, seed, keys = seen["rgbd"]
    assert (prm.inlier_threshold, prm.max_reproj, prm.hypotheses, prm.max_tries) == (12.0, 80.0, 40, 16)   # 12 cm, 80 cm
    assert prm.inlier_alpha == 100.0 and seed == ses.opt.register_seed
    assert keys == [0, 1, 2, 3, 4]                                                # the RNG keys are the frame positions, as in the RGB loop
    assert seen["cc"] == ((5, 6, 8), [500.0] * 5, 32.0, 24.0) and list(inl) == [777] * 5 and "rgb" not in seen
    ses.register({}, 500.0)                                                       # the RGB call of the same session: same numbers, pixels
    prm, _, keys = seen["rgb"]
    assert (prm.inlier_threshold, prm.max_reproj, prm.subsampling) == (12.0, 80.0, 8) and keys == [0, 1, 2, 3, 4]


# ------------------------------------------------------------------------------------------------------------------------
# the loop: tests/test_session_cpu.py's scripted scenarios (the reference's own decisions, tests/golden/ace_zero_loop.json) with rgbd=True
class _ScriptedSession(session.ReconstructionSession):
    """map / register replaced by scripted outcomes that record with_depth / use_depth; everything else is the product's reconstruct()."""

    def __init__(self, opt, rates, n=200):
        self.opt, self.n, self.H, self.W = opt, n, 480, 640
        self.depth = torch.zeros(1)
        f_ext = float(opt.use_external_focal_length)
        self.focal0 = f_ext if f_ext > 0 else -1.0
        self.history, self.calls, self._rates, self._maps = [], [], list(rates), 0
        self.rank, self.world, self.group = 0, 1, None

    def map(self, image_ids, poses_c2w, focal, *, iterations, loss_type, schedule, lr_max, refinement="none", pose_wait=0,
            refine_calibration=False, load_weights=None, with_depth=False, tag="map", data_parallel=None):
        seed = tag.startswith("iteration0_seed")                        # (in RGB mode with_depth itself marks the seed trials)
        if not seed:
            self._maps += 1
        self.calls.append({"cmd": "train", "id": tag, "seed": seed, "iterations": iterations, "loss": loss_type, "schedule": schedule,
                           "lr_max": lr_max, "pose_wait": pose_wait, "refinement": refinement, "refine_calibration": bool(refine_calibration),
                           "load_weights": None if load_weights is None else load_weights["id"], "images": len(list(image_ids)),
                           "with_depth": with_depth})
        return {"head": {"id": tag}, "poses_w2c": None, "focal": 500.0 + self._maps if not seed else focal, "iterations": iterations,
                "seconds": 0.0}

    def register(self, head_sd, focal, max_estimates=-1, tag="register", max_tries=16, use_depth=False):
        rate = self._rates.pop(0)
        conf = np.zeros(self.n, np.int32)
        conf[:round(rate * self.n)] = 1000
        self.calls.append({"cmd": "register", "network": head_sd["id"], "session": tag, "focal": focal, "max_estimates": max_estimates,
                           "use_depth": use_depth})
        return np.tile(np.eye(4, dtype=np.float32), (self.n, 1, 1)), conf


def _reference_decisions(calls):
    out = []
    for c in calls:
        f = c["flags"]
        if c["cmd"] == "train":
            out.append({"cmd": "train", "id": c["id"], "seed": "use_pose_seed" in f, "iterations": int(f.get("iterations", 25000)),
                        "loss": f["repro_loss_type"], "schedule": f["learning_rate_schedule"], "lr_max": float(f["learning_rate_max"]),
                        "pose_wait": int(f["pose_refinement_wait"]), "refinement": f.get("pose_refinement", "none"),
                        "refine_calibration": f.get("refine_calibration", "False") == "True",
                        "load_weights": os.path.splitext(os.path.basename(f["load_weights"]))[0] if "load_weights" in f else None})
        else:
            out.append({"cmd": "register", "network": c["network"], "session": f["session"], "focal": float(f["use_external_focal_length"]),
                        "max_estimates": int(f.get("max_estimates", -1))})
    return out


def _scenario(golden_dir, name, rgbd):
    g = json.load(open(os.path.join(golden_dir, "ace_zero_loop.json")))[name]
    argv = g["argv"]
    over = {argv[i].lstrip("-"): argv[i + 1] for i in range(0, len(argv), 2)}
    conv = {"final_refine": lambda v: v == "True", "final_refit": lambda v: v == "True", "warmstart": lambda v: v == "True",
            "refine_calibration": lambda v: v == "True", "iterations_max": int, "refinement": str,
            "seed_network": lambda v: {"id": "seed_network"}}
    opt = session.default_options(try_seeds=2, rgbd=rgbd, **{k: conv[k](v) for k, v in over.items()})
    ses = _ScriptedSession(opt, g["rates"])
    return g, ses, ses.reconstruct()


SCENARIOS = ["reaches_threshold", "relative_threshold", "no_final_refine", "no_final_refit", "iterations_max", "no_warmstart",
             "naive_refinement_no_calibration", "slow_growth", "seed_network"]


@pytest.mark.parametrize("name", SCENARIOS)
def test_rgbd_loop_uses_depth_in_every_round_and_makes_the_reference_decisions(golden_dir, name):
    g, ses, res = _scenario(golden_dir, name, rgbd=True)
    trains, regs = [c for c in ses.calls if c["cmd"] == "train"], [c for c in ses.calls if c["cmd"] == "register"]
    assert trains and regs
    assert all(c["with_depth"] is True for c in trains), [c["id"] for c in trains if not c["with_depth"]]
    assert all(c["use_depth"] is True for c in regs), [c["session"] for c in regs if not c["use_depth"]]
    # warm-started rounds, the final refine and the final refit are among them
    rounds = [c for c in trains if not c["seed"]]
    if name == "slow_growth":
        assert sum(c["load_weights"] is not None for c in rounds) >= 2                         # warm-started rounds, with depth
        assert rounds[-1]["loss"] == "dyntanh" and rounds[-1]["load_weights"] is None          # the final refit: a fresh network, with depth
    # the decisions (which rounds, which settings, warm start, focal hand-over, seed scoring subset) are the RGB loop's = the reference's
    ref = _reference_decisions(g["calls"])
    mine = [{k: v for k, v in c.items() if k not in ("images", "with_depth", "use_depth")} for c in ses.calls]
    assert len(mine) == len(ref)
    for a, b in zip(mine, ref):
        assert a == b, (a, b)
    assert len(g["rates"]) - len(ses._rates) == g["registers_used"]
    first = 0 if name == "seed_network" else 2
    assert [c["images"] for c in rounds] == [round(r * 200) for r in g["rates"][first:first + len(rounds)]]
    assert res["iterations"] == len(rounds)


@pytest.mark.parametrize("name", ["reaches_threshold", "seed_network"])
def test_rgb_loop_passes_no_depth_beyond_the_seeds(golden_dir, name):
    """rgbd off: only the seed trials are depth-supervised and no registration sees depth (what the loop did before the mode existed)."""
    _, ses, _ = _scenario(golden_dir, name, rgbd=False)
    assert all(c["with_depth"] == c["seed"] for c in ses.calls if c["cmd"] == "train")
    assert not any(c["use_depth"] for c in ses.calls if c["cmd"] == "register")


def test_rgbd_loop_is_refused_on_several_ranks():
    ses = _ScriptedSession(session.default_options(rgbd=True, try_seeds=1), [1.0, 1.0])
    ses.world = 2
    with pytest.raises(RuntimeError, match="--rgbd True runs on one GPU"):
        ses.reconstruct()
    assert ses.calls == []
