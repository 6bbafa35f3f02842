"""GPU: bench.py --dump-outputs writes what the last timed headline step computed (float32 / float64 .npy, 64 MB at most), --steps is the
number of timed steps, and two runs with the same arguments start from the same seeded inputs, so they write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, steps, warmup, mode=("--headline-only",)):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *mode, "--steps", str(steps), "--warmup", str(warmup),
           "--buffer-patches", "262144", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {name[:-4]: np.load(os.path.join(d, name)) for name in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_dump_outputs_hold_the_last_timed_step_and_repeat(tmp_path):
    steps, warmup = 3, 2
    line = _run(tmp_path / "a", steps, warmup)
    assert line["steps"] == steps and line["ms_per_step"] > 0 and len(line["window_ms_per_step"]) == 1
    assert abs(line["ms_per_step"] - line["window_ms_per_step"][0]) < 1e-9
    a = _load(tmp_path / "a")
    assert sorted(a) == ["adam_m", "adam_v", "head_params", "scene_coords", "step_state"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["head_params"].shape == a["adam_m"].shape == a["adam_v"].shape == (2_103_300,)
    assert a["scene_coords"].shape == (5120, 3) and np.isfinite(a["scene_coords"]).all()
    assert a["step_state"][0] == warmup + steps and np.isfinite(a["step_state"]).all()   # the iteration the dump was taken at
    assert (a["adam_v"] > 0).any()                                                           # the optimiser has run
    _run(tmp_path / "b", steps, warmup)
    b = _load(tmp_path / "b")
    assert sorted(b) == sorted(a)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
def test_plain_run_dumps_what_the_headline_leg_dumps(tmp_path):
    """Without --full or --headline-only the run times the same steps on the same inputs: the same arrays, and a line of the headline
    fields alone."""
    line = _run(tmp_path / "plain", 3, 2, mode=())
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert not {"summary", "roofline", "registration", "per_class_us_per_step", "device_state", "cpu_baseline"} & set(line)
    _run(tmp_path / "headline", 3, 2)
    a, b = _load(tmp_path / "plain"), _load(tmp_path / "headline")
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
