"""GPU: the ICP kernels of acezero_amd/csrc/geometry_api.hip (acez_geom_icp_accumulate, acez_geom_icp_update) against the numpy
restatement of include/acez.h section N (tests/icp_restated.py, itself checked in tests/test_icp_cpu.py): the sums bit for bit, the
correspondences those of nearest_distances, the trajectory step by step from the kernel's own transforms, the recovery of a known
displacement, the stopping rules, determinism, and eval_geometry.py --icp end to end."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import geometry_cases as GC
from tests import geometry_restated as R
from tests import icp_restated as I

pytestmark = pytest.mark.gpu
F = np.float32
RADIUS = 0.1
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def state_of(T):
    s = np.zeros(34)
    s[:12] = np.asarray(T, np.float64)[:3].reshape(-1)
    return s


def device_accumulate(src, tgt, radius, T, status=0.0):
    """acez_geom_icp_accumulate itself on the sources in the order given: (partials [blocks,18], pivot float32 [3])."""
    from acezero_amd import _native as N
    from acezero_amd import geometry as G
    from acezero_amd.head import _ptr
    g = G.build_grid(torch.from_numpy(tgt).cuda(), radius)
    pivot = (g.origin + g.hi) * F(0.5)
    s = state_of(T)
    s[12] = status
    state = torch.from_numpy(s).cuda()
    src_d = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    partials = torch.full(((len(src) + 255) // 256, 18), -7.0, dtype=torch.float64, device="cuda")
    N.check(N.lib().acez_geom_icp_accumulate(_ptr(g.ref_sorted), _ptr(g.ref_index), _ptr(g.cell_start), g.ref_sorted.shape[0],
                                             *[float(v) for v in g.origin], float(g.cell), *g.dims, _ptr(src_d), len(src), radius,
                                             *[float(v) for v in pivot], _ptr(state), _ptr(partials), None))
    torch.cuda.synchronize()
    return partials.cpu().numpy(), pivot


def device_update(partials, n, pivot, state, with_scale=False, max_iterations=4, rel=1e-6):
    """acez_geom_icp_update itself: (state [34], history [max_iterations,16])."""
    from acezero_amd import _native as N
    from acezero_amd.head import _ptr
    state_d, partials_d = torch.from_numpy(state.copy()).cuda(), torch.from_numpy(np.ascontiguousarray(partials)).cuda()
    history = torch.full((max_iterations, 16), -7.0, dtype=torch.float64, device="cuda")
    N.check(N.lib().acez_geom_icp_update(_ptr(partials_d), n, *[float(v) for v in pivot], int(with_scale), rel, rel, max_iterations,
                                         _ptr(state_d), _ptr(history), None))
    torch.cuda.synchronize()
    return state_d.cpu().numpy(), history.cpu().numpy()


@functools.lru_cache(maxsize=None)
def sums_case():
    """(sources [1000,3], target [502,3], T): a similarity with scale; sources that land near the target, four that land 5 m away, two
    that are not finite, and source 0 with two targets at exactly the same d2 (rows 500 and 501)."""
    T = GC.similarity(scale=1.3, angle=0.4, t=(0.2, -0.1, 0.3))
    rng = np.random.default_rng(21)
    tgt = I.scene(500, 11)
    near = (I.scene(1000, 12) + rng.normal(scale=0.03, size=(1000, 3))).astype(F)
    near[0] = [1.5, 1.0, 1.25]                                   # in the open: the tied pair below is its nearest
    src = R.apply_similarity(near, np.linalg.inv(T))
    src[[40, 41, 300, 999]] += F(5)
    src[5, 1], src[17, 2], src[600, 0] = np.nan, np.inf, -np.inf
    x0 = R.apply_similarity(src[:1], T)[0]
    step = np.array([2.0 ** -6, 0, 0], F)
    tgt = np.concatenate([tgt, [x0 + step, x0 - step]]).astype(F)
    return src, tgt, T


@functools.lru_cache(maxsize=None)
def sums_reference(n, order):
    src, tgt, T = sums_case()
    src = src[:n]
    if order == "shuffled":
        src = src[np.random.default_rng(4).permutation(n)]
    elif order == "by_cell":
        src = src[I.source_order(src, tgt, RADIUS)]
    partials, d2, idx = I.accumulate(src, tgt, RADIUS, T, I.pivot_of(tgt, RADIUS))
    return src, partials, d2, idx


@functools.lru_cache(maxsize=None)
def dense_case():
    """(sources [600,3], target [3002,3], T): everything inside a box of 4 x 2 x 1 cells, so that every workgroup's box of cells is
    compact and ACCUMULATE takes the LDS-staged form; some 1500 targets per row of cells, so that a staged row takes two chunks."""
    T = GC.similarity(scale=1.3, angle=0.4, t=(0.2, -0.1, 0.3))
    rng = np.random.default_rng(31)
    box = np.array([0.35, 0.15, 0.08])
    tgt = np.concatenate([np.zeros((1, 3)), box[None], rng.uniform(0, 1, (3000, 3)) * box]).astype(F)
    near = (0.01 + rng.uniform(0, 1, (600, 3)) * (box - 0.02)).astype(F)
    src = R.apply_similarity(near, np.linalg.inv(T))
    src[7, 0], src[300, 2] = np.nan, np.inf
    return src, tgt, T


@functools.lru_cache(maxsize=None)
def dense_reference(order):
    src, tgt, T = dense_case()
    if order == "shuffled":
        src = src[np.random.default_rng(5).permutation(len(src))]
    partials, d2, idx = I.accumulate(src, tgt, RADIUS, T, I.pivot_of(tgt, RADIUS))
    return src, partials, d2, idx


def compact_workgroups(x, tgt, radius):
    """The kernel's rule restated: per workgroup of 256 transformed sources x (float32), whether it takes the staged form. The box of
    the live sources' cells (clamped to -1 .. n per axis) must span at most 12 rows of cells with their neighbours, (jspan + 3) *
    (kspan + 3), and at most 4 cells along x."""
    lo, _, c, dims = I.grid_of(tgt, radius)
    out = []
    for at in range(0, len(x), 256):
        p = x[at:at + 256]
        p = p[np.isfinite(p).all(1)]
        if not len(p):
            out.append(False)
            continue
        with np.errstate(all="ignore"):
            f = np.floor((p - lo) / c)
        assert f.dtype == F
        cell = np.clip(f, -1, np.array(dims, F)).astype(np.int64)
        span = cell.max(0) - cell.min(0)
        out.append(bool((span[1] + 3) * (span[2] + 3) <= 12 and span[0] + 1 <= 4))
    return out


def test_what_the_dense_case_is_for():
    src, tgt, T = dense_case()
    lo, _, c, dims = I.grid_of(tgt, RADIUS)
    assert dims == [4, 2, 1]
    rows = np.floor((tgt[:, 1] - lo[1]) / c).astype(int)
    assert (np.bincount(rows) > 1024).all(), "a staged row of cells holds more than one chunk of 1024 targets"
    for order in ("given", "shuffled"):
        ordered, partials, d2, idx = dense_reference(order)
        assert compact_workgroups(R.apply_similarity(ordered, T), tgt, RADIUS) == [True, True, True], "every workgroup takes the staged form"
        assert (idx >= 0).sum() == 598 and partials.shape == (3, 18) and (partials[:, 0] > 80).all()
    # the sparse case above is the other side: its full workgroups span too many cells, only a single live source is compact
    ordered, _, _, _ = sums_reference(1000, "by_cell")
    assert compact_workgroups(R.apply_similarity(ordered, sums_case()[2]), sums_case()[1], RADIUS) == [False] * 4
    assert compact_workgroups(R.apply_similarity(sums_case()[0][:1], sums_case()[2]), sums_case()[1], RADIUS) == [True]


@pytest.mark.parametrize("order", ["given", "shuffled"])
def test_accumulate_staged_form_bit_for_bit(order):
    """Full workgroups in the LDS-staged form, two chunks per staged row, in the product build."""
    _, tgt, T = dense_case()
    ordered, want, _, _ = dense_reference(order)
    got, pivot = device_accumulate(ordered, tgt, RADIUS, T)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]
    state, history = device_update(got, len(ordered), pivot, state_of(T), with_scale=True)
    assert np.array_equal(bits(state[16:]), bits(I.totals(want))) and history[0, 12] == 598


def test_what_the_sums_case_is_for():
    src, tgt, T = sums_case()
    _, partials, d2, idx = sums_reference(1000, "given")
    assert idx[0] == 500 and d2[0] == F(2.0 ** -12), "the tie: rows 500 and 501 at the same d2, the lower row wins"
    assert R.nearest(R.apply_similarity(src[:1], T), tgt[::-1], RADIUS)[1][0] == 0, "reversed, the other one of the pair wins"
    assert (idx[[5, 17, 600, 40, 41, 300, 999]] == -1).all() and 400 < (idx >= 0).sum() < 800, "many with and many without a correspondence"
    assert partials.shape == (4, 18) and np.isfinite(partials).all() and partials[:, 0].sum() == (idx >= 0).sum()


@pytest.mark.parametrize("n", COUNTS)
def test_accumulate_sums_bit_for_bit(n):
    src, tgt, T = sums_case()
    for order in ("given",) + (("by_cell", "shuffled") if n == 1000 else ()):
        ordered, want, _, _ = sums_reference(n, order)
        got, pivot = device_accumulate(ordered, tgt, RADIUS, T)
        assert np.array_equal(pivot, I.pivot_of(tgt, RADIUS))
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (n, order, np.argwhere(bits(got) != bits(want))[:5])
        state, history = device_update(got, n, pivot, state_of(T), with_scale=True)
        total = I.totals(want)
        assert np.array_equal(bits(state[16:]), bits(total)), (n, order)
        assert state[13] == 1 and history[0, 12] == total[0] and bits(history[0, 13]) == bits(total[17])
        assert np.array_equal(bits(history[0, :12]), bits(state_of(T)[:12])) and (history[1:] == -7).all()


def test_accumulate_both_kernel_forms_give_the_same_bits(diag_lib, monkeypatch):
    """The dense case takes the staged form in every workgroup (test_what_the_dense_case_is_for), the sparse case the per-lane form in
    every full one; ACEZ_GEOM_PLAIN sends both down the per-lane form. All give the restatement's bits."""
    monkeypatch.delenv("ACEZ_GEOM_PLAIN", raising=False)
    cases = [("dense " + order, dense_case(), dense_reference(order)) for order in ("given", "shuffled")]
    cases += [("sparse " + order, sums_case(), sums_reference(1000, order)) for order in ("by_cell", "shuffled")]
    for name, (_, tgt, T), (ordered, want, _, _) in cases:
        assert np.array_equal(bits(device_accumulate(ordered, tgt, RADIUS, T)[0]), bits(want)), f"{name}, diagnostics build"
        with monkeypatch.context() as m:
            m.setenv("ACEZ_GEOM_PLAIN", "1")
            assert np.array_equal(bits(device_accumulate(ordered, tgt, RADIUS, T)[0]), bits(want)), f"{name}, per-lane form"


def test_update_sums_more_rows_than_threads():
    """700 partial rows: thread t adds rows t, t + 256, t + 512 in that order."""
    rng = np.random.default_rng(8)
    partials = rng.normal(size=(700, 18)) * 10.0 ** rng.integers(-3, 4, (700, 1))
    partials[:, 0] = rng.integers(0, 257, 700)
    partials[:, 17] = np.abs(partials[:, 17])
    n = 700 * 256 - 100
    state, history = device_update(partials, n, np.zeros(3, F), state_of(np.eye(4)))
    want = I.totals(partials)
    assert np.array_equal(bits(state[16:]), bits(want))
    assert history[0, 12] == want[0] and history[0, 14] == want[0] / n and history[0, 15] == np.sqrt(want[17] / want[0])


def test_same_correspondences_as_the_search():
    from acezero_amd.geometry import apply_similarity, nearest_distances
    src, tgt, T = sums_case()
    d2, idx = nearest_distances(apply_similarity(torch.from_numpy(src).cuda(), T), torch.from_numpy(tgt).cuda(), RADIUS)
    d2, found = d2.cpu().numpy(), idx.cpu().numpy() >= 0
    t = np.zeros((len(src), 18))
    t[:, 0], t[:, 17] = found, np.where(found, d2.astype(np.float64), 0.0)
    want = I.totals(I.block_sums(t))
    got, pivot = device_accumulate(src, tgt, RADIUS, T)
    state, _ = device_update(got, len(src), pivot, state_of(T))
    assert state[16] == want[0] == found.sum() and bits(state[33]) == bits(want[17])
    assert np.array_equal(bits(got[:, [0, 17]]), bits(I.block_sums(t)[:, [0, 17]]))


def test_a_stopped_loop_launches_nothing():
    src, tgt, T = sums_case()
    for status in (1.0, 2.0):
        got, pivot = device_accumulate(src, tgt, RADIUS, T, status=status)
        assert (got == -7).all(), "ACCUMULATE returns at once"
        s = state_of(T)
        s[12] = status
        state, history = device_update(np.ones((4, 18)), len(src), pivot, s)
        assert np.array_equal(bits(state), bits(s)) and (history == -7).all(), "UPDATE returns at once"
    s = state_of(T)
    s[13] = 4.0                                                  # all of max_iterations = 4 records written
    state, history = device_update(np.ones((4, 18)), len(src), pivot, s)
    assert np.array_equal(bits(state), bits(s)) and (history == -7).all()


# ---------------------------------------------------------------------------------------------------------------- the loop
def stage(src, tgt, radius, **kw):
    from acezero_amd.geometry import icp_stage
    return icp_stage(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), radius, **kw)


@functools.lru_cache(maxsize=None)
def noisy_run():
    src, tgt, radius = I.noisy_case()
    return stage(src, tgt, radius)


def test_trajectory_teacher_forced():
    """Every recorded iteration on its own: from the kernel's T_k the restatement finds the same correspondences (count and sum of d2
    exactly) and the next transform within the SVD's bound. Forcing each step from the kernel's transform keeps a one-ulp difference
    in the solve from flipping a correspondence and compounding."""
    from acezero_amd import geometry as G
    src, tgt, radius = I.noisy_case()
    T, info = noisy_run()
    order = I.source_order(src, tgt, radius)
    g = G.build_grid(torch.from_numpy(tgt).cuda(), radius)
    assert np.array_equal(G.order_by_cell(torch.from_numpy(src).cuda(), g).cpu().numpy(), order)
    pivot = I.pivot_of(tgt, radius)
    ordered = src[order]
    done = info["iterations"]
    print(f"{done} iterations, {info['status']}, fitness {info['fitness'][-1]}, rmse {info['rmse'][-1]}")
    assert 3 <= done <= 30 and info["status"] == "converged" and 0.7 < info["fitness"][-1] < 0.85
    assert np.array_equal(info["transforms"][0], np.eye(4))
    for k in range(done):
        T_k = info["transforms"][k]
        total = I.totals(I.accumulate(ordered, tgt, radius, T_k, pivot)[0])
        assert info["count"][k] == total[0] and bits(info["sum_d2"][k]) == bits(total[17]), k
        assert info["fitness"][k] == total[0] / len(src) and info["rmse"][k] == np.sqrt(total[17] / total[0])
        T_next = info["transforms"][k + 1] if k + 1 < done else T
        if k == done - 1:                                        # the converged record: no step
            assert np.array_equal(bits(T_next), bits(T_k))
        else:
            want = I.solve(total, pivot, False, T_k)
            np.testing.assert_allclose(T_next, want, rtol=1e-9, atol=1e-9 * np.abs(want).max(), err_msg=f"step {k}")


@pytest.mark.parametrize("with_scale", [False, True], ids=["rigid", "with_scale"])
def test_recovery(with_scale):
    from acezero_amd.geometry import refine_alignment
    src, tgt, S = I.recovery_case(with_scale)
    T, infos = refine_alignment(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), None, distances=I.STAGES, with_scale=with_scale)
    worst = np.linalg.norm(R.apply_similarity(src, T).astype(np.float64) - tgt[::2], axis=1).max()
    print([(i["iterations"], i["status"], i["fitness"][-1], i["rmse"][-1]) for i in infos], np.abs(T - S).max(), worst)
    for info, d in zip(infos, I.STAGES):
        assert info["status"] == "converged" and info["fitness"][-1] == 1.0 and info["count"][-1] == len(src)
        assert info["distance"] == d and info["voxel"] is None and info["kept_previous"] is False
    assert np.abs(T - S).max() <= I.T_BOUND
    assert worst <= I.POINT_BOUND
    # from an initial alignment, with a voxel size per stage: the downsampled clouds are different samples of the surface, so the
    # alignment is found to the voxel's scale only
    T0 = np.eye(4)
    T0[:3, 3] = [0.01, 0.0, 0.01]
    T_v, infos_v = refine_alignment(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), T0, distances=[0.2, 0.1], voxels=[0.05, None],
                                    with_scale=with_scale)
    assert infos_v[0]["voxel"] == 0.05 and infos_v[0]["count"][-1] < len(src) and infos_v[1]["count"][-1] == len(src)
    assert np.abs(T_v - S).max() <= I.T_BOUND


def test_stopping():
    src, tgt, _ = I.recovery_case(False)
    T30, info30 = stage(src, tgt, 0.2, max_iterations=30)
    T60, info60 = stage(src, tgt, 0.2, max_iterations=60)
    assert info30["status"] == info60["status"] == "converged" and info30["iterations"] == info60["iterations"] < 30
    assert np.array_equal(bits(T30), bits(T60))
    for key in ("fitness", "rmse", "count", "sum_d2"):
        assert info30[key] == info60[key] and len(info30[key]) == info30["iterations"]
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(info30["transforms"], info60["transforms"]))
    # after the last record the history is untouched: the idle launches wrote nothing
    T, info = stage(src + F(10), tgt, 0.2)
    assert info["status"] == "degenerate" and info["iterations"] == 1 and info["count"] == [0] and np.array_equal(T, np.eye(4))
    T2, info2 = stage(src, tgt, 0.2, max_iterations=2)
    assert info2["status"] == "max_iterations" and info2["iterations"] == 2
    assert np.array_equal(bits(info2["transforms"][1]), bits(info30["transforms"][1]))
    from acezero_amd.geometry import refine_alignment
    T0 = GC.similarity(scale=1.0, angle=0.1, t=(10.0, 0.0, 0.0))
    T_kept, infos = refine_alignment(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), T0, distances=[0.2])
    assert infos[0]["kept_previous"] is True and np.array_equal(T_kept, T0), "a degenerate stage keeps the alignment it started with"


def test_determinism():
    src, tgt, radius = I.noisy_case()
    T_a, a = noisy_run()
    T_b, b = stage(src, tgt, radius)
    assert np.array_equal(bits(T_a), bits(T_b)) and a["iterations"] == b["iterations"] and a["status"] == b["status"]
    for key in ("fitness", "rmse", "count", "sum_d2"):
        assert np.array_equal(bits(a[key]), bits(b[key]))
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a["transforms"], b["transforms"]))


# ------------------------------------------------------------------------------------------------------------ command line
TODAYS_KEYS = {"rec_points_read", "gt_points_read", "max_distance", "voxel", "rec_points", "gt_points", "dropped", "thresholds", "rec_within",
               "gt_within", "precision", "recall", "fscore", "accuracy_mean", "accuracy_median", "completeness_mean",
               "completeness_median", "transform"}


def test_command_line(tmp_path, caplog):
    import logging
    from acezero_amd import cli
    from acezero_amd.formats import write_ply
    src, tgt, S = I.recovery_case(False)
    rec, gt = tmp_path / "rec.ply", tmp_path / "gt.ply"
    write_ply(rec, src, np.zeros((len(src), 3), np.uint8))
    write_ply(gt, tgt, np.zeros((len(tgt), 3), np.uint8))

    def run(name, *flags):
        out = tmp_path / name
        assert cli.eval_geometry_main([str(rec), str(gt), "--thresholds", "0.0001", "--crop", "False", "--output_json", str(out)] + list(flags)) == 0
        return json.loads(out.read_text())

    plain = run("plain.json")
    assert plain["precision"][0] < 0.05 and set(plain) == TODAYS_KEYS and plain["transform"] is None
    run("off.json", "--icp", "False")
    assert (tmp_path / "off.json").read_bytes() == (tmp_path / "plain.json").read_bytes()
    with caplog.at_level(logging.INFO, logger="eval_geometry"):
        res = run("icp.json", "--icp", "True", "--icp_distances", "0.2", "0.1", "0.05")
    assert res["precision"][0] == 1.0 and res["rec_within"][0] == len(src)
    assert np.abs(np.array(res["transform"]) - S).max() <= I.T_BOUND and res["transform_initial"] is None
    assert set(res) == TODAYS_KEYS | {"transform_initial", "icp"}
    assert [s["distance"] for s in res["icp"]] == [0.2, 0.1, 0.05] and all(s["status"] == "converged" for s in res["icp"])
    assert all("transforms" not in s and len(s["fitness"]) == s["iterations"] for s in res["icp"])
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("ICP stage")]
    assert len(lines) == 3 and "ICP stage at 0.2 m" in lines[0] and "converged, fitness 100.00%" in lines[0], lines
    # a stage that finds nothing has no rmse: null in the file, which stays strict JSON
    far = np.eye(4)
    far[0, 3] = 10.0
    np.savetxt(tmp_path / "far.txt", far)
    out = tmp_path / "far.json"
    assert cli.eval_geometry_main([str(rec), str(gt), "--thresholds", "0.05", "--crop", "False", "--icp", "True", "--icp_distances", "0.2",
                                   "--transform", str(tmp_path / "far.txt"), "--output_json", str(out)]) == 0

    def not_json(token):
        raise AssertionError(f"{token} in the JSON file")

    res = json.loads(out.read_text(), parse_constant=not_json)
    assert res["icp"][0]["status"] == "degenerate" and res["icp"][0]["rmse"] == [None] and res["icp"][0]["count"] == [0]
    assert np.array_equal(np.array(res["transform"]), far) and res["precision"][0] == 0.0
    # from a --transform, with the default distances (4, 2, 1 times the search radius) and a scale
    T0 = np.eye(4)
    T0[:3, 3] = [0.01, -0.01, 0.01]
    np.savetxt(tmp_path / "T0.txt", T0)
    res = run("from.json", "--icp", "True", "--transform", str(tmp_path / "T0.txt"), "--max_distance", "0.05", "--icp_scale", "True")
    assert [s["distance"] for s in res["icp"]] == [0.2, 0.1, 0.05] and np.array_equal(np.array(res["transform_initial"]), T0)
    assert res["precision"][0] == 1.0 and np.abs(np.array(res["transform"]) - S).max() <= I.T_BOUND
