"""GPU: the cloud-distance kernels of acezero_amd/csrc/geometry_api.hip against the numpy restatement of their definition
(tests/geometry_restated.py, itself checked in tests/test_geometry_cpu.py), bit for bit; the entry points' argument checks with device
buffers; evaluate_geometry against the restated metric; eval_geometry.py end to end on the fused box room."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import fusion_cases as FC
from tests import geometry_cases as GC
from tests import geometry_restated as R
from tests.test_fusion_cpu import DISTANCE_BOUND

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CASES = GC.search_cases()


@functools.lru_cache(maxsize=None)
def reference(name):
    q, p, r, _ = CASES[name]
    return R.nearest(q, p, r)


def search(q, p, r, cell=None):
    from acezero_amd.geometry import nearest_distances
    d2, idx = nearest_distances(torch.from_numpy(q).cuda(), torch.from_numpy(p).cuda(), r, cell=cell)
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.shape == idx.shape == (len(q),)
    return d2.cpu().numpy(), idx.cpu().numpy()


def assert_same(got, want, what):
    bad = (got[0].view(np.uint32) != want[0].view(np.uint32)) | (got[1] != want[1])
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} queries differ, first {int(np.argmax(bad))}: " \
                          f"got {got[0][np.argmax(bad)]!r} / {got[1][np.argmax(bad)]}, want {want[0][np.argmax(bad)]!r} / {want[1][np.argmax(bad)]}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_nearest_matches_the_restatement(name):
    q, p, r, cell = CASES[name]
    want = reference(name)
    assert_same(search(q, p, r, cell), want, name)
    if cell is None and len(p) and len(q):                       # the result does not depend on the grid
        c = float(F(r) * GC.MARGIN)
        for factor in (1.0, 1.5, 7.0):
            assert_same(search(q, p, r, cell=c * factor), want, f"{name}, cell x {factor}")


def test_what_the_cases_are_for():
    d2, idx = reference("one_and_one_found")
    assert idx.tolist() == [0] and d2[0] > 0
    assert reference("one_and_one_too_far")[1].tolist() == [-1]
    d2, idx = reference("exactly_the_radius")
    assert idx.tolist() == [0, -1, 0, -1] and d2[0] == F(0.75) * F(0.75)
    d2, idx = reference("outside_the_box")
    q = CASES["outside_the_box"][0]
    assert ((q < 0) | (q > 1)).any(1).all() and 50 < (idx >= 0).sum() < len(q) - 150, "outside queries with and without a reference in reach"
    d2, idx = reference("ties")
    q, p, r, _ = CASES["ties"]
    assert (idx >= 0).all()
    both = R.nearest(q, p[::-1], r)                              # a tie shows as two different points at the same d2
    tied = (len(p) - 1 - both[1]) != idx
    assert tied.sum() > 20 and np.array_equal(both[0], d2) and (idx[tied] < len(p) - 1 - both[1][tied]).all()
    assert (reference("one_cell_5000")[1] >= 0).all()
    for name in ("plane_nz_1", "line_ny_nz_1", "dense_cube", "dense_surface", "faces_and_corners", "uniform_257"):
        found = reference(name)[1] >= 0
        assert 0.2 * len(found) < found.sum(), name
    assert not (reference("uniform_257")[1] >= 0).all() or not (reference("dense_surface")[1] >= 0).all()


def test_both_kernel_forms_give_the_same_bits(diag_lib, monkeypatch):
    """The diagnostics build can send every workgroup down the per-lane form (ACEZ_GEOM_PLAIN): the staged and the per-lane form are
    then compared on the same inputs, whichever of them a case's geometry selects in the product build."""
    monkeypatch.delenv("ACEZ_GEOM_PLAIN", raising=False)
    for name in ("dense_cube", "dense_surface", "dense_plane", "one_cell_5000", "plane_nz_1", "uniform_257", "straddling_a_face", "not_finite"):
        q, p, r, cell = CASES[name]
        assert_same(search(q, p, r, cell), reference(name), f"{name}, diagnostics build")
        with monkeypatch.context() as m:
            m.setenv("ACEZ_GEOM_PLAIN", "1")
            assert_same(search(q, p, r, cell), reference(name), f"{name}, per-lane form")


def test_shuffled_references_change_only_the_index():
    q, p, r, _ = CASES["dense_surface"]
    want = reference("dense_surface")
    perm = np.random.default_rng(1).permutation(len(p))
    d2, idx = search(q, p[perm], r)
    assert len(np.unique(p, axis=0)) == len(p)
    assert np.array_equal(d2.view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(np.where(idx >= 0, perm[idx.clip(0)], -1), want[1])


def test_unordered_queries_through_the_entry_point():
    """acez_geom_nearest itself takes queries in any order: here they arrive as they are, not sorted by cell."""
    from acezero_amd import _native as N
    from acezero_amd import geometry as G
    from acezero_amd.head import _ptr
    q, p, r, _ = CASES["dense_cube"]
    lo, c = p.min(0), F(r) * GC.MARGIN
    dims = G.grid_dims(lo, p.max(0), c)
    cells = R.cells(p, lo, c, dims)
    order = np.argsort(cells, kind="stable")
    start = np.r_[0, np.cumsum(np.bincount(cells, minlength=dims[0] * dims[1] * dims[2]))].astype(np.int32)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (p[order], order.astype(np.int32), start, q)]
    d2, idx = torch.empty(len(q), device="cuda"), torch.empty(len(q), dtype=torch.int32, device="cuda")
    assert np.array_equal(G.point_cells(dev[3], lo, c, dims).cpu().numpy(), R.cells(q, lo, c, dims))
    N.check(N.lib().acez_geom_nearest(_ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), len(p), *[float(v) for v in lo], float(c), *dims, _ptr(dev[3]),
                                      len(q), r, _ptr(d2), _ptr(idx), None))
    torch.cuda.synchronize()
    assert_same((d2.cpu().numpy(), idx.cpu().numpy()), reference("dense_cube"), "unsorted queries")
    # a malformed cell table gives wrong numbers, never a read out of bounds: every range is clamped to [0, m]
    broken = torch.from_numpy(np.where(np.arange(len(start)) % 3 == 0, 2 ** 31 - 1, np.where(np.arange(len(start)) % 3 == 1, -5, start)).astype(np.int32)).cuda()
    N.check(N.lib().acez_geom_nearest(_ptr(dev[0]), _ptr(dev[1]), _ptr(broken), len(p), *[float(v) for v in lo], float(c), *dims, _ptr(dev[3]),
                                      len(q), r, _ptr(d2), _ptr(idx), None))
    torch.cuda.synchronize()
    got = idx.cpu().numpy()
    assert got.min() >= -1 and got.max() < len(p)


@pytest.mark.parametrize("name", sorted(GC.downsample_cases()))
def test_voxel_downsample_matches_the_restatement(name):
    from acezero_amd.geometry import voxel_downsample
    pts, voxel = GC.downsample_cases()[name]
    want = R.voxel_downsample(pts, voxel)
    got = voxel_downsample(torch.from_numpy(pts).cuda(), voxel).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_evaluate_geometry_matches_the_restated_metric():
    from acezero_amd.geometry import evaluate_geometry, log_lines
    gt = GC.surface(41, 6000)
    rec = np.concatenate([GC.surface(42, 4000, noise=0.01), np.array([[1.3, 0, 0.5], [np.nan, 0, 0]], F)])
    T = GC.similarity()
    moved = R.apply_similarity(rec, T)
    thresholds = [0.01, 0.02, 0.05]
    keys = ("rec_points", "gt_points", "dropped", "rec_within", "gt_within", "precision", "recall", "fscore", "accuracy_mean",
            "accuracy_median", "completeness_mean", "completeness_median")
    for kw in (dict(), dict(crop=False), dict(max_distance=0.03), dict(voxel=0.05), dict(transform=np.linalg.inv(T))):
        source = moved if "transform" in kw else rec
        got = evaluate_geometry(torch.from_numpy(source).cuda(), torch.from_numpy(gt).cuda(), thresholds, **kw)
        want = R.evaluate(source, gt, thresholds, transform=kw.get("transform"), voxel=kw.get("voxel"), do_crop=kw.get("crop", True),
                          max_distance=kw.get("max_distance"))
        for k in keys:
            assert got[k] == want[k], (kw, k, got[k], want[k])
        assert 0 < got["precision"][0] < got["precision"][2] <= 1 and 0 < got["recall"][0] < 1
        assert len(log_lines(got)) == 2 + len(thresholds)
    assert got["dropped"] >= 1
    with pytest.raises(ValueError, match="empty after cropping"):
        evaluate_geometry(torch.from_numpy(rec + F(10)).cuda(), torch.from_numpy(gt).cuda(), thresholds)


def test_argument_validation_with_device_buffers():
    from acezero_amd import _native as N
    from acezero_amd.head import _ptr
    lib = N.lib()
    pts = torch.from_numpy(GC.uniform(1, 64)).cuda()
    index = torch.arange(64, dtype=torch.int32, device="cuda")
    start = torch.tensor([0, 64], dtype=torch.int32, device="cuda")
    d2 = torch.full((64,), -7.0, device="cuda")
    idx = torch.full((64,), -7, dtype=torch.int32, device="cuda")

    def call(ref=pts, start=start, m=64, c=2.0, dims=(1, 1, 1), n=64, r=0.5, out=d2):
        return lib.acez_geom_nearest(_ptr(ref), _ptr(index), _ptr(start), m, 0.0, 0.0, 0.0, c, *dims, _ptr(pts), n, r, _ptr(out), _ptr(idx), None)

    assert call(c=0.5) == -1 and b"2^-10" in lib.acez_last_error()                       # c = R exactly
    assert call(ref=None) == -1 and call(start=None) == -1 and call(out=None) == -1 and b"null pointer" in lib.acez_last_error()
    assert call(m=-1) == -1 and call(n=2 ** 31) == -1 and b"count" in lib.acez_last_error()
    assert call(dims=(1, 0, 1)) == -1 and call(dims=(1, 1025, 1)) == -1 and b"dimensions" in lib.acez_last_error()
    assert call(dims=(1024, 1024, 17)) == -1 and b"too large" in lib.acez_last_error()
    assert call(r=0.0) == -1 and call(r=float("nan")) == -1 and b"radius" in lib.acez_last_error()
    assert call(c=float("inf")) == -1 and b"cell edge" in lib.acez_last_error()
    assert lib.acez_geom_cells(_ptr(pts), 64, 0.0, 0.0, 0.0, 0.0, 1, 1, 1, _ptr(idx), None) == -1
    assert lib.acez_geom_voxel_means(_ptr(pts), 64, None, 1, _ptr(d2), None) == -1
    with pytest.raises(N.AcezError, match="ACEZ_ERR_INVALID"):
        N.check(call(c=0.5))
    torch.cuda.synchronize()                                     # nothing was launched by the refused calls; the device is fine
    assert (d2 == -7.0).all() and (idx == -7).all()
    assert call() == 0
    torch.cuda.synchronize()
    want = R.nearest(pts.cpu().numpy(), pts.cpu().numpy(), 0.5)
    assert np.array_equal(d2.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[1])


# ------------------------------------------------------------------------------------------------------------ end to end
TAU = 0.02


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    """The box room fused by fuse_depth.py, the ground-truth lattice as a .ply, and eval_geometry.py's scores of the one against the
    other (identity alignment, no crop), run twice."""
    from acezero_amd.formats import write_ply
    tmp = tmp_path_factory.mktemp("room")
    args = FC.write_room_scene(tmp, 12, 120, 160, 100.0)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "fuse_depth.py")] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    gt = GC.room_lattice()
    write_ply(tmp / "gt.ply", gt, np.full((len(gt), 3), 128, np.uint8), alpha=False)
    command = [args[2], str(tmp / "gt.ply"), "--thresholds", "0.01", str(TAU), "--crop", "False", "--output_json"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval_geometry.py")] + command + [str(tmp / "scores_0.json")], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    run_command(command + [str(tmp / "scores_1.json")])           # the second run in this process
    runs = [(tmp / f"scores_{k}.json").read_bytes() for k in range(2)]
    return dict(tmp=tmp, mesh=args[2], pose_file=args[0], gt=gt, runs=runs, log=r.stderr)


def run_command(argv):
    from acezero_amd import cli
    assert cli.eval_geometry_main([str(a) for a in argv]) == 0
    return json.load(open(argv[argv.index("--output_json") + 1]))


def test_eval_geometry_end_to_end(room):
    from acezero_amd.formats import read_ply_points
    res = json.loads(room["runs"][0])
    assert room["runs"][0] == room["runs"][1], "two runs wrote different files"
    vertices = read_ply_points(room["mesh"])
    assert np.array_equal(vertices, FC.read_mesh_ply(room["mesh"])[0]) and np.array_equal(read_ply_points(room["tmp"] / "gt.ply"), room["gt"])
    # every vertex is within DISTANCE_BOUND of a wall plane, so within sqrt(9.75^2 + 2 (2.5 + 9.75)^2) = 19.9 mm of a lattice sample
    assert np.sqrt(DISTANCE_BOUND ** 2 + 2 * (0.0025 + DISTANCE_BOUND) ** 2) < TAU
    assert res["thresholds"] == [0.01, TAU] and res["precision"][1] == 1.0 and res["rec_within"][1] == res["rec_points"] == len(vertices)
    assert res["dropped"] == 0 and res["gt_points"] == len(room["gt"]) and res["recall"][0] > 0
    want = R.evaluate(vertices, room["gt"], [0.01, TAU], do_crop=False, search=R.nearest_d2_tree)
    print(f"{len(vertices)} vertices against {len(room['gt'])} samples: precision {res['precision']}, recall {res['recall']}, "
          f"accuracy {res['accuracy_mean'] * 1000:.3f} mm mean")
    for k in ("rec_points", "gt_points", "rec_within", "gt_within", "precision", "recall", "fscore", "accuracy_median", "completeness_median"):
        assert res[k] == want[k], (k, res[k], want[k])
    for line in ("Threshold 0.02 m: precision 100.00%", f"Reconstruction: {len(vertices)} points", "0 dropped"):
        assert line in room["log"], room["log"][-2000:]


def test_a_shifted_mesh_loses_its_precision(room):
    from acezero_amd.formats import write_ply
    v, c, f = FC.read_mesh_ply(room["mesh"])
    write_ply(room["tmp"] / "shifted.ply", v + np.array([0.03, 0, 0], F), c, f)
    res = run_command([room["tmp"] / "shifted.ply", room["tmp"] / "gt.ply", "--thresholds", "0.01", TAU, "--crop", "False", "--output_json",
                       room["tmp"] / "shifted.json"])
    assert res["precision"][0] < 0.5 < json.loads(room["runs"][0])["precision"][0]
    # the same shift given back as --transform restores the scores, up to the points that the float32 rounding of the round trip moves
    T = np.eye(4)
    T[0, 3] = -0.03
    np.savetxt(room["tmp"] / "back.txt", T)
    back = run_command([room["tmp"] / "shifted.ply", room["tmp"] / "gt.ply", "--thresholds", "0.01", TAU + 1e-4, "--crop", "False",
                        "--transform", room["tmp"] / "back.txt", "--output_json", room["tmp"] / "back.json"])
    assert back["precision"][1] == 1.0


def test_alignment_from_the_pose_pair(room):
    """The mesh and the pose file moved by a known similarity, the original poses as 7-Scenes ground truth: the command finds the
    similarity back from the two sets of poses."""
    from acezero_amd.formats import read_pose_file, write_ply, write_pose_line
    tmp = room["tmp"]
    S = GC.similarity(scale=1.3)
    scale = 1.3
    v, c, f = FC.read_mesh_ply(room["mesh"])
    write_ply(tmp / "moved.ply", R.apply_similarity(v, S), c, f)
    os.makedirs(tmp / "gt_poses", exist_ok=True)
    entries = read_pose_file(room["pose_file"])
    with open(tmp / "moved_poses.txt", "w") as fh:
        for k, e in enumerate(sorted(entries, key=lambda e: e.file)):
            c2w = np.linalg.inv(e.w2c)
            np.savetxt(tmp / "gt_poses" / f"frame_{k:03d}.pose.txt", c2w)
            moved = c2w.copy()                                   # the camera in the moved frame: rotated, its centre moved; poses stay rigid
            moved[:3, :3] = (S[:3, :3] / scale) @ c2w[:3, :3]
            moved[:3, 3] = S[:3, :3] @ c2w[:3, 3] + S[:3, 3]
            write_pose_line(fh, e.file, np.linalg.inv(moved), e.confidence_text, e.focal)
    res = run_command([tmp / "moved.ply", tmp / "gt.ply", "--thresholds", TAU + 1e-4, "--crop", "False", "--ace_pose_file", tmp / "moved_poses.txt",
                       "--gt_pose_files", str(tmp / "gt_poses" / "*.pose.txt"), "--output_json", tmp / "aligned.json"])
    identity = json.loads(room["runs"][0])
    assert np.allclose(np.array(res["transform"]), np.linalg.inv(S), atol=1e-5)
    # the poses are exact, so the residual is rounding: 1e-4 m is about 1000 float32 ulps at these coordinates
    assert res["precision"][0] == 1.0
    assert res["recall"][0] >= identity["recall"][1]
    with pytest.raises(SystemExit, match="alignment .* failed"):
        run_command([tmp / "moved.ply", tmp / "gt.ply", "--ace_pose_file", tmp / "moved_poses.txt", "--gt_pose_files",
                     str(tmp / "gt_poses" / "*.pose.txt"), "--estimate_alignment_conf_threshold", "1e9", "--output_json", tmp / "none.json"])
