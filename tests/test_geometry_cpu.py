"""CPU: the DEFINITION of the cloud distances (include/acez.h section N) checked on its numpy restatement
(tests/geometry_restated.py) against scipy's k-d tree, so that the kernels' bit-for-bit parity with it (tests/test_geometry_gpu.py)
means something; the PLY point reader, the F-score arithmetic, eval_geometry.py's refusals and the entry points' argument checks,
none of which needs a device."""
import numpy as np
import pytest
import torch

from tests import fusion_cases as FC
from tests import geometry_cases as GC
from tests import geometry_restated as R

F = np.float32
REL = 1e-6


def test_restatement_agrees_with_a_kd_tree():
    from scipy.spatial import cKDTree
    radius, thresholds = 0.05, (0.01, 0.02, 0.05)
    for seed, (n, m) in enumerate(((1500, 2500), (2500, 1500), (700, 4000))):
        q, p = GC.surface(100 + seed, n), GC.surface(200 + seed, m)
        d2, idx = R.nearest(q, p, radius)
        dist, nn = cKDTree(p.astype(np.float64)).query(q.astype(np.float64), k=2)
        # the clouds are chosen so that no distance is within REL of a threshold or of the radius: every decision is then the same in
        # float32 and in float64
        for t in thresholds + (radius,):
            assert (np.abs(dist[:, 0] - float(F(t))) > 4 * REL * t).all(), f"seed {seed}: a distance too close to {t}"
        found = dist[:, 0] <= float(F(radius))
        assert 0.2 * n < found.sum() < n, "the case should have queries with and without a reference in reach"
        assert np.array_equal(np.isfinite(d2), found) and np.array_equal(idx >= 0, found)
        assert np.allclose(np.sqrt(d2[found].astype(np.float64)), dist[found, 0], rtol=REL, atol=0)
        clear = found & (dist[:, 1] - dist[:, 0] > REL * dist[:, 1])
        assert clear.sum() > 0.9 * found.sum() and np.array_equal(idx[clear], nn[clear, 0])
        for t in thresholds:
            assert np.count_nonzero(d2 <= F(t) * F(t)) == np.count_nonzero(dist[:, 0] <= float(F(t)))
        # the k-d tree shortcut of the end-to-end test gives the scan's d2
        assert np.array_equal(R.nearest_d2_tree(q, p, radius).view(np.uint32), d2.view(np.uint32))


def test_restated_edge_cases():
    cases = GC.search_cases()
    d2, idx = R.nearest(*cases["exactly_the_radius"][:3])
    r2 = F(0.75) * F(0.75)
    assert d2[0] == r2 and d2[2] == r2 and idx[0] == 0 and idx[2] == 0
    q = cases["exactly_the_radius"][0]
    assert (q[1, 0] * q[1, 0] + q[1, 1] * q[1, 1]) + q[1, 2] * q[1, 2] == np.nextafter(r2, F(1))     # the next float above R * R
    assert np.isinf(d2[1]) and np.isinf(d2[3]) and idx[1] == -1 and idx[3] == -1
    d2, idx = R.nearest(*cases["no_reference"][:3])
    assert np.isinf(d2).all() and (idx == -1).all()
    q, p, r, _ = cases["duplicates"]
    d2, idx = R.nearest(q, p, r)
    assert (idx[idx >= 0] < 500).all(), "of duplicated points the lowest row wins"
    q, p, r, _ = cases["not_finite"]
    d2, idx = R.nearest(q, p, r)
    assert (idx[[0, 17, 63, 64, 299]] == -1).all() and not np.isin(idx, [5, 100]).any() and (idx >= 0).sum() > 200
    q, p, r, c = cases["straddling_a_face"]
    d2, idx = R.nearest(q, p, r)
    lo = p.min(0)
    dims = [int(v) + 1 for v in np.floor((p.max(0) - lo) / F(c))]
    apart = np.abs(np.floor((q - lo) / F(c)) - np.floor((p - lo) / F(c))).max(1)
    assert (idx >= 0).all() and (apart == 1).sum() > 300, "pairs within the radius whose cells differ"
    assert apart.max() == 1 and max(dims) <= 1024, "a reference within the radius is never two cells away"


def test_cells_and_downsample_restated():
    pts = np.array([[0, 0, 0], [0.25, 0.5, 0.75], [0.2499999, 0, 0], [1.0, 0, 0], [-1e-9, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]], F)
    assert R.cells(pts, (0, 0, 0), 0.25, (4, 4, 4)).tolist() == [0, (3 * 4 + 2) * 4 + 1, 0, -1, -1, -1, -1]
    pts, voxel = GC.downsample_cases()["crowd_and_singles"]
    out = R.voxel_downsample(pts, voxel)
    c = R.cells(pts, pts.min(0), voxel, (6, 6, 6))
    counts = np.bincount(c)
    assert counts.max() >= 3000 and (counts == 1).sum() >= 10 and len(out) == (counts > 0).sum()
    # against float64 means: the sequential float32 sum of 3000 values of about 0.55 is within 3000 * 2^-24 relative of it
    want = np.stack([pts[c == v].astype(np.float64).mean(0) for v in np.unique(c)])
    assert np.allclose(out, want, rtol=3000 * 2.0 ** -24, atol=0)
    single = np.unique(c)[counts[np.unique(c)] == 1]
    assert all(np.array_equal(out[np.searchsorted(np.unique(c), v)], pts[c == v][0]) for v in single)
    assert len(R.voxel_downsample(GC.downsample_cases()["a_nan"][0], 0.1)) == len(out)


def test_read_ply_points(tmp_path):
    from acezero_amd.formats import read_ply_points, read_ply_vertices, write_ply
    rng = np.random.default_rng(2)
    xyz = rng.normal(size=(50, 3)).astype(F)
    rgb = rng.integers(0, 256, (50, 3), dtype=np.uint8)
    faces = rng.integers(0, 50, (20, 3)).astype(np.int32)
    write_ply(tmp_path / "own.ply", xyz, rgb, faces)
    write_ply(tmp_path / "no_alpha.ply", xyz, rgb, alpha=False)
    assert np.array_equal(read_ply_points(tmp_path / "own.ply"), xyz) and np.array_equal(read_ply_vertices(tmp_path / "own.ply"), xyz)
    assert np.array_equal(read_ply_points(tmp_path / "no_alpha.ply"), xyz)
    # doubles and normals, another property order, a comment and a face element
    rec = np.zeros(50, dtype=[("nx", "<f4"), ("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("ny", "<f4"), ("nz", "<f4"), ("intensity", "<u2")])
    rec["x"], rec["y"], rec["z"], rec["nx"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 7.0
    head = ("ply\nformat binary_little_endian 1.0\ncomment a scanner wrote this\nelement vertex 50\nproperty float nx\nproperty double x\n"
            "property double y\nproperty float64 z\nproperty float ny\nproperty float32 nz\nproperty ushort intensity\nelement face 0\n"
            "property list uchar int vertex_indices\nend_header\n")
    (tmp_path / "doubles.ply").write_bytes(head.encode() + rec.tobytes())
    got = read_ply_points(tmp_path / "doubles.ply")
    assert got.dtype == F and got.flags["C_CONTIGUOUS"] and np.array_equal(got, xyz)
    with pytest.raises(SystemExit, match="vertex layout"):
        read_ply_vertices(tmp_path / "doubles.ply")
    text = "ply\nformat ascii 1.0\nelement vertex 3\nproperty float y\nproperty float x\nproperty float z\nproperty uchar red\nend_header\n"
    text += "1 0 2 255\n1.5 -2.5e-1 3 0\n4 5 6 7\n"
    (tmp_path / "ascii.ply").write_text(text)
    assert np.array_equal(read_ply_points(tmp_path / "ascii.ply"), np.array([[0, 1, 2], [-0.25, 1.5, 3], [5, 4, 6]], F))
    (tmp_path / "cut.ply").write_bytes((tmp_path / "doubles.ply").read_bytes()[:-40])
    (tmp_path / "cut_ascii.ply").write_text(text[:-6])
    (tmp_path / "no_x.ply").write_bytes(head.replace("double x", "double u").encode() + rec.tobytes())
    (tmp_path / "big_endian.ply").write_bytes(head.replace("little", "big").encode() + rec.tobytes())
    (tmp_path / "not_a.ply").write_bytes(b"solid mesh\n")
    for name, text in (("cut.ply", "truncated"), ("cut_ascii.ply", "truncated"), ("no_x.ply", "no x, y, z"), ("big_endian.ply", "little-endian"),
                       ("not_a.ply", "not a .ply")):
        with pytest.raises(SystemExit, match=text) as e:
            read_ply_points(tmp_path / name)
        assert name in str(e.value)


def test_fscore_arithmetic():
    from acezero_amd import geometry as G
    inf = np.inf
    clip = lambda r: float(np.sqrt(np.float64(F(r) * F(r))))    # what a distance is clipped to: the root of the float32 square
    for mod in (G, R):
        s = mod.scores(np.array([inf, inf, inf], F), np.array([inf, inf], F), [0.01, 0.02], 0.02)
        assert s["precision"] == [0.0, 0.0] and s["recall"] == [0.0, 0.0] and s["fscore"] == [0.0, 0.0]       # P = R = 0: no division
        assert s["accuracy_mean"] == s["accuracy_median"] == s["completeness_median"] == clip(0.02)     # all clipped
        # d2 of 1, 3, 2, 4 mm and nothing; the threshold's square is the float32 product
        d2_rec = (np.array([0.001, 0.003, 0.002, 0.004], F) ** 2).astype(F)
        d2_rec = np.append(d2_rec, F(inf))
        d2_gt = np.array([F(0.002) * F(0.002), inf, inf, inf], F)
        s = mod.scores(d2_rec, d2_gt, [0.002, 0.0035], 0.01)
        assert s["rec_within"] == [2, 3] and s["gt_within"] == [1, 1]
        assert s["precision"] == [2 / 5, 3 / 5] and s["recall"] == [1 / 4, 1 / 4]
        assert s["fscore"] == [2 * (2 / 5) * (1 / 4) / (2 / 5 + 1 / 4), 2 * (3 / 5) * (1 / 4) / (3 / 5 + 1 / 4)]
        # the median is element n // 2 of the sorted distances: of 1, 2, 3, 4, 10 mm the third, of 2, 10, 10, 10 mm the third
        assert s["accuracy_median"] == float(np.sqrt(np.float64(d2_rec[1]))) and s["completeness_median"] == clip(0.01)
        assert s["accuracy_mean"] == pytest.approx((0.001 + 0.002 + 0.003 + 0.004 + 0.01) / 5, rel=1e-6)
    assert G.fscore(0.0, 0.0) == 0.0 and G.fscore(1.0, 1.0) == 1.0 and G.fscore(0.5, 0.25) == pytest.approx(1 / 3)


def test_crop_count_and_transform_direction():
    from acezero_amd import geometry as G
    gt = GC.surface(31, 3000)
    rec = np.concatenate([GC.surface(32, 2000), np.array([[1.2, 0, 0.5], [0, -1.2, 0.5], [0, 0, 1.2], [np.nan, 0, 0], [1.04, 0, 0.5]], F)])
    kept, dropped = R.crop(rec, gt, 0.05)
    assert dropped == 4 and len(kept) == len(rec) - 4, "three points beyond the box + 5 cm and the NaN; the one 4 cm outside stays"
    kept_t, dropped_t = G.crop_to_box(torch.from_numpy(rec), torch.from_numpy(gt), 0.05)
    assert dropped_t == 4 and np.array_equal(kept_t.numpy(), kept)
    # a cloud moved by a known similarity, given the transform back, scores as the unmoved one: `transform` maps reconstruction -> gt
    T = GC.similarity()
    moved = R.apply_similarity(rec[:2000], T)
    back = np.linalg.inv(T)
    assert np.array_equal(G.apply_similarity(torch.from_numpy(moved), back).numpy(), R.apply_similarity(moved, back))
    assert np.abs(R.apply_similarity(moved, back) - rec[:2000]).max() < 1e-6
    plain = R.evaluate(rec[:2000], gt, [0.02, 0.05], search=R.nearest_d2_tree)
    aligned = R.evaluate(moved, gt, [0.02, 0.05], transform=back, search=R.nearest_d2_tree)
    wrong = R.evaluate(moved, gt, [0.02, 0.05], transform=T, do_crop=False, search=R.nearest_d2_tree)
    assert 0.1 < plain["precision"][0] < plain["precision"][1] <= 1.0
    for k in range(2):       # the round trip moves a point by float32 rounding, some 1e-7 m: a count may move by the points that close to a threshold
        assert abs(aligned["rec_within"][k] - plain["rec_within"][k]) <= 2 and abs(aligned["gt_within"][k] - plain["gt_within"][k]) <= 2
    assert wrong["precision"][1] < 0.05


def test_host_tensors_are_refused():
    from acezero_amd import geometry as G
    pts = torch.zeros(4, 3)
    for call in (lambda: G.nearest_distances(pts, pts, 0.1), lambda: G.voxel_downsample(pts, 0.1),
                 lambda: G.evaluate_geometry(pts, pts, [0.1])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_argument_validation_without_device():
    from acezero_amd import _native as N
    lib = N.lib()
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data                                          # never dereferenced: every call below is refused before any launch

    def refused(rc, text):
        assert rc == -1 and text in lib.acez_last_error(), (rc, lib.acez_last_error())

    def cells(pts=p, n=10, o=(0.0, 0.0, 0.0), c=0.1, dims=(4, 4, 4), out=p):
        return lib.acez_geom_cells(pts, n, *o, c, *dims, out, None)

    def nearest(ref=p, ref_index=p, start=p, m=10, o=(0.0, 0.0, 0.0), c=0.1, dims=(4, 4, 4), q=p, n=10, r=0.05, d2=p, idx=p):
        return lib.acez_geom_nearest(ref, ref_index, start, m, *o, c, *dims, q, n, r, d2, idx, None)

    def means(pts=p, n=10, start=p, s=3, out=p):
        return lib.acez_geom_voxel_means(pts, n, start, s, out, None)

    refused(cells(pts=None), b"null pointer")
    refused(cells(out=None), b"null pointer")
    refused(cells(n=-1), b"count")
    refused(cells(n=2 ** 31), b"count")
    refused(cells(dims=(4, 0, 4)), b"dimensions")
    refused(cells(dims=(4, 4, 1025)), b"dimensions")
    refused(cells(dims=(1024, 1024, 17)), b"too large")
    refused(cells(c=0.0), b"cell edge")
    refused(cells(c=-0.1), b"cell edge")
    refused(cells(c=float("nan")), b"cell edge")
    refused(cells(c=float("inf")), b"cell edge")
    refused(cells(o=(0.0, float("inf"), 0.0)), b"origin")
    for name in ("ref", "ref_index", "start", "q", "d2", "idx"):
        refused(nearest(**{name: None}), b"null pointer")
    refused(nearest(m=-1), b"count")
    refused(nearest(n=-1), b"count")
    refused(nearest(m=2 ** 31), b"count")
    refused(nearest(n=2 ** 31), b"count")
    refused(nearest(dims=(0, 4, 4)), b"dimensions")
    refused(nearest(dims=(1025, 4, 4)), b"dimensions")
    refused(nearest(dims=(512, 512, 65)), b"too large")
    refused(nearest(c=float("nan")), b"cell edge")
    refused(nearest(c=0.0, r=0.0), b"cell edge")
    refused(nearest(r=0.0), b"radius")
    refused(nearest(r=-0.05), b"radius")
    refused(nearest(r=float("inf")), b"radius")
    refused(nearest(r=float("nan")), b"radius")
    refused(nearest(c=0.05, r=0.05), b"2^-10")                   # c = R exactly
    refused(nearest(c=float(F(0.05) * F(1 + 2.0 ** -11)), r=0.05), b"2^-10")
    refused(means(pts=None), b"null pointer")
    refused(means(start=None), b"null pointer")
    refused(means(out=None), b"null pointer")
    refused(means(n=-1), b"count")
    refused(means(s=-1), b"count")
    refused(means(s=2 ** 31), b"count")
    if not torch.cuda.is_available():                            # what is valid gets as far as the device check, and no further
        for rc in (cells(), nearest(), nearest(c=float(F(0.05) * GC.MARGIN), r=0.05), means()):
            assert rc == -3 and b"no HIP device" in lib.acez_last_error()


def test_cli_refusals(tmp_path):
    from acezero_amd import cli
    from acezero_amd.formats import write_ply
    pts = GC.uniform(1, 20)
    rec, gt = str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply")
    write_ply(rec, pts, np.zeros((20, 3), np.uint8))
    write_ply(gt, pts, np.zeros((20, 3), np.uint8))
    np.savetxt(tmp_path / "T.txt", np.eye(4))
    (tmp_path / "poses.txt").write_text("")
    with pytest.raises(SystemExit, match="not both"):
        cli.eval_geometry_main([rec, gt, "--transform", str(tmp_path / "T.txt"), "--ace_pose_file", str(tmp_path / "poses.txt"),
                                "--gt_pose_files", str(tmp_path / "*.pose.txt")])
    with pytest.raises(SystemExit, match="go together"):
        cli.eval_geometry_main([rec, gt, "--ace_pose_file", str(tmp_path / "poses.txt")])
    with pytest.raises(SystemExit, match="missing.ply: no such file"):
        cli.eval_geometry_main([str(tmp_path / "missing.ply"), gt])
    with pytest.raises(SystemExit, match="nowhere.ply: no such file"):
        cli.eval_geometry_main([rec, str(tmp_path / "nowhere.ply")])
    with pytest.raises(SystemExit, match="T2.txt: no such file"):
        cli.eval_geometry_main([rec, gt, "--transform", str(tmp_path / "T2.txt")])
    with pytest.raises(SystemExit, match="must be positive"):
        cli.eval_geometry_main([rec, gt, "--thresholds", "0.01", "-0.02"])
    with pytest.raises(SystemExit, match="must be positive"):
        cli.eval_geometry_main([rec, gt, "--voxel_size", "0"])


def test_room_lattice():
    gt = GC.room_lattice()
    assert gt.dtype == F and 356000 < len(gt) < 358000
    assert FC.wall_distance(gt).max() < 1e-7 and (np.abs(gt) <= FC.ROOM_HALF.astype(F) + 1e-7).all()
    corner = np.abs(np.abs(gt) - FC.ROOM_HALF).max(1) < 1e-6
    assert corner.sum() == 8 * 3, "every corner once per wall that meets there"
