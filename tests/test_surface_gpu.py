"""GPU: the face sampler and the polygon crop of acezero_amd/csrc/surface_api.hip against the numpy restatement of their definition
(tests/surface_restated.py, itself checked in tests/test_surface_cpu.py), bit for bit; the entry points' argument checks with device
buffers; eval_geometry.py --sample_spacing / --crop_file end to end on the box room written as its exact surface."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import fusion_cases as FC
from tests import geometry_cases as GC
from tests import geometry_restated as R
from tests import surface_cases as SC
from tests import surface_restated as SR

pytestmark = pytest.mark.gpu
F = np.float32
MESHES = SC.mesh_cases()
CROPS = SC.crop_cases()


@functools.lru_cache(maxsize=None)
def reference(name, seed):
    v, f, spacing, colours = MESHES[name]
    counts, areas = SR.face_counts(v, f, SR.density_of(spacing), seed)
    return counts, areas, SR.sample_mesh(v, f, spacing, seed, colours)


def device_counts(v, f, spacing, seed):
    from acezero_amd import _native as N
    from acezero_amd.head import _ptr
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    counts = torch.full((len(f),), -7, dtype=torch.int32, device="cuda")
    areas = torch.full((len(f),), -7.0, dtype=torch.float64, device="cuda")
    N.check(N.lib().acez_geom_face_counts(_ptr(vd), len(v), _ptr(fd), len(f), SR.density_of(spacing), seed, _ptr(counts), _ptr(areas), None))
    torch.cuda.synchronize()
    return counts.cpu().numpy(), areas.cpu().numpy()


def sample(v, f, spacing, seed, colours):
    from acezero_amd.geometry import sample_mesh
    points, face, col, info = sample_mesh(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), spacing=spacing, seed=seed,
                                          colours=None if colours is None else torch.from_numpy(colours).cuda())
    assert points.dtype == torch.float32 and face.dtype == torch.int32 and points.shape == (info["samples"], 3) and face.shape == (info["samples"],)
    assert (col is None) == (colours is None) and (col is None or (col.dtype == torch.uint8 and col.shape == points.shape))
    return points.cpu().numpy(), face.cpu().numpy(), None if col is None else col.cpu().numpy(), info


def assert_same_samples(got, want, what):
    assert got[3] == want[3], (what, got[3], want[3])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), f"{what}: points differ"
    assert np.array_equal(got[1], want[1]), f"{what}: face indices differ"
    assert (got[2] is None) == (want[2] is None) and (got[2] is None or np.array_equal(got[2], want[2])), f"{what}: colours differ"


@pytest.mark.parametrize("name", sorted(MESHES))
def test_counts_and_samples_match_the_restatement(name):
    v, f, spacing, colours = MESHES[name]
    for seed in (0, 5):
        want_counts, want_areas, want = reference(name, seed)
        counts, areas = device_counts(v, f, spacing, seed)
        ulps = np.abs(areas.view(np.int64) - want_areas.view(np.int64)).max() if len(f) else 0
        print(f"{name}, seed {seed}: {len(f)} faces, {int(want_counts.sum())} samples, areas differ by at most {ulps} ulp")
        assert np.array_equal(areas.view(np.uint64), want_areas.view(np.uint64)), f"{name}: areas differ by up to {ulps} ulp"
        assert np.array_equal(counts, want_counts)
        got = sample(v, f, spacing, seed, colours)
        assert_same_samples(got, want, f"{name}, seed {seed}")
        if seed == 0:
            assert_same_samples(sample(v, f, spacing, seed, colours), got, f"{name}: the second run")
            if colours is not None:                               # the points do not depend on whether colours are asked for
                assert np.array_equal(sample(v, f, spacing, seed, None)[0], got[0])


def test_what_the_cases_are_for():
    counts, areas, (points, face, _, info) = reference("one_face_100k", 0)
    assert counts.tolist() == [len(points)] and len(points) >= 100000
    counts, areas, (points, face, _, info) = reference("sparse_5000", 0)
    assert (counts == 0).mean() > 0.8 and counts.max() >= 1 and np.diff(face).max() > 20, "runs of faces without samples between two samples"
    counts, areas, (points, face, _, info) = reference("degenerate", 0)
    assert info["faces_invalid"] == 5 and (areas[[5, 11, 12]] == 0).all() and np.isfinite(points).all()
    assert not np.isin(face, [5, 11, 12, 20, 21, 33, 40, 41]).any()
    assert reference("k0", 0)[2][3] == {"faces": 0, "faces_invalid": 0, "area": 0.0, "samples": 0}
    for name in ("k63", "k64", "k65", "k257"):
        counts = reference(name, 0)[0]
        assert counts.sum() > 256 and (counts == 0).any() and np.unique(reference(name, 0)[2][1]).size > 40, name


def test_shuffled_faces_and_other_seeds():
    perm = SC.shuffle()
    plain, shuffled = reference("k257", 0), reference("k257_shuffled", 0)
    v, f, spacing, colours = MESHES["k257_shuffled"]
    counts, areas = device_counts(v, f, spacing, 0)
    assert np.array_equal(areas.view(np.uint64), plain[1][perm].view(np.uint64)), "a face's area does not depend on its row"
    info = sample(v, f, spacing, 0, colours)[3]
    assert info["area"] == plain[2][3]["area"], "the sum is exactly rounded: the order of the faces does not change it"
    # two seeds: other points, and counts that differ only in the draw of the remainder
    v, f, spacing, colours = MESHES["k257"]
    a, b = sample(v, f, spacing, 0, colours), sample(v, f, spacing, 12345, colours)
    ca, cb = np.bincount(a[1], minlength=257), np.bincount(b[1], minlength=257)
    assert np.abs(ca - cb).max() == 1 and abs(int(ca.sum()) - int(cb.sum())) < 5 * np.sqrt(257 * 0.25)
    n = min(len(a[0]), len(b[0]))
    assert not np.array_equal(a[0][:n], b[0][:n]) and a[3]["area"] == b[3]["area"]


def test_empty_results_and_the_sample_limit():
    from acezero_amd.geometry import sample_mesh
    v = torch.from_numpy(np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], F)).cuda()
    for faces in (np.zeros((0, 3), np.int32), np.array([[0, 1, 2], [3, 3, 3], [0, 1, 9]], np.int32)):
        colours = torch.zeros((4, 3), dtype=torch.uint8, device="cuda")
        points, face, col, info = sample_mesh(v, torch.from_numpy(faces).cuda(), spacing=0.01, colours=colours)
        assert points.shape == (0, 3) and face.shape == (0,) and col.shape == (0, 3) and info["samples"] == 0 and info["area"] == 0.0
        assert info["faces"] == len(faces) and info["faces_invalid"] == (1 if len(faces) else 0)
    big = torch.from_numpy(np.array([[0, 1, 3]] * 3, np.int32)).cuda()        # 0.5 m^2 each at 10 um: 5e9 samples, capped at 2^30 a face
    with pytest.raises(ValueError, match="use a larger spacing"):
        sample_mesh(v, big, spacing=1e-5)
    with pytest.raises(ValueError, match="expected integer faces"):
        sample_mesh(v, big.float(), spacing=0.1)
    with pytest.raises(ValueError, match="colours"):
        sample_mesh(v, big, spacing=0.1, colours=torch.zeros((3, 3), dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("name", sorted(CROPS))
def test_crop_matches_the_restatement(name):
    from acezero_amd.formats import CropVolume
    from acezero_amd.geometry import crop_to_polygon, polygon_mask
    points, polygon, axis, lo, hi = CROPS[name]
    want = SR.crop_keep(points, polygon, axis, lo, hi)
    crop = CropVolume(polygon, axis, F(lo), F(hi))
    pd = torch.from_numpy(points).cuda()
    keep = polygon_mask(pd, crop)
    assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), want), name
    kept, dropped = crop_to_polygon(pd, crop)
    assert dropped == int((~want).sum()) and np.array_equal(kept.cpu().numpy().view(np.uint32), points[want].view(np.uint32))
    assert np.array_equal(polygon_mask(pd, crop).cpu().numpy(), want), "the second run"


def test_argument_validation_with_device_buffers():
    from acezero_amd import _native as N
    from acezero_amd.head import _ptr
    lib = N.lib()
    v, f, spacing, colours = MESHES["k64"]
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    want_counts, want_areas, want = reference("k64", 0)
    n = len(want[0])
    offsets = torch.from_numpy(SR.offsets_of(want_counts)).cuda()
    counts = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    areas = torch.full((64,), -7.0, dtype=torch.float64, device="cuda")
    points = torch.full((n, 3), -7.0, device="cuda")
    face = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    polygon = torch.from_numpy(SC.TRIANGLE).cuda()
    col = torch.zeros((len(v), 3), dtype=torch.uint8, device="cuda")

    def count(m=len(v), k=64, density=SR.density_of(spacing), faces=fd):
        return lib.acez_geom_face_counts(_ptr(vd), m, _ptr(faces), k, density, 0, _ptr(counts), _ptr(areas), None)

    def draw(m=len(v), k=64, n=n, off=offsets, colours=None, out=points):
        return lib.acez_geom_sample_faces(_ptr(vd), m, _ptr(fd), k, _ptr(off), n, 0, _ptr(colours), _ptr(out), _ptr(face), None, None)

    def crop(n=n, corners=3, axis=2, lo=-1.0, hi=1.0, poly=polygon):
        return lib.acez_geom_crop_polygon(_ptr(points), n, _ptr(poly), corners, axis, lo, hi, _ptr(keep), None)

    assert count(k=-1) == -1 and count(m=2 ** 31) == -1 and b"count" in lib.acez_last_error()
    assert count(density=0.0) == -1 and count(density=float("inf")) == -1 and count(density=float("nan")) == -1 and b"density" in lib.acez_last_error()
    assert count(faces=None) == -1 and b"null pointer" in lib.acez_last_error()
    assert draw(n=-1) == -1 and draw(n=2 ** 31) == -1 and b"count" in lib.acez_last_error()
    assert draw(off=None) == -1 and draw(out=None) == -1 and b"null pointer" in lib.acez_last_error()
    assert draw(m=0) == -1 and draw(k=0) == -1 and b"without vertices" in lib.acez_last_error()
    assert draw(colours=col) == -1 and b"go together" in lib.acez_last_error()
    assert crop(corners=2) == -1 and crop(corners=1025) == -1 and b"corners" in lib.acez_last_error()
    assert crop(axis=3) == -1 and b"axis" in lib.acez_last_error()
    assert crop(lo=1.0, hi=-1.0) == -1 and crop(hi=float("nan")) == -1 and b"bounds" in lib.acez_last_error()
    assert crop(poly=None) == -1 and b"null pointer" in lib.acez_last_error()
    with pytest.raises(N.AcezError, match="ACEZ_ERR_INVALID"):
        N.check(count(density=-1.0))
    torch.cuda.synchronize()                                     # nothing was launched by the refused calls; the device is fine
    assert (counts == -7).all() and (areas == -7.0).all() and (points == -7.0).all() and (face == -7).all() and (keep == 7).all()
    assert count() == 0 and draw() == 0
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy(), want_counts) and np.array_equal(points.cpu().numpy(), want[0]) and np.array_equal(face.cpu().numpy(), want[1])
    assert crop() == 0
    torch.cuda.synchronize()
    assert np.array_equal(keep.cpu().numpy().astype(bool), SR.crop_keep(want[0], SC.TRIANGLE, 2, -1.0, 1.0))


# ------------------------------------------------------------------------------------------------------------ end to end
THRESHOLDS = [0.004, 0.02]
SPACING = 0.005


def run_command(argv):
    from acezero_amd import cli
    assert cli.eval_geometry_main([str(a) for a in argv]) == 0
    return json.load(open(argv[argv.index("--output_json") + 1]))


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    """The box room as its exact surface (8 vertices, 12 triangles, coloured), the ground-truth lattice as a .ply, the restated samples
    at 5 mm and their restated scores."""
    from acezero_amd.formats import write_ply
    tmp = tmp_path_factory.mktemp("surface_room")
    v, f = SC.box_room()
    colours = np.random.default_rng(4).integers(0, 256, (8, 3), dtype=np.uint8)
    write_ply(tmp / "rec.ply", v, colours, f)
    gt = GC.room_lattice()
    write_ply(tmp / "gt.ply", gt, np.full((len(gt), 3), 128, np.uint8), alpha=False)
    samples = SR.sample_mesh(v, f, SPACING, 0, colours)
    want = R.evaluate(samples[0], gt, THRESHOLDS, do_crop=False, search=R.nearest_d2_tree)
    common = [tmp / "gt.ply", "--thresholds", *THRESHOLDS, "--crop", "False", "--output_json"]
    return dict(tmp=tmp, v=v, f=f, colours=colours, gt=gt, samples=samples, want=want, common=common)


def test_a_mesh_scored_by_its_vertices(room):
    res = run_command([room["tmp"] / "rec.ply"] + room["common"] + [room["tmp"] / "vertices.json"])
    assert res["rec_points"] == 8 and res["recall"][1] < 0.01 and res["precision"] == [1.0, 1.0]
    assert "sampling" not in res and "crop_file" not in res


def test_a_mesh_scored_by_its_surface(room, caplog):
    from acezero_amd.formats import read_ply_mesh
    tmp, want = room["tmp"], room["want"]
    argv = [tmp / "rec.ply"] + room["common"]
    with caplog.at_level("INFO"):
        res = run_command(argv + [tmp / "surface_0.json", "--sample_spacing", SPACING, "--write_samples", tmp / "samples.ply"])
    run_command(argv + [tmp / "surface_1.json", "--sample_spacing", SPACING, "--write_samples", tmp / "samples_1.ply"])
    assert (tmp / "surface_0.json").read_bytes() == (tmp / "surface_1.json").read_bytes(), "two runs wrote different files"
    assert (tmp / "samples.ply").read_bytes() == (tmp / "samples_1.ply").read_bytes()
    assert res["precision"][0] == 1.0 and res["recall"][1] == 1.0
    assert res["sampling"] == dict(room["samples"][3], seed=0, spacing=SPACING) and res["sampling"]["samples"] == 354016
    assert "crop_file" not in res and res["transform"] is None
    for k in ("rec_points", "gt_points", "rec_within", "gt_within", "precision", "recall", "fscore", "accuracy_median", "completeness_median"):
        assert res[k] == want[k], (k, res[k], want[k])
    points, colours, faces = read_ply_mesh(tmp / "samples.ply")
    assert np.array_equal(points.view(np.uint32), room["samples"][0].view(np.uint32)) and np.array_equal(colours, room["samples"][2]) and len(faces) == 0
    assert "Sampled 354016 points, 0.005 m apart, from the 12 faces of the reconstruction" in caplog.text
    other = run_command(argv + [tmp / "seed.json", "--sample_spacing", SPACING, "--sample_seed", 2019])
    assert other["sampling"]["samples"] == 354016 and other["sampling"]["seed"] == 2019 and other["precision"][0] == 1.0 and other["recall"][1] == 1.0


def test_the_density_is_that_of_the_ground_truths_frame(room):
    """The room moved by a similarity of scale 1.3 and given back through --transform: the vertices are moved first, the samples are
    drawn from the moved mesh, so the mesh gets the samples of the unmoved one, to within one per face."""
    from acezero_amd.formats import write_ply
    tmp = room["tmp"]
    S = GC.similarity(scale=1.3)
    write_ply(tmp / "moved.ply", R.apply_similarity(room["v"], S), room["colours"], room["f"])
    np.savetxt(tmp / "back.txt", np.linalg.inv(S))
    res = run_command([tmp / "moved.ply", tmp / "gt.ply", "--thresholds", 0.004 + 1e-4, 0.02, "--crop", "False", "--transform", tmp / "back.txt",
                       "--sample_spacing", SPACING, "--output_json", tmp / "moved.json"])
    assert abs(res["sampling"]["samples"] - 354016) <= 12
    assert np.allclose(res["transform"], np.linalg.inv(S), rtol=0, atol=1e-12)
    back = R.apply_similarity(R.apply_similarity(room["v"], S), np.linalg.inv(S))
    want = SR.sample_mesh(back, room["f"], SPACING, 0)[3]
    assert {k: res["sampling"][k] for k in want} == want
    # the round trip moves a vertex by float32 rounding, some 1e-7 m: 0.1 mm on the first threshold covers it
    assert res["precision"][0] == 1.0 and res["recall"][1] == 1.0


def test_a_crop_file_over_half_the_room(room, caplog):
    tmp = room["tmp"]
    doc = {"class_name": "SelectionPolygonVolume", "orthogonal_axis": "Z", "axis_min": -1.0, "axis_max": 1.0, "version_major": 1,
           "bounding_polygon": [[0.0, -1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]]}
    (tmp / "half.json").write_text(json.dumps(doc))
    polygon = np.array([[0, -1], [1, -1], [1, 1], [0, 1]], F)
    keep = SR.crop_keep(room["samples"][0], polygon, 2, -1.0, 1.0)
    assert 0.4 * len(keep) < keep.sum() < 0.6 * len(keep)
    with caplog.at_level("INFO"):
        res = run_command([tmp / "rec.ply"] + room["common"] + [tmp / "half.json.scores", "--sample_spacing", SPACING, "--crop_file", tmp / "half.json",
                                                                "--write_samples", tmp / "half.ply"])
    assert res["crop_file"]["dropped"] == int((~keep).sum()) and res["rec_points"] == int(keep.sum()) and res["crop_file"]["corners"] == 4
    assert res["crop_file"]["orthogonal_axis"] == "Z" and "gt_dropped" not in res["crop_file"]
    assert res["precision"] == [1.0, 1.0] and 0.4 < res["recall"][1] < 0.6
    from acezero_amd.formats import read_ply_points
    assert np.array_equal(read_ply_points(tmp / "half.ply"), room["samples"][0][keep])
    assert f"{int((~keep).sum())} reconstruction points dropped" in caplog.text
    both = run_command([tmp / "rec.ply"] + room["common"] + [tmp / "both.json", "--sample_spacing", SPACING, "--crop_file", tmp / "half.json",
                                                             "--crop_file_ground_truth", "True"])
    gt_keep = SR.crop_keep(room["gt"], polygon, 2, -1.0, 1.0)
    assert both["crop_file"]["gt_dropped"] == int((~gt_keep).sum()) and both["gt_points"] == int(gt_keep.sum()) and both["recall"][1] == 1.0
    # the crop file alone, on the vertices: four of the eight have x >= 0
    plain = run_command([tmp / "rec.ply"] + room["common"] + [tmp / "plain.json", "--crop_file", tmp / "half.json"])
    assert plain["crop_file"]["dropped"] == 4 and plain["rec_points"] == 4 and "sampling" not in plain
    doc["bounding_polygon"] = [[5.0, 5.0, 0.0], [6.0, 5.0, 0.0], [6.0, 6.0, 0.0]]
    (tmp / "elsewhere.json").write_text(json.dumps(doc))
    with pytest.raises(SystemExit, match="reconstruction is empty after the crop file's polygon \\(8 points dropped\\)"):
        run_command([tmp / "rec.ply"] + room["common"] + [tmp / "none.json", "--crop_file", tmp / "elsewhere.json"])


def test_score_reconstruction_is_the_commands_pipeline(room, tmp_path):
    """geometry.score_reconstruction called directly -- surface samples, a crop volume, a --transform that is off by a centimetre and
    two ICP stages -- returns the numbers eval_geometry.py writes to --output_json for the same inputs (all but the crop file's name)
    and the points it writes to --write_samples, bit for bit."""
    from acezero_amd import geometry
    from acezero_amd.formats import read_crop_file, read_ply_mesh, read_ply_points, write_ply
    tmp, spacing, distances = room["tmp"], 0.02, [0.08, 0.04]
    S, off = GC.similarity(scale=1.3), np.eye(4)
    off[:3, 3] = [0.01, -0.005, 0.008]
    write_ply(tmp_path / "moved.ply", R.apply_similarity(room["v"], S), room["colours"], room["f"])
    np.savetxt(tmp_path / "nearly_back.txt", off @ np.linalg.inv(S))
    doc = {"orthogonal_axis": "Z", "axis_min": -1.0, "axis_max": 1.0, "bounding_polygon": [[0.0, -1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]]}
    (tmp_path / "half.json").write_text(json.dumps(doc))
    written = run_command([tmp_path / "moved.ply", tmp / "gt.ply", "--thresholds", *THRESHOLDS, "--transform", tmp_path / "nearly_back.txt",
                           "--sample_spacing", spacing, "--crop_file", tmp_path / "half.json", "--icp", "True", "--icp_distances", *distances,
                           "--icp_max_iterations", 5, "--write_samples", tmp_path / "scored.ply", "--output_json", tmp_path / "scores.json"])
    assert written["crop_file"].pop("file") == str(tmp_path / "half.json")
    v, colours, f = read_ply_mesh(tmp_path / "moved.ply")
    device = lambda a: torch.from_numpy(a).cuda()
    res, points, point_colours = geometry.score_reconstruction(
        device(v), device(read_ply_points(tmp / "gt.ply")), THRESHOLDS, rec_faces=device(f), rec_colours=device(colours),
        transform=np.loadtxt(tmp_path / "nearly_back.txt"), sample_spacing=spacing, crop_volume=read_crop_file(tmp_path / "half.json"),
        icp_distances=distances, icp_max_iterations=5)
    assert json.loads(json.dumps(res)) == written                       # (the round trip turns tuples into lists, nothing else)
    assert len(res["icp"]) == 2 and res["sampling"]["spacing"] == spacing and 0 < res["crop_file"]["dropped"] < res["sampling"]["samples"]
    assert res["transform_initial"] == np.loadtxt(tmp_path / "nearly_back.txt").tolist() and res["transform"] != res["transform_initial"]
    scored, scored_colours, _ = read_ply_mesh(tmp_path / "scored.ply")
    assert len(scored) == res["rec_points_read"] == res["sampling"]["samples"] - res["crop_file"]["dropped"]
    assert np.array_equal(points.cpu().numpy().view(np.uint32), scored.view(np.uint32))
    assert np.array_equal(point_colours.cpu().numpy(), scored_colours)


def test_the_fused_mesh_by_its_surface(room, tmp_path):
    """fuse_depth.py's surface-nets mesh of the room: eval_geometry.py samples it as the restatement does, and the recall below the
    voxel edge, which its vertices alone cannot reach, is there."""
    from acezero_amd import cli
    from acezero_amd.formats import read_ply_mesh
    args = FC.write_room_scene(tmp_path, 12, 120, 160, 100.0)
    assert cli.fuse_depth_main(args) == 0
    v, colours, f = read_ply_mesh(args[2])
    assert np.array_equal(v, FC.read_mesh_ply(args[2])[0]) and np.array_equal(f, FC.read_mesh_ply(args[2])[2]) and len(f) > 1000
    want = SR.sample_mesh(v, f, SPACING, 0)[3]
    # the twelve frames see a part of the walls. Of that part, at 5 mm, a quarter of the voxel edge, discs around the vertices of a
    # 20 mm grid cover pi 5^2 / 20^2 = 20%, while a lattice point there expects pi 5^2 / 5^2 = 3.1 samples in reach (2.6 with the
    # surface 2 mm off the wall), so some 90% have one: 4.6 times the recall, of which the test asks for 3
    command = [args[2], room["tmp"] / "gt.ply", "--thresholds", 0.005, "--crop", "False", "--output_json"]
    res = run_command(command + [tmp_path / "sampled.json", "--sample_spacing", SPACING])
    assert res["sampling"] == dict(want, seed=0, spacing=SPACING) and res["rec_points"] == want["samples"] > 10 * len(v)
    by_vertices = run_command(command + [tmp_path / "vertices.json"])
    print(f"{len(v)} vertices, {len(f)} faces, {want['samples']} samples: recall at 5 mm {by_vertices['recall'][0]:.4f} by vertices, "
          f"{res['recall'][0]:.4f} by surface")
    assert res["recall"][0] > 3 * by_vertices["recall"][0] > 0
