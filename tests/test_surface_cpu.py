"""CPU: the DEFINITION of the face sampler and of the polygon crop (include/acez.h section O) checked on its numpy restatement
(tests/surface_restated.py), so that the kernels' bit-for-bit parity with it (tests/test_surface_gpu.py) means something: the counts,
the fold, uniformity, the box room at 5 mm against the lattice, the crossing rule against matplotlib; the mesh and crop file readers,
eval_geometry.py's new refusals and the entry points' argument checks, none of which needs a device."""
import json

import numpy as np
import pytest
import torch

from tests import geometry_cases as GC
from tests import surface_cases as SC
from tests import surface_restated as SR

F = np.float32


def test_counts_are_floor_or_floor_plus_one():
    for name, (v, f, spacing, _) in SC.mesh_cases().items():
        for seed in (0, 5):
            counts, areas = SR.face_counts(v, f, SR.density_of(spacing), seed)
            valid = areas >= 0
            x = areas[valid] * SR.density_of(spacing)
            extra = counts[valid] - np.floor(x)
            assert ((extra == 0) | (extra == 1)).all() and (counts[~valid] == 0).all(), name
            assert (extra[x == np.floor(x)] == 0).all(), "u0 < 0 never holds: a whole x gets exactly x samples"
            # the cases stay clear of the decisions that one ulp of the area could move (what a device square root may differ by)
            assert not SC.area_guard(v, f, spacing, seed).any(), (name, seed)
    v, f, spacing, _ = SC.mesh_cases()["degenerate"]
    counts, areas = SR.face_counts(v, f, SR.density_of(spacing), 0)
    assert (areas[[20, 21, 33, 40, 41]] == -1.0).all() and (counts[[20, 21, 33, 40, 41]] == 0).all(), "indices -1, m, 2^31 - 1; NaN; infinity"
    assert (areas[[5, 11, 12]] == 0.0).all() and (counts[[5, 11, 12]] == 0).all(), "zero area is valid and gets no sample"
    assert (areas < 0).sum() == 5
    # the expectation: over many faces with x = 0.1 the total is the total of x, within 5 sigma of the Bernoulli sum
    v, f, spacing, _ = SC.mesh_cases()["sparse_5000"]
    counts, areas = SR.face_counts(v, f, SR.density_of(spacing), 3)
    x = areas * SR.density_of(spacing)
    assert x.max() < 1 and 0.05 < x.mean() < 0.2 and (counts == 0).mean() > 0.8
    assert abs(counts.sum() - x.sum()) < 5 * np.sqrt((x * (1 - x)).sum())


def test_samples_lie_in_their_triangle_and_are_uniform():
    for seed in (0, 7):
        t = np.repeat(np.arange(50), 400)
        i = np.tile(np.arange(400), 50)
        u, v = SR.barycentric(seed, t, i)
        assert (u >= 0).all() and (v >= 0).all() and (u + v <= 1).all()
    v, f = SC.unit_right_triangle()
    p, face, _ = SR.sample_faces(v, f, SR.offsets_of([20000]), 7)
    x, y = p[:, 0], p[:, 1]
    assert (face == 0).all() and (p[:, 2] == 0).all() and (x >= 0).all() and (y >= 0).all() and (x + y <= 1).all()
    parts = [int(((x < 0.5) & (y < 0.5) & (x + y <= 0.5)).sum()), int((x >= 0.5).sum()), int((y >= 0.5).sum()),
             int(((x < 0.5) & (y < 0.5) & (x + y > 0.5)).sum())]
    print("samples per medial sub-triangle:", parts)
    assert sum(parts) == 20000
    sigma = np.sqrt(20000 * 0.25 * 0.75)                          # 61.2: 5 sigma = 306
    assert all(abs(c - 5000) <= 5 * sigma for c in parts), parts
    # faces without samples are skipped: the face of every sample has a count, and every count is used up
    counts = np.array([0, 3, 0, 0, 2, 0], np.int32)
    vv, ff, _ = SC.random_mesh(3, 6)
    p, face, _ = SR.sample_faces(vv, ff, SR.offsets_of(counts), 1)
    assert face.tolist() == [1, 1, 1, 4, 4]
    # colours: a sample's colour is inside the corners' range, and a corner-coloured face gives the barycentric weights
    vv, ff, spacing, col = SC.mesh_cases()["one_face_100k"]
    p, face, c, info = SR.sample_mesh(vv, ff, spacing, 0, col)
    assert c.dtype == np.uint8 and len(c) == len(p) >= 100000 and info["samples"] == len(p)
    assert (c.min(0) >= col.min(0)).all() and (c.max(0) <= col.max(0)).all() and len(np.unique(c, axis=0)) > 1000


@pytest.fixture(scope="module")
def lattice_tree():
    from scipy.spatial import cKDTree
    gt = GC.room_lattice()
    return gt, cKDTree(gt.astype(np.float64))


@pytest.mark.parametrize("seed", SC.SEEDS)
def test_box_room_at_5_mm(seed, lattice_tree):
    from scipy.spatial import cKDTree
    gt, tree = lattice_tree
    v, f = SC.box_room()
    assert v.shape == (8, 3) and f.shape == (12, 3) and len(gt) == 356950
    p, face, _, info = SR.sample_mesh(v, f, 0.005, seed)
    assert info["samples"] == len(p) == 354016 and info["faces"] == 12 and info["faces_invalid"] == 0
    assert abs(info["area"] - 8.8504) < 1e-6
    to_lattice = tree.query(p.astype(np.float64))[0].max()
    to_samples = cKDTree(p.astype(np.float64)).query(gt.astype(np.float64))[0].max()
    print(f"seed {seed}: sample -> lattice at most {to_lattice * 1000:.3f} mm, lattice -> sample at most {to_samples * 1000:.3f} mm")
    assert to_lattice <= 0.00354, "every sample within sqrt(2) * 2.5 mm of a lattice point"
    assert to_samples <= 0.020, "every lattice point within 20 mm of a sample"
    if seed == SC.SEEDS[0]:
        reach = (cKDTree(v.astype(np.float64)).query(gt.astype(np.float64))[0] <= 0.020).mean()
        print(f"the 8 vertices alone reach {reach * 100:.2f}% of the lattice at 20 mm")
        assert 0.0010 < reach < 0.0012


def test_read_ply_mesh(tmp_path):
    from acezero_amd.formats import read_ply_mesh, read_ply_points, write_ply
    rng = np.random.default_rng(2)
    xyz = rng.normal(size=(50, 3)).astype(F)
    rgb = rng.integers(0, 256, (50, 3), dtype=np.uint8)
    faces = rng.integers(0, 50, (20, 3)).astype(np.int32)
    write_ply(tmp_path / "own.ply", xyz, rgb, faces)
    write_ply(tmp_path / "no_alpha.ply", xyz, rgb, faces, alpha=False)
    write_ply(tmp_path / "cloud.ply", xyz, rgb)
    for name in ("own.ply", "no_alpha.ply"):
        v, c, f = read_ply_mesh(tmp_path / name)
        assert np.array_equal(v, xyz) and np.array_equal(c, rgb) and np.array_equal(f, faces) and f.dtype == np.int32 and c.dtype == np.uint8
    v, c, f = read_ply_mesh(tmp_path / "cloud.ply")                # a file without faces
    assert np.array_equal(v, xyz) and f.shape == (0, 3) and f.dtype == np.int32
    # ASCII with quads, a pentagon and a triangle (the fan), another property order, no colours, a scalar after the list
    text = ("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 6\nproperty float y\nproperty float x\nproperty float z\n"
            "element face 4\nproperty list uchar int vertex_index\nproperty uchar flags\nend_header\n"
            "0 0 0\n0 1 0\n1 1 0\n1 0 0\n2 0 0.5\n2 1 0.5\n4 0 1 2 3 7\n3 3 2 5 0\n5 0 1 2 5 4 9\n4 1 2 5 4 0\n")
    (tmp_path / "quads.ply").write_text(text)
    v, c, f = read_ply_mesh(tmp_path / "quads.ply")
    assert c is None and np.array_equal(v, read_ply_points(tmp_path / "quads.ply")) and v[1].tolist() == [1, 0, 0]
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [3, 2, 5], [0, 1, 2], [0, 2, 5], [0, 5, 4], [1, 2, 5], [1, 5, 4]]
    # all quads: the one-table path
    quads = "ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 2\n" \
            "property list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n4 3 2 1 0\n"
    (tmp_path / "all_quads.ply").write_text(quads)
    assert read_ply_mesh(tmp_path / "all_quads.ply")[2].tolist() == [[0, 1, 2], [0, 2, 3], [3, 2, 1], [3, 1, 0]]
    # binary: a uint index list with an int count, doubles, an element between vertices and faces, mixed face sizes
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 50\nproperty double x\nproperty double y\nproperty double z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nelement edge 2\nproperty int a\nproperty int b\n"
            "element face 3\nproperty float quality\nproperty list int uint vertex_indices\nend_header\n")
    rec = np.zeros(50, dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    rec["x"], rec["y"], rec["z"], rec["r"], rec["g"], rec["b"] = *xyz.T, *rgb.T
    body = rec.tobytes() + np.array([[0, 1], [1, 2]], "<i4").tobytes()
    for quality, idx in ((0.5, [4, 5, 6]), (0.25, [7, 8, 9, 10]), (1.0, [49, 0, 2 ** 32 - 1])):
        body += np.array([quality], "<f4").tobytes() + np.array([len(idx)], "<i4").tobytes() + np.array(idx, "<u4").tobytes()
    (tmp_path / "uint.ply").write_bytes(head.encode() + body)
    v, c, f = read_ply_mesh(tmp_path / "uint.ply")
    assert np.array_equal(v, xyz) and np.array_equal(c, rgb)
    assert f.tolist() == [[4, 5, 6], [7, 8, 9], [7, 9, 10], [49, 0, -1]], "an index beyond int32 is -1: the sampler counts the face invalid"
    uniform = head.replace("element face 3", "element face 2")
    (tmp_path / "uint_uniform.ply").write_bytes(uniform.encode() + body[:len(rec.tobytes()) + 16 + 20] + body[-20:])
    assert read_ply_mesh(tmp_path / "uint_uniform.ply")[2].tolist() == [[4, 5, 6], [49, 0, -1]]
    # refusals name the file
    (tmp_path / "cut.ply").write_bytes((tmp_path / "own.ply").read_bytes()[:-5])
    (tmp_path / "cut_mixed.ply").write_bytes((tmp_path / "uint.ply").read_bytes()[:-3])
    (tmp_path / "cut_vertices.ply").write_bytes((tmp_path / "own.ply").read_bytes()[:400])
    (tmp_path / "cut_ascii.ply").write_text(text[:-8])
    (tmp_path / "float_index.ply").write_text(quads.replace("uchar int vertex_indices", "uchar float vertex_indices"))
    (tmp_path / "other_list.ply").write_text(quads.replace("vertex_indices", "texcoord"))
    (tmp_path / "two_corners.ply").write_text(text.replace("3 3 2 5 0", "2 3 2 0"))
    (tmp_path / "not_a.ply").write_bytes(b"solid mesh\n")
    for name, what in (("cut.ply", "truncated"), ("cut_mixed.ply", "truncated"), ("cut_vertices.ply", "truncated"), ("cut_ascii.ply", "truncated"),
                       ("float_index.ply", "integer"), ("other_list.ply", "vertex_indices"), ("two_corners.ply", "2 vertices"),
                       ("not_a.ply", "not a .ply")):
        with pytest.raises(SystemExit, match=what) as e:
            read_ply_mesh(tmp_path / name)
        assert name in str(e.value)


def crop_document(**changes):
    doc = {"axis_max": 4.5, "axis_min": -1.25, "bounding_polygon": [[0, 7, 0], [2, 7, 0.5], [2.5, 7, 3], [0.1, 7, 2]],
           "class_name": "SelectionPolygonVolume", "orthogonal_axis": "Y", "version_major": 1, "version_minor": 0}
    doc.update(changes)
    return {k: v for k, v in doc.items() if v is not ...}


def test_read_crop_file(tmp_path):
    from acezero_amd.formats import read_crop_file
    path = tmp_path / "crop.json"
    path.write_text(json.dumps(crop_document()))
    crop = read_crop_file(path)
    assert crop.axis == 1 and crop.polygon.dtype == F and crop.polygon.tolist() == [[0, 0], [2, 0.5], [2.5, 3], [F(0.1), 2]]
    assert crop.axis_min == F(-1.25) and crop.axis_max == F(4.5) and type(crop.axis_min) is F
    for axis, plane in (("x", [[7, 0], [7, 0.5], [7, 3], [7, 2]]), ("Z", [[0, 7], [2, 7], [2.5, 7], [F(0.1), 7]])):
        path.write_text(json.dumps(crop_document(orthogonal_axis=axis)))
        assert read_crop_file(path).polygon.tolist() == plane and read_crop_file(path).axis == "xyz".index(axis.lower())
    path.write_text(json.dumps(crop_document(class_name=..., axis_min=2, axis_max=2, comment="other keys are ignored")))
    assert read_crop_file(path).axis_min == read_crop_file(path).axis_max == 2
    refusals = [(dict(bounding_polygon=...), "bounding_polygon"), (dict(orthogonal_axis=...), "orthogonal_axis"), (dict(axis_min=...), "axis_min"),
                (dict(axis_max=...), "axis_max"), (dict(orthogonal_axis="W"), "orthogonal_axis"), (dict(orthogonal_axis=1), "orthogonal_axis"),
                (dict(axis_min=5.0), "axis_min"), (dict(axis_max="4"), "axis_max"), (dict(axis_min=float("nan")), "axis_min"),
                (dict(axis_max=float("inf")), "axis_max"), (dict(axis_max=1e39), "axis_max"), (dict(class_name="Box"), "class_name"),
                (dict(bounding_polygon=[[0, 0, 0], [1, 0, 0]]), "bounding_polygon"), (dict(bounding_polygon=[[0, 0, 0]] * 1025), "bounding_polygon"),
                (dict(bounding_polygon=[[0, 0, 0], [1, 0, 0], [1, 1]]), "bounding_polygon"),
                (dict(bounding_polygon=[[0, 0, 0], [1, 0, 0], [1, "a", 0]]), "bounding_polygon"),
                (dict(bounding_polygon=[[0, 0, 0], [1, 0, 0], [1, float("nan"), 0]]), "bounding_polygon"),
                (dict(bounding_polygon=[[0, 0, 0], [1, 0, 0], [1e39, 0, 1]]), "bounding_polygon"), (dict(bounding_polygon="polygon"), "bounding_polygon")]
    for changes, key in refusals:
        path.write_text(json.dumps(crop_document(**changes)))
        with pytest.raises(SystemExit, match=key) as e:
            read_crop_file(path)
        assert "crop.json" in str(e.value), changes
    path.write_text(json.dumps(crop_document(bounding_polygon=[[k, 0, k * k] for k in range(1024)])))
    assert read_crop_file(path).polygon.shape == (1024, 2)
    for text in ("[1, 2, 3]", "{not json"):
        path.write_text(text)
        with pytest.raises(SystemExit, match="crop.json"):
            read_crop_file(path)
    with pytest.raises(SystemExit, match="nowhere.json"):
        read_crop_file(tmp_path / "nowhere.json")


def test_crossing_rule_against_matplotlib():
    from matplotlib.path import Path
    rng = np.random.default_rng(5)
    for polygon in (SC.CONVEX, SC.L_SHAPE, SC.L_SHAPE[::-1], SC.star(64)):
        q = rng.uniform(-1.5, 1.5, (20000, 2)).astype(F)
        q = q[SR.edge_distance(q[:, 0], q[:, 1], polygon) > 1e-6]
        assert len(q) > 19000
        want = Path(polygon.astype(np.float64)).contains_points(q.astype(np.float64))
        assert 0.05 * len(q) < want.sum() < 0.95 * len(q)
        assert np.array_equal(want, SR.winding_inside(q[:, 0], q[:, 1], polygon))
        for axis in (0, 1, 2):
            iu, iv = {0: (1, 2), 1: (0, 2), 2: (0, 1)}[axis]
            p = np.zeros((len(q), 3), F)
            p[:, iu], p[:, iv], p[:, axis] = q[:, 0], q[:, 1], rng.uniform(-1, 1, len(q))
            got = SR.crop_keep(p, polygon, axis, -0.5, 0.5)
            assert np.array_equal(got, want & (p[:, axis] >= F(-0.5)) & (p[:, axis] <= F(0.5))), axis


def test_crossing_rule_is_half_open():
    """Two polygons that share an edge: a point of their union's interior, on the shared edge and at its ends included, is in exactly
    one of them; an edge along u never counts; the axis bounds are closed; points that are not finite are outside."""
    left = np.array([[0, 0], [0.5, 0], [0.5, 1], [0, 1]], F)
    right = np.array([[0.5, 0], [1, 0], [1, 1], [0.5, 1]], F)
    top = np.array([[0, 1], [1, 1], [1, 2], [0, 2]], F)
    g = np.arange(0, 17, dtype=F) / F(8)                           # 0, 1/8 .. 2: on the corners, on the edges, inside
    u, v = [a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij")]
    p = np.stack([u, v, np.zeros_like(u)], 1)
    inside = [SR.crop_keep(p, poly, 2, 0.0, 0.0) for poly in (left, right, top)]
    total = inside[0].astype(int) + inside[1] + inside[2]
    union = SR.crop_keep(p, np.array([[0, 0], [1, 0], [1, 2], [0, 2]], F), 2, 0.0, 0.0)
    assert np.array_equal(total, union.astype(int)) and union.sum() == 8 * 16, "u in [0, 1), v in [0, 2)"
    assert inside[0][(u == 0) & (v == 0)].all() and not union[(u == 1) | (v == 2)].any()
    for name, (pts, polygon, axis, lo, hi) in SC.crop_cases().items():
        keep = SR.crop_keep(pts, polygon, axis, lo, hi)
        assert not keep[~np.isfinite(pts).all(1)].any(), name
        if len(pts) >= 63:
            rows = 2 * min(len(polygon), 8)
            w = pts[rows:rows + 4, axis]
            assert w[0] == F(lo) and w[1] == F(hi) and keep[rows:rows + 2].all() and not keep[rows + 2:rows + 4].any(), name
            assert 0 < keep.sum() < len(pts)


def test_host_tensors_are_refused_and_the_functions_are_exported():
    from acezero_amd import geometry as G
    from acezero_amd.formats import CropVolume
    assert {"sample_mesh", "crop_to_polygon"} <= set(G.__all__)
    v, f = SC.box_room()
    crop = CropVolume(SC.TRIANGLE, 2, F(0), F(1))
    for call in (lambda: G.sample_mesh(torch.from_numpy(v), torch.from_numpy(f), spacing=0.1),
                 lambda: G.crop_to_polygon(torch.from_numpy(v), crop)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    for spacing in (0.0, -1.0, float("nan"), float("inf"), 1e-200):
        with pytest.raises(ValueError, match="spacing"):
            G.sample_density(spacing)
    assert G.sample_density(0.005) == SR.density_of(0.005) == 1.0 / (0.005 * 0.005)


def test_argument_validation_without_device():
    from acezero_amd import _native as N
    lib = N.lib()
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data                                          # never dereferenced: every call below is refused before any launch

    def refused(rc, text):
        assert rc == -1 and text in lib.acez_last_error(), (rc, lib.acez_last_error())

    def counts(v=p, m=10, f=p, k=10, density=100.0, seed=0, out=p, areas=p):
        return lib.acez_geom_face_counts(v, m, f, k, density, seed, out, areas, None)

    def sample(v=p, m=10, f=p, k=10, off=p, n=10, seed=0, col=None, pts=p, face=p, out_col=None):
        return lib.acez_geom_sample_faces(v, m, f, k, off, n, seed, col, pts, face, out_col, None)

    def crop(pts=p, n=10, poly=p, corners=4, axis=1, lo=0.0, hi=1.0, keep=p):
        return lib.acez_geom_crop_polygon(pts, n, poly, corners, axis, lo, hi, keep, None)

    for name in ("v", "f", "out", "areas"):
        refused(counts(**{name: None}), b"null pointer")
    for kw in (dict(m=-1), dict(k=-1), dict(m=2 ** 31), dict(k=2 ** 31)):
        refused(counts(**kw), b"count")
    for density in (0.0, -1.0, float("nan"), float("inf")):
        refused(counts(density=density), b"density")
    for name in ("v", "f", "off", "pts", "face"):
        refused(sample(**{name: None}), b"null pointer")
    for kw in (dict(m=-1), dict(k=-1), dict(n=-1), dict(m=2 ** 31), dict(k=2 ** 31), dict(n=2 ** 31)):
        refused(sample(**kw), b"count")
    refused(sample(m=0), b"without vertices")
    refused(sample(k=0), b"without vertices")
    refused(sample(col=p), b"go together")
    refused(sample(out_col=p), b"go together")
    for name in ("pts", "poly", "keep"):
        refused(crop(**{name: None}), b"null pointer")
    refused(crop(n=-1), b"count")
    refused(crop(n=2 ** 31), b"count")
    refused(crop(corners=2), b"corners")
    refused(crop(corners=1025), b"corners")
    refused(crop(axis=-1), b"axis")
    refused(crop(axis=3), b"axis")
    refused(crop(lo=1.0, hi=0.5), b"bounds")
    refused(crop(lo=float("nan")), b"bounds")
    refused(crop(hi=float("inf")), b"bounds")
    if not torch.cuda.is_available():                            # what is valid gets as far as the device check, and no further
        for rc in (counts(), counts(k=0, f=None, out=None, areas=None), sample(), sample(col=p, out_col=p), sample(n=0, pts=None, face=None),
                   crop(), crop(lo=0.5, hi=0.5), crop(n=0, pts=None, keep=None)):
            assert rc == -3 and b"no HIP device" in lib.acez_last_error()


def test_cli_refusals(tmp_path):
    from acezero_amd import cli
    from acezero_amd.formats import write_ply
    pts = GC.uniform(1, 20)
    cloud, mesh, crop = str(tmp_path / "cloud.ply"), str(tmp_path / "mesh.ply"), str(tmp_path / "crop.json")
    write_ply(cloud, pts, np.zeros((20, 3), np.uint8))
    write_ply(mesh, pts, np.zeros((20, 3), np.uint8), np.arange(18, dtype=np.int32).reshape(6, 3))
    (tmp_path / "crop.json").write_text(json.dumps(crop_document()))
    (tmp_path / "bad.json").write_text(json.dumps(crop_document(orthogonal_axis="Q")))
    opt = cli.eval_geometry_parser().parse_args([mesh, cloud])
    assert opt.sample_spacing is None and opt.gt_sample_spacing is None and opt.sample_seed == 0 and opt.write_samples is None
    assert opt.crop_file is None and opt.crop_file_ground_truth is False
    for flag in ("--sample_spacing", "--gt_sample_spacing"):
        for value in ("0", "-0.01", "nan", "inf", "1e-200"):
            with pytest.raises(SystemExit, match=f"{flag} must be positive"):
                cli.eval_geometry_main([mesh, mesh, flag, value])
    with pytest.raises(SystemExit, match="cloud.ply: --sample_spacing needs a mesh") as e:
        cli.eval_geometry_main([cloud, mesh, "--sample_spacing", "0.01"])
    assert "no faces" in str(e.value)
    with pytest.raises(SystemExit, match="cloud.ply: --gt_sample_spacing needs a mesh"):
        cli.eval_geometry_main([mesh, cloud, "--sample_spacing", "0.01", "--gt_sample_spacing", "0.01"])
    with pytest.raises(SystemExit, match="--write_samples needs --sample_spacing"):
        cli.eval_geometry_main([mesh, cloud, "--write_samples", str(tmp_path / "s.ply")])
    with pytest.raises(SystemExit, match="--crop_file_ground_truth needs --crop_file"):
        cli.eval_geometry_main([mesh, cloud, "--crop_file_ground_truth", "True"])
    with pytest.raises(SystemExit, match="missing.json: no such file"):
        cli.eval_geometry_main([mesh, cloud, "--crop_file", str(tmp_path / "missing.json")])
    with pytest.raises(SystemExit, match="bad.json: orthogonal_axis"):
        cli.eval_geometry_main([mesh, cloud, "--crop_file", str(tmp_path / "bad.json")])
    if not torch.cuda.is_available():                            # valid options get as far as the device check
        with pytest.raises(SystemExit, match="needs a GPU"):
            cli.eval_geometry_main([mesh, cloud, "--sample_spacing", "0.01", "--crop_file", crop, "--write_samples", str(tmp_path / "s.ply")])
