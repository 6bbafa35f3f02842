"""CPU: the DEFINITION of the mesh simplification (include/acez.h section Q) checked on its host restatement
(tests/simplify_restated.py), so that the kernels' bit-for-bit parity with it (tests/test_simplify_gpu.py) means something: the host
instantiation of the placement (acezero_amd/csrc/simplify_solve.h, through tests/simplify_probe.hip) against the restated one bit for
bit, the restatement against a brute-force dictionary formulation on the soup, and what the simplified cube, sphere and fused sphere
look like; then what needs no device: the parsers, simplify_mesh.py's refusals and the entry points' argument checks.

The measured figures below were printed by this file's tests from the restatement and are asserted at 1.25 x the measured deviation
(DESIGN.md section 4p); the kernels equal the restatement bit for bit, so the margin absorbs a later change of the shapes only."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from acezero_amd import _native as N
from acezero_amd import cli, simplify
from tests import fusion_cases as FC
from tests import simplify_cases as SC
from tests import simplify_restated as SR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
MARGIN = 1.25

# measured with the restatement (test output); see DESIGN.md section 4p
CUBE_QUADRIC_OFF_SURFACE = 0.0                   # m: every vertex of the quadric placement lies on the cube, to the last bit of fp32
CUBE_MEAN_OFF_SURFACE = 0.035472973              # m, the contrast: the mean placement cuts the edges and corners
SPHERE_RADIUS_BELOW, SPHERE_RADIUS_ABOVE = 1.262e-8, 4.717578e-4         # m below and above SC.SPHERE_R, quadric placement
SPHERE_VOLUME_DEFICIT = 3.1473370e-3             # 1 - volume / (4/3 pi r^3), quadric placement
FUSED_OPEN_EDGES = 0
FUSED_VOLUME_EXCESS = 3.5128726e-3               # volume / (4/3 pi r^3) - 1, quadric placement at a cell of three voxels


@functools.lru_cache(maxsize=None)
def restated(name, placement, with_colours=True):
    """The restated result of a case of SC.cases(), computed once; tests/test_simplify_gpu.py shares it. Read-only."""
    v, c, f, cell = SC.cases()[name]
    out = SR.simplify_mesh(v, c if with_colours else None, f, cell, placement)
    for a in out[:3]:
        if a is not None:
            a.setflags(write=False)
    return out


# --------------------------------------------------------------------------------------------------------------- the solve
@pytest.fixture(scope="module")
def probe():
    so = os.path.join(HERE, "_build", "libsimplify_probe.so")
    src = os.path.join(HERE, "simplify_probe.hip")
    deps = [src] + [os.path.join(ROOT, "acezero_amd", "csrc", f) for f in ("simplify_solve.h", "svd3.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                        "-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.probe_simplify_solve.restype = C.c_int
    lib.probe_simplify_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    lib.probe_simplify_add_corner.restype = None
    lib.probe_simplify_add_corner.argtypes = [C.c_void_p] * 4
    lib.probe_svd3.restype = None
    lib.probe_svd3.argtypes = [C.c_void_p] * 4
    return lib


def _p(a):
    return a.ctypes.data


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def planes_quadric(rng, normals, through, faces_per_plane=4, spread=0.04):
    """The nine sums of triangles lying in the planes with the given normals through the point `through`, by the restated terms."""
    q = np.zeros(9)
    for n in normals:
        n = np.asarray(n, np.float64) / np.linalg.norm(n)
        t1 = np.cross(n, [0.3, -0.8, 0.5])
        t1 /= np.linalg.norm(t1)
        t2 = np.cross(n, t1)
        for _ in range(faces_per_plane):
            uv = rng.uniform(-spread, spread, (3, 2))
            a, b, c = (np.asarray(through) + uv[i, 0] * t1 + uv[i, 1] * t2 for i in range(3))
            q = q + SR.corner_terms(a[None], b[None], c[None])[0]
    return q


def solve_cases():
    """name -> (q, mean, cell, solved, rank): walls, edges, corners, nothing, and a corner outside the cell."""
    rng = np.random.default_rng(31)
    x, y, z, tilt = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.6, 0.1, 0.79]
    inside, cell = [0.011, -0.02, 0.007], 0.05
    mean = np.array([0.004, 0.013, -0.009])
    out = {}
    for i in range(6):
        out[f"rank1_{i}"] = (planes_quadric(rng, [tilt if i % 2 else z], inside), mean + rng.uniform(-0.01, 0.01, 3), cell, True, 1)
        out[f"rank2_{i}"] = (planes_quadric(rng, [x, tilt] if i % 2 else [y, z], inside), mean + rng.uniform(-0.01, 0.01, 3), cell, True, 2)
        out[f"rank3_{i}"] = (planes_quadric(rng, [x, y, tilt] if i % 2 else [x, y, z], inside), mean + rng.uniform(-0.01, 0.01, 3), cell, True, 3)
    out["zero"] = (np.zeros(9), mean, cell, False, 0)
    out["corner_outside_the_cell"] = (planes_quadric(rng, [x, y, z], [0.2, 0.01, 0.0]), mean, cell, False, 3)
    out["wall_outside_the_cell"] = (planes_quadric(rng, [z], [0.0, 0.0, 0.0501]), mean, cell, False, 1)
    out["not_finite"] = (np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0, np.inf, 0.0, 0.0]), mean, cell, False, 3)
    out["not_a_number"] = (np.full(9, np.nan), mean, cell, False, 0)
    return out


@pytest.mark.parametrize("name", sorted(solve_cases()))
def test_host_solve_is_the_restated_solve_bit_for_bit(probe, name):
    q, mean, cell, solved, rank = solve_cases()[name]
    q, mean = np.ascontiguousarray(q, np.float64), np.ascontiguousarray(mean, np.float64)
    want_solved, want = SR.solve(q, mean, cell)
    x = np.full(3, -7.0)
    got_solved = probe.probe_simplify_solve(_p(q), _p(mean), cell, _p(x))
    assert bool(got_solved) == want_solved == solved
    assert np.array_equal(bits(x), bits(np.array(want, np.float64)))
    if not solved:
        assert np.array_equal(bits(x), bits(mean))                                  # a fallback is the mean itself
        return
    A = np.array([[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]])
    s = np.linalg.svd(A, compute_uv=False)
    assert int((s > SR.RANK_RATIO * s[0]).sum()) == rank
    # the minimiser property on the kept directions, and no movement along the others
    _, v, sv = SR.svd3(A.reshape(-1))
    gradient = A @ x + q[6:]
    for i in range(3):
        if sv[i] > SR.RANK_RATIO * sv[0]:
            assert abs(np.dot(v[i], gradient)) <= 1e-9 * sv[0] * cell
        else:
            assert abs(np.dot(v[i], x - mean)) <= 1e-12


def test_host_svd3_and_corner_terms_are_the_restated_ones_bit_for_bit(probe):
    rng = np.random.default_rng(32)
    matrices = [rng.normal(size=9) for _ in range(20)] + [np.zeros(9), np.eye(3).reshape(-1), np.outer([1.0, 2.0, -1.0], [1.0, 2.0, -1.0]).reshape(-1)]
    for name, (q, _, _, _, _) in solve_cases().items():
        if np.isfinite(q).all():
            matrices.append(np.array([q[0], q[1], q[2], q[1], q[3], q[4], q[2], q[4], q[5]]))
    for Cm in matrices:
        Cm = np.ascontiguousarray(Cm, np.float64)
        u, v, s = np.zeros(9), np.zeros(9), np.zeros(3)
        probe.probe_svd3(_p(Cm), _p(u), _p(v), _p(s))
        wu, wv, ws = SR.svd3([float(t) for t in Cm])
        assert np.array_equal(bits(u), bits(np.array(wu).reshape(-1))) and np.array_equal(bits(v), bits(np.array(wv).reshape(-1)))
        assert np.array_equal(bits(s), bits(np.array(ws)))
    q, want = np.zeros(9), np.zeros(9)
    for _ in range(50):
        a, b, c = (np.ascontiguousarray(rng.uniform(-0.1, 0.1, 3)) for _ in range(3))
        probe.probe_simplify_add_corner(_p(a), _p(b), _p(c), _p(q))
        want = want + SR.corner_terms(a[None], b[None], c[None])[0]
        assert np.array_equal(bits(q), bits(want))


# ------------------------------------------------------------------------------------------------------------- brute force
def brute_force(vertices, colours, faces, cell):
    """Section Q with dictionaries and loops, the mean placement: (vertices, colours, faces, counts)."""
    v, m, cell = np.asarray(vertices, F), len(vertices), F(cell)
    finite = [i for i in range(m) if np.isfinite(v[i]).all()]
    origin = v[finite].min(0)
    cells = {}
    for i in finite:
        cells.setdefault(tuple(int(t) for t in np.floor((v[i] - origin) / cell))[::-1], []).append(i)           # (z, y, x): the key's order
    occupied = sorted(cells)
    cluster_of = {i: c for c, cell_index in enumerate(occupied) for i in cells[cell_index]}
    seen, out, counts = {}, [], dict(invalid=0, degenerate=0, collapsed=0, duplicate=0)
    for a, b, c in np.asarray(faces).tolist():
        if not all(0 <= t < m for t in (a, b, c)):
            counts["invalid"] += 1
        elif len({a, b, c}) < 3:
            counts["degenerate"] += 1
        elif not all(t in cluster_of for t in (a, b, c)):
            counts["invalid"] += 1
        else:
            tri = [cluster_of[a], cluster_of[b], cluster_of[c]]
            if len(set(tri)) < 3:
                counts["collapsed"] += 1
                continue
            at = tri.index(min(tri))
            tri = tuple(tri[at:] + tri[:at])
            if tri in seen:
                counts["duplicate"] += 1
            else:
                seen[tri] = True
                out.append(tri)
    used = sorted({c for tri in out for c in tri})
    rename = {c: i for i, c in enumerate(used)}
    points, rgb = [], []
    for c in used:
        members = cells[occupied[c]]
        total = np.zeros(3)
        for i in members:
            total = total + v[i].astype(np.float64)
        points.append((total / float(len(members))).astype(F))
        channel = np.asarray(colours)[members].astype(np.int64).sum(0)
        rgb.append((2 * channel + len(members)) // (2 * len(members)))
    return np.array(points, F), np.array(rgb, np.uint8), np.array([[rename[c] for c in tri] for tri in out], np.int32), counts, len(occupied)


def test_restatement_is_the_brute_force_formulation_on_the_soup():
    v, c, f, cell = SC.soup()
    want_v, want_c, want_f, counts, n_clusters = brute_force(v, c, f, cell)
    got_v, got_c, got_f, info = restated("soup", "mean")
    assert np.array_equal(got_f, want_f) and np.array_equal(got_c, want_c)
    assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32))
    assert info == dict(clusters=n_clusters, vertices_in=len(v), faces_in=len(f), vertices_out=len(want_v), faces_out=len(want_f),
                        invalid_faces=counts["invalid"], degenerate_faces=counts["degenerate"], nonfinite_vertices=2,
                        collapsed_faces=counts["collapsed"], duplicate_faces=counts["duplicate"], unused_clusters=n_clusters - len(want_v), fallbacks=0)
    # the soup holds what it was built to hold, and the counts add up
    assert info["invalid_faces"] >= 4 and info["degenerate_faces"] >= 2 and info["duplicate_faces"] >= 3 and info["collapsed_faces"] > 0
    assert info["unused_clusters"] >= 1
    assert info["faces_in"] == sum(info[key] for key in ("invalid_faces", "degenerate_faces", "collapsed_faces", "duplicate_faces", "faces_out"))
    assert (got_f[:, 0] < got_f[:, 1]).all() and (got_f[:, 0] < got_f[:, 2]).all()                 # the smallest id first
    # the quadric placement differs in nothing but the positions
    quadric = restated("soup", "quadric")
    assert np.array_equal(quadric[2], got_f) and np.array_equal(quadric[1], got_c) and quadric[0].shape == got_v.shape
    assert {k: t for k, t in quadric[3].items() if k != "fallbacks"} == {k: t for k, t in info.items() if k != "fallbacks"}
    bare = restated("soup", "quadric", with_colours=False)
    assert bare[1] is None and np.array_equal(bare[0].view(np.uint32), quadric[0].view(np.uint32)) and np.array_equal(bare[2], quadric[2])


# -------------------------------------------------------------------------------------------------------------- the shapes
def test_the_cases_are_what_they_claim():
    v, _, f = SC.cube()
    assert (len(v), len(f)) == (6146, 12288) and SC.closedness(f) == (0, 0, 0) and abs(FC.signed_volume(v, f) - 1.0) < 1e-6
    assert SC.cube_distance(v).max() < 1e-7
    v, _, f = SC.sphere()
    assert (len(v), len(f)) == (4514, 9024) and SC.closedness(f) == (0, 0, 0) and FC.signed_volume(v, f) > 0
    v, _, f, cell = SC.cone()
    _, vertex_cluster, _ = SR.clusters(v, cell)
    _, _, valid, mapped = SR.classify(f, vertex_cluster)
    assert valid.all() and np.bincount(mapped.reshape(-1)).max() == 200 > 64 * 3              # the apex's cluster
    v, _, f, cell = SC.one_triangle()
    assert np.bincount(SR.classify(f, SR.clusters(v, cell)[1])[3].reshape(-1)).tolist() == [1, 1, 1]


@pytest.mark.parametrize("name", ["cube_0.1", "cube_0.13"])
def test_cube_keeps_its_edges_and_corners(name):
    v, _, f, info = restated(name, "quadric")
    assert SC.closedness(f) == (0, 0, 0) and info["fallbacks"] == 0 and info["unused_clusters"] == 0
    off = float(SC.cube_distance(v).max())
    volume = FC.signed_volume(v, f)
    mv, _, mf, minfo = restated(name, "mean")
    mean_off = float(SC.cube_distance(mv).max())
    print(f"{name}: {info['vertices_in']} vertices, {info['faces_in']} faces -> {info['vertices_out']}, {info['faces_out']}; quadric: off the "
          f"surface by at most {off:.9g} m, volume {volume:.9f}; mean: {mean_off:.9g} m, volume {FC.signed_volume(mv, mf):.9f}")
    assert off <= MARGIN * CUBE_QUADRIC_OFF_SURFACE and abs(volume - 1.0) < 1e-6
    assert SC.closedness(mf) == (0, 0, 0) and np.array_equal(mf, f) and minfo["fallbacks"] == 0
    if name == "cube_0.1":
        assert (info["vertices_out"], info["faces_out"]) == (602, 1200)
        assert CUBE_MEAN_OFF_SURFACE / MARGIN <= mean_off <= MARGIN * CUBE_MEAN_OFF_SURFACE      # the contrast is there, and is this size


def test_sphere_stays_closed_and_round():
    v, _, f, info = restated("sphere_0.03", "quadric")
    assert SC.closedness(f) == (0, 0, 0) and info["fallbacks"] == 0
    radius = np.linalg.norm(v.astype(np.float64), axis=1)
    exact = 4.0 / 3.0 * np.pi * SC.SPHERE_R ** 3
    deficit = 1.0 - FC.signed_volume(v, f) / exact
    print(f"sphere: {info['vertices_in']} vertices, {info['faces_in']} faces -> {info['vertices_out']}, {info['faces_out']}; radii "
          f"{radius.min():.10f} .. {radius.max():.10f} (below {SC.SPHERE_R - radius.min():.4g}, above {radius.max() - SC.SPHERE_R:.7g}), volume "
          f"deficit {deficit:.8g}")
    assert SC.SPHERE_R - radius.min() <= MARGIN * SPHERE_RADIUS_BELOW and radius.max() - SC.SPHERE_R <= MARGIN * SPHERE_RADIUS_ABOVE
    assert 0.0 < deficit <= MARGIN * SPHERE_VOLUME_DEFICIT
    mv, _, mf, minfo = restated("sphere_0.03", "mean")
    assert SC.closedness(mf) == (0, 0, 0) and minfo["fallbacks"] == 0 and np.array_equal(mf, f)
    assert np.linalg.norm(mv.astype(np.float64), axis=1).max() <= SC.SPHERE_R + 2e-8             # a mean of points of a ball lies in it


def test_fused_sphere_at_three_voxels():
    """The surface-net sphere of tests/fusion_cases.py (voxel 0.02) at a cell of 0.06: no edge is left open; some edges of the
    simplified mesh carry more than two faces (thin cells fold), which is recorded, not tuned away."""
    from tests.test_fusion_cpu import sphere_mesh
    v, c, f = sphere_mesh()
    assert len(v) == 4458
    out_v, out_c, out_f, info = SR.simplify_mesh(v, c, f, F(3 * FC.SPHERE_VOLUME["voxel_size"]), "quadric")
    open_edges, crowded, repeated = SC.closedness(out_f)
    exact = 4.0 / 3.0 * np.pi * FC.SPHERE_R ** 3
    excess = FC.signed_volume(out_v, out_f) / exact - 1.0
    print(f"fused sphere: {len(v)} vertices, {len(f)} faces (volume {FC.signed_volume(v, f) / exact - 1.0:+.4%}) -> {info['vertices_out']}, "
          f"{info['faces_out']}: {open_edges} open edges, {crowded} edges with more than two faces, {repeated} directed edges repeated, "
          f"{info['fallbacks']} fallbacks, volume {excess:+.8g}")
    assert open_edges <= FUSED_OPEN_EDGES
    assert abs(excess) <= MARGIN * FUSED_VOLUME_EXCESS
    assert len(out_c) == len(out_v) == info["vertices_out"] < len(v) // 8 and info["faces_out"] < len(f) // 8


# ---------------------------------------------------------------------------------------------- parsers, refusals, arguments
def test_parser_defaults_and_module_surface():
    opt = cli.simplify_mesh_parser().parse_args(["in.ply", "out.ply", "--cell", "0.03"])
    assert (opt.cell, opt.placement) == (0.03, "quadric")
    assert cli.simplify_mesh_parser().parse_args(["in.ply", "out.ply", "--cell", "0.03", "--placement", "mean"]).placement == "mean"
    with pytest.raises(SystemExit):
        cli.simplify_mesh_parser().parse_args(["in.ply", "out.ply"])                              # --cell is required
    with pytest.raises(SystemExit):
        cli.simplify_mesh_parser().parse_args(["in.ply", "out.ply", "--cell", "0.03", "--placement", "median"])
    opt = cli.fuse_depth_parser().parse_args(["poses.txt", "*.png", "out.ply", "--depth_files", "*.png"])
    assert (opt.simplify_cell, opt.simplify_placement) == (None, "quadric")
    opt = cli.fuse_depth_parser().parse_args(["poses.txt", "*.png", "out.ply", "--depth_files", "*.png", "--simplify_cell", "0.06",
                                              "--simplify_placement", "mean"])
    assert (opt.simplify_cell, opt.simplify_placement) == (0.06, "mean")
    assert simplify.__all__ == ["simplify_mesh"]
    assert sorted(restated("one_triangle", "mean")[3]) == sorted(
        ["clusters", "vertices_in", "faces_in", "vertices_out", "faces_out", "invalid_faces", "degenerate_faces", "nonfinite_vertices",
         "collapsed_faces", "duplicate_faces", "unused_clusters", "fallbacks"])


def test_simplify_mesh_refusals(tmp_path):
    from acezero_amd.formats import write_ply
    v, c, f, _ = SC.one_triangle()
    write_ply(tmp_path / "in.ply", v, c, f)
    with pytest.raises(SystemExit, match="use .ply"):
        cli.simplify_mesh_main([str(tmp_path / "in.ply"), str(tmp_path / "out.obj"), "--cell", "0.1"])
    with pytest.raises(SystemExit, match="no such file"):
        cli.simplify_mesh_main([str(tmp_path / "missing.ply"), str(tmp_path / "out.ply"), "--cell", "0.1"])
    for bad in ("0", "-0.1", "nan", "inf"):
        with pytest.raises(SystemExit, match="--cell must be positive and finite"):
            cli.simplify_mesh_main([str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), "--cell", bad])
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match="needs a GPU.*no CPU path"):
            cli.simplify_mesh_main([str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), "--cell", "0.1"])
    assert not (tmp_path / "out.obj").exists()
    with pytest.raises(RuntimeError, match="no CPU path"):
        simplify.simplify_mesh(torch.from_numpy(v), None, torch.from_numpy(f), 0.1)


def entry_point_calls(lib, p):
    """name -> call(**overrides) for the six entry points; p: a buffer pointer."""
    def keys(vertices=p, m=8, origin=(0.0, 0.0, 0.0), top=(1.0, 1.0, 1.0), cell=0.1, out=p):
        return lib.acez_simplify_keys(vertices, m, *origin, *top, cell, out, None)

    def clusters(order=p, cluster_sorted=p, m=8, vertex_cluster=p):
        return lib.acez_simplify_clusters(order, cluster_sorted, m, vertex_cluster, None)

    def faces(faces=p, k=4, vertex_cluster=p, m=8, face_class=p, triples=p, corner_keys=p):
        return lib.acez_simplify_faces(faces, k, vertex_cluster, m, face_class, triples, corner_keys, None)

    def quadrics(vertices=p, m=8, faces=p, k=4, sorted_keys=p, segments=p, corner_order=p, corner_segments=p, origin=(0.0, 0.0, 0.0), cell=0.1,
                 out=p):
        return lib.acez_simplify_quadrics(vertices, m, faces, k, sorted_keys, segments, corner_order, corner_segments, *origin, cell, out, None)

    def place(vertices=p, colours=None, m=8, sorted_keys=p, order=p, segments=p, quadrics=p, origin=(0.0, 0.0, 0.0), cell=0.1, out_v=p,
              out_c=None, out_fallback=p):
        return lib.acez_simplify_place(vertices, colours, m, sorted_keys, order, segments, quadrics, *origin, cell, out_v, out_c, out_fallback, None)

    def unique(triples=p, face_class=p, perm=p, k=4, m=8, face_keep=p, cluster_used=p):
        return lib.acez_simplify_unique(triples, face_class, perm, k, m, face_keep, cluster_used, None)

    return dict(keys=keys, clusters=clusters, faces=faces, quadrics=quadrics, place=place, unique=unique)


POINTERS = dict(keys=("vertices", "out"), clusters=("order", "cluster_sorted", "vertex_cluster"),
                faces=("faces", "vertex_cluster", "face_class", "triples", "corner_keys"),
                quadrics=("vertices", "faces", "sorted_keys", "segments", "corner_order", "corner_segments", "out"),
                place=("vertices", "sorted_keys", "order", "segments", "out_v", "out_fallback"),           # quadrics may be null: the mean
                unique=("triples", "face_class", "perm", "face_keep", "cluster_used"))


def check_refusals(lib, calls, p):
    """What every entry point refuses before it launches anything; shared with the device test. p: a buffer pointer."""
    def refused(rc, text):
        assert rc == -1 and text in lib.acez_last_error(), (rc, lib.acez_last_error())

    for name, call in calls.items():
        for arg in POINTERS[name]:
            refused(call(**{arg: None}), b"null pointer")
        refused(call(m=-1), b"out of range")
        refused(call(m=2 ** 31), b"out of range")
        if "k" in call.__code__.co_varnames:
            refused(call(k=-1), b"out of range")
            refused(call(k=2 ** 31), b"out of range")
    for cell in (0.0, -0.1, float("nan"), float("inf")):
        refused(calls["keys"](cell=cell), b"positive and finite")
        refused(calls["place"](cell=cell), b"positive and finite")
        refused(calls["quadrics"](cell=cell), b"positive and finite")
    refused(calls["keys"](origin=(0.0, float("nan"), 0.0)), b"bounds finite")
    refused(calls["keys"](top=(1.0, 1.0, float("inf"))), b"bounds finite")
    refused(calls["keys"](origin=(0.0, 2.0, 0.0)), b"ordered")
    refused(calls["place"](origin=(float("inf"), 0.0, 0.0)), b"origin finite")
    refused(calls["quadrics"](origin=(0.0, 0.0, float("nan"))), b"origin finite")
    # 2^21 cells on an axis are one too many: the last index is floor(top / cell)
    cell = float(F(2.0 ** -10))
    refused(calls["keys"](top=(1.0, 2.0 ** 11 - 2.0 ** -10, 1.0), cell=cell), b"fewer than 2^21 cells")
    refused(calls["keys"](top=(1.0, 1.0, 1.0), cell=1e-30), b"fewer than 2^21 cells")
    refused(calls["place"](colours=p), b"go together")
    refused(calls["place"](out_c=p), b"go together")


def test_argument_validation_without_device():
    lib = N.lib()
    buffer = np.zeros(256, np.int64)
    calls = entry_point_calls(lib, buffer.ctypes.data)
    check_refusals(lib, calls, buffer.ctypes.data)
    if not torch.cuda.is_available():                                              # host pointers: refused for want of a device
        for name, call in calls.items():
            assert call() == -3 and b"no HIP device" in lib.acez_last_error(), name
        cell = float(F(2.0 ** -10))
        assert calls["keys"](top=(1.0, 2.0 ** 11 - 2.0 ** -9, 1.0), cell=cell) == -3  # 2^21 - 1 cells on an axis are allowed
        assert calls["keys"](vertices=None, out=None, m=0) == -3                   # an array of count 0 may be null
        assert calls["place"](quadrics=None) == -3                                  # the mean placement
        assert calls["quadrics"](faces=None, corner_order=None, k=0) == -3
        assert calls["unique"](triples=None, face_class=None, perm=None, face_keep=None, k=0) == -3
    assert not buffer.any()
