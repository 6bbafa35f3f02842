"""CPU: the DEFINITION of the mesh clean-up (include/acez.h section P) checked on its host restatement (tests/mesh_restated.py), so
that the kernels' integer-for-integer parity with it (tests/test_mesh_gpu.py) means something: its labels against scipy's connected
components, the selection rules on hand-made cases, the filter on a sphere with a floater; then what needs no device: the parsers,
clean_mesh.py's refusals, the entry points' argument checks, and that the fused room of the GPU test has the floater it is about."""
import functools

import numpy as np
import pytest
import torch

from acezero_amd import _native as N
from acezero_amd import cli, mesh
from tests import mesh_cases as MC
from tests import mesh_restated as MR


@functools.lru_cache(maxsize=None)
def restated(name):
    """(labels, faces_of, vertices_of) of a case, computed once; tests/test_mesh_gpu.py shares it. Read-only."""
    faces, m = MC.label_cases()[name]
    lab = MR.labels(faces, m)
    out = (lab,) + MR.sizes(faces, lab)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", sorted(MC.label_cases()))
def test_restated_labels_are_scipys_components(name):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    faces, m = MC.label_cases()[name]
    lab, faces_of, vertices_of = restated(name)
    assert lab.shape == (m,) and lab.dtype == np.int32
    if m == 0:
        return
    valid, _, _ = MR.classify(faces, m)
    f = faces[valid].astype(np.int64)
    rows, cols = np.concatenate([f[:, 0], f[:, 1], f[:, 0]]), np.concatenate([f[:, 1], f[:, 2], f[:, 2]])
    n, part = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(m, m)), directed=False)
    smallest = np.full(n, m, np.int64)
    np.minimum.at(smallest, part, np.arange(m))
    assert np.array_equal(lab, smallest[part])                                 # the same partition, every label its part's minimum
    in_face = np.zeros(m, bool)
    in_face[f.reshape(-1)] = True
    assert np.array_equal(lab[~in_face], np.arange(m)[~in_face])
    assert int(faces_of.sum()) == len(f) and int(vertices_of.sum()) == int(in_face.sum())
    assert np.array_equal(faces_of > 0, vertices_of > 0) and (lab[faces_of > 0] == np.flatnonzero(faces_of > 0)).all()


def test_definition_on_the_hand_made_cases():
    lab, faces_of, vertices_of = restated("messy")
    assert sorted(np.flatnonzero(faces_of).tolist()) == [2, 3] and faces_of[2] == 3 and faces_of[3] == 1
    assert vertices_of[2] == 5 and vertices_of[3] == 3 and lab[5] == 2 and lab[19] == 3 and lab[9] == 9 and lab[0] == 0
    _, invalid, degenerate = MR.classify(*MC.messy())
    assert int(invalid.sum()) == 4 and int(degenerate.sum()) == 4
    assert restated("tetrahedra_apart")[1].tolist() == [4, 0, 0, 0, 4, 0, 0, 0]
    assert restated("tetrahedra_touching")[1].tolist() == [8, 0, 0, 0, 0, 0, 0] and restated("tetrahedra_touching")[2][0] == 7
    assert restated("islands")[1].max() == 2 and int((restated("islands")[1] > 0).sum()) == 30_000


def test_selection_rules():
    faces_of = restated("ties")[1]
    kept = lambda **kw: np.flatnonzero(MR.select(faces_of, **kw)).tolist()      # noqa: E731
    assert kept() == [0, 2, 6, 10, 14, 20]
    assert kept(keep_largest=1) == [2]                                         # two components of 4 faces: the smaller label
    assert kept(keep_largest=3) == [2, 6, 10]                                  # three of 2 faces: again the smallest label
    assert kept(keep_largest=0) == [] and kept(keep_largest=6) == kept(keep_largest=99) == kept()
    assert kept(min_faces=2) == [2, 6, 10, 14, 20] and kept(min_faces=3) == [2, 10] and kept(min_faces=5) == []
    assert kept(min_ratio=0.5) == [2, 6, 10, 14, 20] and kept(min_ratio=0.51) == [2, 10] and kept(min_ratio=1.0) == [2, 10]
    assert kept(min_faces=2, keep_largest=4, min_ratio=0.5) == [2, 6, 10, 14]   # conjunctive
    assert kept(min_faces=3, keep_largest=1) == [2] and kept(min_faces=5, keep_largest=1) == []
    faces_of = restated("ratios")[1]
    sizes = lambda **kw: sorted(faces_of[MR.select(faces_of, **kw)].tolist())   # noqa: E731
    assert sizes() == [9, 10, 50, 100]
    assert sizes(min_ratio=0.1) == [10, 50, 100] and sizes(min_ratio=0.1000001) == [50, 100] and sizes(min_ratio=0.09) == [9, 10, 50, 100]
    assert sizes(min_ratio=0.1, keep_largest=2) == [50, 100] and sizes(min_ratio=0.1, min_faces=11, keep_largest=3) == [50, 100]


def test_filter_keeps_the_sphere_and_drops_the_floater():
    v, c, f, n_sphere = MC.sphere_with_floater()
    out_v, out_c, out_f, info = MR.filter_components(v, c, f, keep_largest=1)
    used = np.unique(f[:n_sphere])
    assert np.array_equal(out_v.view(np.uint32), v[used].view(np.uint32)) and np.array_equal(out_c, c[used])
    assert np.array_equal(out_v[out_f], v[f[:n_sphere]])                         # the sphere's faces, in their order, on the same points
    assert info["components_kept"] == 1 and info["components"] >= 2 and info["faces_dropped"] == 40
    assert info["largest_component_faces"] == n_sphere and info["vertices_dropped"] == len(v) - len(used)
    same = MR.filter_components(v, c, f)                                         # no criterion: only the unreferenced vertices go
    assert len(same[2]) == len(f) and np.array_equal(same[0][same[2]], v[f]) and same[3]["vertices_dropped"] == len(v) - len(np.unique(f))
    messy_f, m = MC.messy()
    mv, mc = MC.attributes(m)
    out_v, out_c, out_f, info = MR.filter_components(mv, mc, messy_f, min_faces=2)
    assert out_f.tolist() == [[1, 2, 3], [2, 3, 4], [0, 4, 1]] and np.array_equal(out_c, mc[[2, 5, 7, 11, 13]])
    assert info == dict(components=2, components_kept=1, faces_dropped=9, vertices_dropped=15, largest_component_faces=3, invalid_faces=4,
                        degenerate_faces=4, size_histogram=[2, 0, 0, 0, 0])


def test_parser_defaults_leave_the_filter_off():
    opt = cli.fuse_depth_parser().parse_args(["poses.txt", "*.png", "out.ply", "--depth_files", "*.png"])
    assert (opt.min_component_faces, opt.min_component_ratio, opt.keep_largest) == (0, 0.0, None)
    assert cli._component_criteria(opt) is None
    opt = cli.clean_mesh_parser().parse_args(["in.ply", "out.ply"])
    assert (opt.min_component_faces, opt.min_component_ratio, opt.keep_largest) == (0, 0.0, None) and cli._component_criteria(opt) is None
    opt = cli.clean_mesh_parser().parse_args(["in.ply", "out.ply", "--min_component_faces", "50", "--keep_largest", "2"])
    assert cli._component_criteria(opt) == dict(min_faces=50, min_ratio=0.0, keep_largest=2)
    opt = cli.fuse_depth_parser().parse_args(["poses.txt", "*.png", "out.ply", "--depth_files", "*.png", "--min_component_ratio", "0.05"])
    assert cli._component_criteria(opt) == dict(min_faces=0, min_ratio=0.05, keep_largest=None)
    for bad in (["--min_component_faces", "-1"], ["--min_component_ratio", "1.5"], ["--min_component_ratio", "nan"], ["--keep_largest", "0"]):
        with pytest.raises(SystemExit, match="min_component"):
            cli._component_criteria(cli.clean_mesh_parser().parse_args(["in.ply", "out.ply"] + bad))


def test_clean_mesh_refusals(tmp_path):
    from acezero_amd.formats import write_ply
    faces, m = MC.two_tetrahedra(False)
    v, c = MC.attributes(m)
    write_ply(tmp_path / "in.ply", v, c, faces)
    with pytest.raises(SystemExit, match="use .ply"):
        cli.clean_mesh_main([str(tmp_path / "in.ply"), str(tmp_path / "out.obj")])
    with pytest.raises(SystemExit, match="no such file"):
        cli.clean_mesh_main([str(tmp_path / "missing.ply"), str(tmp_path / "out.ply")])
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match="needs a GPU.*no CPU path"):
            cli.clean_mesh_main([str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), "--keep_largest", "1"])
    assert not (tmp_path / "out.obj").exists()


def test_host_tensors_are_refused():
    faces = torch.from_numpy(MC.two_tetrahedra(False)[0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.connected_components(faces, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.component_sizes(faces, torch.zeros(8, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.filter_components(torch.zeros(8, 3), None, faces, keep_largest=1)
    assert sorted(mesh.__all__) == ["component_sizes", "connected_components", "filter_components"]


def entry_point_calls(lib, p, b):
    """name -> call(**overrides) for the four entry points; p: an int32 / float buffer pointer, b: a byte buffer pointer."""
    def components(faces=p, k=4, m=8, labels=p, status=p):
        return lib.acez_mesh_components(faces, k, m, labels, status, None)

    def counts(faces=p, k=4, labels=p, m=8, faces_of=p, vertices_of=p):
        return lib.acez_mesh_component_counts(faces, k, labels, m, faces_of, vertices_of, None)

    def select(faces=p, k=4, labels=p, m=8, keep=b, face_keep=b, used=b):
        return lib.acez_mesh_select(faces, k, labels, m, keep, face_keep, used, None)

    def compact(vertices=p, colours=None, m=8, faces=p, k=4, face_keep=b, face_rank=p, used=b, vertex_rank=p, out_v=p, out_c=None, n_v=8,
                out_f=p, n_f=4):
        return lib.acez_mesh_compact(vertices, colours, m, faces, k, face_keep, face_rank, used, vertex_rank, out_v, out_c, n_v, out_f, n_f, None)

    return dict(components=components, counts=counts, select=select, compact=compact)


def check_refusals(lib, calls):
    """What every entry point refuses before it launches anything; shared with the device test."""
    def refused(rc, text):
        assert rc == -1 and text in lib.acez_last_error(), (rc, lib.acez_last_error())

    for name, call in calls.items():
        for arg in ("faces", "labels") if name != "compact" else ("faces", "vertices", "face_keep", "face_rank", "used", "vertex_rank", "out_v", "out_f"):
            refused(call(**{arg: None}), b"null pointer")
        refused(call(k=-1), b"out of range")
        refused(call(m=-1), b"out of range")
        refused(call(k=2 ** 31), b"out of range")
        refused(call(m=2 ** 31), b"out of range")
    refused(calls["components"](status=None), b"null pointer")
    refused(calls["components"](status=None, k=0, m=0), b"null pointer")
    refused(calls["counts"](faces_of=None), b"null pointer")
    refused(calls["counts"](vertices_of=None), b"null pointer")
    for arg in ("keep", "face_keep", "used"):
        refused(calls["select"](**{arg: None}), b"null pointer")
    refused(calls["compact"](n_v=9), b"more output rows")
    refused(calls["compact"](n_f=5), b"more output rows")
    refused(calls["compact"](n_f=-1), b"more output rows")


def test_argument_validation_without_device():
    lib = N.lib()
    ints, bytes_ = np.zeros(64, np.int32), np.zeros(64, np.uint8)
    p, b = ints.ctypes.data, bytes_.ctypes.data
    calls = entry_point_calls(lib, p, b)
    check_refusals(lib, calls)
    refused = lambda rc, text: (rc, text in lib.acez_last_error()) == (-1, True)   # noqa: E731
    assert refused(calls["compact"](colours=b), b"go together") and refused(calls["compact"](out_c=b), b"go together")
    if not torch.cuda.is_available():                                              # host pointers: refused for want of a device
        for name, call in calls.items():
            assert call() == -3 and b"no HIP device" in lib.acez_last_error(), name
        assert calls["components"](faces=None, k=0, labels=None, m=0) == -3        # an array of count 0 may be null
        assert calls["compact"](out_v=None, n_v=0, out_f=None, n_f=0) == -3


def test_the_fused_room_has_its_floater(tmp_path):
    """The precondition of the GPU test of fuse_depth.py's flags: by the host restatement of the fusion, the scene's mesh is the room
    and one floater of at least 8 faces and at most a tenth of the room's, so --min_component_faces MC.ROOM_MIN_FACES separates them."""
    v, _, f = MC.restated_room_mesh(MC.write_room_with_floater(tmp_path))
    faces_of = MR.sizes(f, MR.labels(f, len(v)))[0]
    room, *rest = sorted(faces_of[faces_of > 0].tolist(), reverse=True)
    print(f"room {room} faces, other components {rest}")
    assert len(rest) == 1 and 8 <= rest[0] <= room // 10
    assert rest[0] < MC.ROOM_MIN_FACES <= room // 4
