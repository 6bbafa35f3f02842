"""GPU: the mesh clean-up kernels (acezero_amd/csrc/mesh_api.hip) against the host restatement of include/acez.h section P
(tests/mesh_restated.py), integer for integer: the labels, the counts, the filtered mesh; then clean_mesh.py and fuse_depth.py's
three flags end to end. The restated labels are computed once (tests/test_mesh_cpu.py: restated) and shared."""
import numpy as np
import pytest
import torch

from acezero_amd import _native as N
from acezero_amd import mesh
from acezero_amd.head import _ptr
from tests import fusion_cases as FC
from tests import mesh_cases as MC
from tests import mesh_restated as MR
from tests.helpers import assert_file_is, device, run
from tests.test_mesh_cpu import check_refusals, entry_point_calls, restated

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(MC.label_cases()))
def test_labels_and_counts_match_the_restatement(name):
    faces, m = MC.label_cases()[name]
    want_labels, want_faces_of, want_vertices_of = restated(name)
    d_faces = device(faces)
    labels = mesh.connected_components(d_faces, m)
    assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), want_labels)
    faces_of, vertices_of = mesh.component_sizes(d_faces, labels)
    assert np.array_equal(faces_of.cpu().numpy(), want_faces_of) and np.array_equal(vertices_of.cpu().numpy(), want_vertices_of)
    # the entry point itself: the status word is cleared and stays 0, whatever it held
    raw, status = torch.full((max(m, 1),), -7, dtype=torch.int32, device="cuda"), torch.full((1,), 5, dtype=torch.int32, device="cuda")
    assert N.lib().acez_mesh_components(_ptr(d_faces), len(faces), m, _ptr(raw), _ptr(status), None) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and np.array_equal(raw.cpu().numpy()[:m], want_labels)
    # another order of the face rows: the same labels
    order = np.random.default_rng(17).permutation(len(faces))
    assert np.array_equal(mesh.connected_components(device(faces[order]), m).cpu().numpy(), want_labels)


CRITERIA = {"none": {}, "min_faces": dict(min_faces=3), "min_ratio": dict(min_ratio=0.1), "keep_largest": dict(keep_largest=3),
            "all": dict(min_faces=2, min_ratio=0.5, keep_largest=4)}


@pytest.mark.parametrize("criteria", sorted(CRITERIA))
@pytest.mark.parametrize("name", ["messy", "ties", "ratios", "tetrahedra_apart", "islands", "sphere_floater", "empty", "no_faces"])
def test_filter_matches_the_restatement(name, criteria):
    faces, m = MC.label_cases()[name]
    v, c = MC.attributes(m)
    kw = CRITERIA[criteria]
    want_v, want_c, want_f, want_info = MR.filter_components(v, c, faces, **kw)
    got_v, got_c, got_f, info = mesh.filter_components(device(v), device(c), device(faces), **kw)
    assert got_v.dtype == torch.float32 and got_c.dtype == torch.uint8 and got_f.dtype == torch.int32
    assert np.array_equal(got_v.cpu().numpy().view(np.uint32), want_v.view(np.uint32))
    assert np.array_equal(got_c.cpu().numpy(), want_c) and np.array_equal(got_f.cpu().numpy(), want_f)
    assert info == want_info
    bare_v, bare_c, bare_f, bare_info = mesh.filter_components(device(v), None, device(faces), **kw)      # a mesh without colours
    assert bare_c is None and torch.equal(bare_v.view(torch.int32), got_v.view(torch.int32)) and torch.equal(bare_f, got_f) and bare_info == info


def test_keep_largest_on_the_sphere_with_a_floater():
    v, c, f, n_sphere = MC.sphere_with_floater()
    got_v, got_c, got_f, info = mesh.filter_components(device(v), device(c), device(f), keep_largest=1)
    used = np.unique(f[:n_sphere])
    assert np.array_equal(got_v.cpu().numpy().view(np.uint32), v[used].view(np.uint32))
    assert np.array_equal(got_v.cpu().numpy()[got_f.cpu().numpy()], v[f[:n_sphere]])
    assert info["components_kept"] == 1 and info["faces_dropped"] == 40 and info["largest_component_faces"] == n_sphere


def test_argument_validation_with_device_buffers():
    lib = N.lib()
    ints, bytes_ = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
    calls = entry_point_calls(lib, ints.data_ptr(), bytes_.data_ptr())
    check_refusals(lib, calls)
    assert calls["compact"](colours=bytes_.data_ptr()) == -1 and b"go together" in lib.acez_last_error()
    with pytest.raises(N.AcezError, match="ACEZ_ERR_INVALID"):
        N.check(calls["select"](k=-1))
    torch.cuda.synchronize()                                     # nothing was launched by the refused calls; the device is fine
    assert int(ints.abs().sum().item()) == 0 and int(bytes_.sum().item()) == 0
    # counts of 0 with null arrays are served without a launch
    status = torch.ones(1, dtype=torch.int32, device="cuda")
    assert lib.acez_mesh_components(None, 0, 0, None, _ptr(status), None) == 0
    assert lib.acez_mesh_component_counts(None, 0, None, 0, None, None, None) == 0
    assert lib.acez_mesh_select(None, 0, None, 0, None, None, None, None) == 0
    assert lib.acez_mesh_compact(None, None, 0, None, 0, None, None, None, None, None, None, 0, None, 0, None) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0


def test_clean_mesh_end_to_end(tmp_path):
    from acezero_amd.formats import write_ply
    v, _, f, n_sphere = MC.sphere_with_floater()
    c = MC.attributes(len(v))[1]
    f = np.concatenate([f[:50], np.array([[0, 0, 1], [-1, 2, 3]], np.int32), f[50:]], 0)       # a degenerate and an invalid face on the way
    write_ply(tmp_path / "in.ply", v, c, f)
    log = run("clean_mesh.py", [tmp_path / "in.ply", tmp_path / "out.ply", "--keep_largest", "1"])
    assert_file_is(tmp_path / "out.ply", MR.filter_components(*FC.read_mesh_ply(tmp_path / "in.ply"), keep_largest=1))
    assert len(FC.read_mesh_ply(tmp_path / "out.ply")[2]) == n_sphere
    assert "connected components" in log and "kept 1" in log and "1 degenerate" in log and "1 with an index out of range" in log
    log = run("clean_mesh.py", [tmp_path / "in.ply", tmp_path / "plain.ply"])                   # no criterion: says so, drops the bad rows
    assert "No criterion given" in log
    assert_file_is(tmp_path / "plain.ply", MR.filter_components(v, c, f))
    log = run("clean_mesh.py", [tmp_path / "in.ply", tmp_path / "nothing.ply", "--min_component_faces", "1000000"])
    assert "Nothing is left" in log
    got = FC.read_mesh_ply(tmp_path / "nothing.ply")
    assert got[0].shape == (0, 3) and got[2].shape == (0, 3)


@pytest.mark.parametrize("sparse", ["False", "True"])
def test_fuse_depth_drops_the_floater(tmp_path, sparse):
    """The scene of tests/test_mesh_cpu.py::test_the_fused_room_has_its_floater."""
    args = MC.write_room_with_floater(tmp_path) + ["--sparse", sparse]
    args[2] = str(tmp_path / "all.ply")
    log = run("fuse_depth.py", args)
    assert "connected components" not in log                                                   # the filter is off by default
    whole = FC.read_mesh_ply(args[2])
    faces_of = MR.sizes(whole[2], MR.labels(whole[2], len(whole[0])))[0]
    found = sorted(faces_of[faces_of > 0].tolist())
    print(f"components of the unfiltered mesh: {found}")
    assert len(found) > 1 and found[-2] < MC.ROOM_MIN_FACES <= found[-1]
    args[2] = str(tmp_path / "room.ply")
    log = run("fuse_depth.py", args + ["--min_component_faces", str(MC.ROOM_MIN_FACES)])
    assert f"{len(found)} connected components" in log and "kept 1" in log
    assert_file_is(args[2], MR.filter_components(*whole, min_faces=MC.ROOM_MIN_FACES))
    room = FC.read_mesh_ply(args[2])
    faces_of = MR.sizes(room[2], MR.labels(room[2], len(room[0])))[0]
    assert int((faces_of > 0).sum()) == 1 and int(faces_of.max()) == found[-1] == len(room[2])
