"""GPU: the mesh simplification kernels (acezero_amd/csrc/simplify_api.hip) against the host restatement of include/acez.h section Q
(tests/simplify_restated.py), bit for bit in vertices and colours, integer for integer in faces and info; then simplify_mesh.py and
fuse_depth.py --simplify_cell end to end. The restated results are computed once (tests/test_simplify_cpu.py: restated) and shared."""
import numpy as np
import pytest
import torch

from acezero_amd import _native as N
from acezero_amd import cli, simplify
from tests import fusion_cases as FC
from tests import mesh_cases as MC
from tests import mesh_restated as MR
from tests import simplify_cases as SC
from tests import simplify_restated as SR
from tests.helpers import assert_file_is, call, device, host, run
from tests.test_simplify_cpu import check_refusals, entry_point_calls, restated

pytestmark = pytest.mark.gpu


def assert_same(got, want):
    got_v, got_c, got_f, got_info = got
    want_v, want_c, want_f, want_info = want
    assert got_info == want_info
    assert got_v.dtype == torch.float32 and got_f.dtype == torch.int32 and tuple(got_v.shape) == want_v.shape and tuple(got_f.shape) == want_f.shape
    assert np.array_equal(host(got_f), want_f)
    differ = np.flatnonzero((host(got_v).view(np.uint32) != want_v.view(np.uint32)).any(1))
    assert len(differ) == 0, (len(differ), host(got_v)[differ[:3]], want_v[differ[:3]])
    if want_c is None:
        assert got_c is None
    else:
        assert got_c.dtype == torch.uint8 and np.array_equal(host(got_c), want_c)


@pytest.mark.parametrize("with_colours", [True, False], ids=["colours", "bare"])
@pytest.mark.parametrize("placement", ["quadric", "mean"])
@pytest.mark.parametrize("name", sorted(SC.cases()))
def test_simplify_matches_the_restatement(name, placement, with_colours):
    v, c, f, cell = SC.cases()[name]
    got = simplify.simplify_mesh(device(v), device(c) if with_colours else None, device(f), float(cell), placement)
    assert_same(got, restated(name, placement, with_colours))


def test_two_calls_give_the_same_bytes():
    v, c, f, cell = SC.cases()["sphere_0.03"]
    d_v, d_c, d_f = device(v), device(c), device(f)
    first = simplify.simplify_mesh(d_v, d_c, d_f, float(cell))
    second = simplify.simplify_mesh(d_v, d_c, d_f, float(cell))
    assert first[3] == second[3]
    for a, b in zip(first[:3], second[:3]):
        assert host(a).tobytes() == host(b).tobytes()
    assert np.array_equal(host(d_v).view(np.uint32), v.view(np.uint32)) and np.array_equal(host(d_f), f)        # the input is not touched


def test_argument_validation_with_device_buffers():
    lib = N.lib()
    buffer = torch.zeros(256, dtype=torch.int64, device="cuda")
    calls = entry_point_calls(lib, buffer.data_ptr())
    check_refusals(lib, calls, buffer.data_ptr())
    torch.cuda.synchronize()                                     # nothing was launched by the refused calls; the device is fine
    assert int(buffer.abs().sum().item()) == 0
    # counts of 0 with null arrays are served without a launch
    assert calls["keys"](vertices=None, out=None, m=0) == 0
    assert calls["clusters"](order=None, cluster_sorted=None, vertex_cluster=None, m=0) == 0
    assert calls["faces"](faces=None, face_class=None, triples=None, corner_keys=None, k=0, vertex_cluster=None, m=0) == 0
    assert calls["quadrics"](vertices=None, faces=None, sorted_keys=None, segments=None, corner_order=None, corner_segments=None, out=None, m=0,
                             k=0) == 0
    assert calls["place"](vertices=None, sorted_keys=None, order=None, segments=None, quadrics=None, out_v=None, out_fallback=None, m=0) == 0
    assert calls["unique"](triples=None, face_class=None, perm=None, face_keep=None, cluster_used=None, k=0, m=0) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="cell must be positive"):
        simplify.simplify_mesh(torch.zeros((3, 3), device="cuda"), None, torch.zeros((1, 3), dtype=torch.int32, device="cuda"), 0.0)
    with pytest.raises(ValueError, match="placement"):
        simplify.simplify_mesh(torch.zeros((3, 3), device="cuda"), None, torch.zeros((1, 3), dtype=torch.int32, device="cuda"), 0.1, "median")
    with pytest.raises(N.AcezError, match="ACEZ_ERR_INVALID.*2\\^21"):                             # 1 m at a cell of 0.1 um
        simplify.simplify_mesh(torch.eye(3, device="cuda"), None, torch.zeros((1, 3), dtype=torch.int32, device="cuda"), 1e-7)


def test_simplify_mesh_end_to_end(tmp_path, caplog):
    from acezero_amd.formats import write_ply
    v, c, f, cell = SC.soup()
    v = np.where(np.isfinite(v), v, np.float32(0.5))            # the file keeps what it is given, but a NaN in a .ply helps nobody
    write_ply(tmp_path / "in.ply", v, c, f)
    log = run("simplify_mesh.py", [tmp_path / "in.ply", tmp_path / "out.ply", "--cell", float(cell)])          # the command itself, once
    want = SR.simplify_mesh(*FC.read_mesh_ply(tmp_path / "in.ply"), cell, "quadric")
    assert_file_is(tmp_path / "out.ply", want)
    assert f"{want[3]['faces_out']} faces left" in log and f"in {want[3]['clusters']} cells" in log and "(quadric)" in log
    call(cli.simplify_mesh_main, [tmp_path / "in.ply", tmp_path / "mean.ply", "--cell", float(cell), "--placement", "mean"], caplog)
    assert_file_is(tmp_path / "mean.ply", SR.simplify_mesh(v, c, f, cell, "mean"))
    log = call(cli.simplify_mesh_main, [tmp_path / "in.ply", tmp_path / "nothing.ply", "--cell", "10"], caplog)
    assert "Nothing is left" in log
    got = FC.read_mesh_ply(tmp_path / "nothing.ply")
    assert got[0].shape == (0, 3) and got[2].shape == (0, 3)


def test_fuse_depth_simplify_cell(tmp_path, caplog):
    """The room of tests/test_mesh_gpu.py. Without the flag the file is the one the restated fusion gives, as it always was; with the
    flag it is simplify_mesh.py applied to that file, byte for byte; with the component flags too, the filter comes first."""
    args = MC.write_room_with_floater(tmp_path)
    args[2] = str(tmp_path / "plain.ply")
    log = call(cli.fuse_depth_main, args, caplog)
    assert "Simplified" not in log                                                               # off by default
    plain = FC.read_mesh_ply(args[2])
    want = MC.restated_room_mesh(args)
    assert np.array_equal(plain[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(plain[2], want[2])
    args[2] = str(tmp_path / "small.ply")
    log = call(cli.fuse_depth_main, args + ["--simplify_cell", "0.06"], caplog)
    assert "Simplified at a cell of 0.06 m (quadric)" in log
    call(cli.simplify_mesh_main, [tmp_path / "plain.ply", tmp_path / "again.ply", "--cell", "0.06"], caplog)
    assert open(tmp_path / "small.ply", "rb").read() == open(tmp_path / "again.ply", "rb").read()
    small = FC.read_mesh_ply(tmp_path / "small.ply")
    assert_file_is(tmp_path / "small.ply", SR.simplify_mesh(*plain, np.float32(0.06), "quadric"))
    assert 0 < len(small[2]) < len(plain[2]) // 4
    args[2] = str(tmp_path / "both.ply")
    call(cli.fuse_depth_main, args + ["--min_component_faces", str(MC.ROOM_MIN_FACES), "--simplify_cell", "0.06", "--simplify_placement", "mean"], caplog)
    room = MR.filter_components(*plain, min_faces=MC.ROOM_MIN_FACES)[:3]
    assert len(room[2]) < len(plain[2])
    assert_file_is(tmp_path / "both.ply", SR.simplify_mesh(*room, np.float32(0.06), "mean"))
