"""GPU: what mesh.filter_components and simplify.simplify_mesh say to a mesh they refuse, and what they return for one without
vertices or faces, message for message and key for key: both go through mesh.check_mesh and mesh.empty_mesh, and the order of their
checks differs. The mesh is one triangle; nothing here but the sample_mesh call at the end launches a kernel."""
import pytest
import torch

from acezero_amd import geometry, mesh, simplify

pytestmark = pytest.mark.gpu

CALLS = {"filter_components": (lambda v, c, f: mesh.filter_components(v, c, f), "mesh components are HIP kernels"),
         "simplify_mesh": (lambda v, c, f: simplify.simplify_mesh(v, c, f, cell=0.1), "the simplification is HIP kernels")}


def triangle(**changed):
    """vertices, colours, faces of the one triangle on the device, `changed` in their place."""
    parts = dict(vertices=torch.eye(3, device="cuda"), colours=torch.full((3, 3), 7, dtype=torch.uint8, device="cuda"),
                 faces=torch.tensor([[0, 1, 2]], dtype=torch.int32, device="cuda"))
    parts.update(changed)
    return parts["vertices"], parts["colours"], parts["faces"]


def no_cpu(what, why):
    return RuntimeError, f"{what} needs device tensors: {why}, there is no CPU path"


# name -> (what is changed, the exception and its message given the function's name and its reason)
REFUSED = {
    "int64_faces": (lambda: dict(faces=torch.tensor([[0, 1, 2]], device="cuda")),
                    lambda what, why: (ValueError, f"{what}: expected int32 faces [k,3], got torch.int64 (1, 3)")),
    "faces_1x4": (lambda: dict(faces=torch.zeros((1, 4), dtype=torch.int32, device="cuda")),
                  lambda what, why: (ValueError, f"{what}: expected int32 faces [k,3], got torch.int32 (1, 4)")),
    "float64_vertices": (lambda: dict(vertices=torch.eye(3, dtype=torch.float64, device="cuda")),
                         lambda what, why: (ValueError, f"{what}: expected float32 vertices [m,3], got torch.float64 (3, 3)")),
    "vertices_3x2": (lambda: dict(vertices=torch.zeros((3, 2), device="cuda")),
                     lambda what, why: (ValueError, f"{what}: expected float32 vertices [m,3], got torch.float32 (3, 2)")),
    "int32_colours": (lambda: dict(colours=torch.zeros((3, 3), dtype=torch.int32, device="cuda")),
                      lambda what, why: (ValueError, f"{what}: expected uint8 colours (3, 3), got torch.int32 (3, 3)")),
    "colours_2x3": (lambda: dict(colours=torch.zeros((2, 3), dtype=torch.uint8, device="cuda")),
                    lambda what, why: (ValueError, f"{what}: expected uint8 colours (3, 3), got torch.uint8 (2, 3)")),
    "host_vertices": (lambda: dict(vertices=torch.eye(3)), no_cpu),
    "host_colours": (lambda: dict(colours=torch.zeros((3, 3), dtype=torch.uint8)), no_cpu),
    # two rules at once: the faces' type wins over the vertices' and the colours'
    "int64_faces_float64_vertices_int32_colours": (
        lambda: dict(faces=torch.tensor([[0, 1, 2]], device="cuda"), vertices=torch.eye(3, dtype=torch.float64, device="cuda"),
                     colours=torch.zeros((3, 3), dtype=torch.int32, device="cuda")),
        lambda what, why: (ValueError, f"{what}: expected int32 faces [k,3], got torch.int64 (1, 3)")),
    # .. and here the two functions differ: filter_components looks at the faces before it asks where the vertices live, simplify_mesh
    # asks where everything lives first
    "int64_faces_host_vertices": (
        lambda: dict(faces=torch.tensor([[0, 1, 2]], device="cuda"), vertices=torch.eye(3)),
        lambda what, why: (ValueError, f"{what}: expected int32 faces [k,3], got torch.int64 (1, 3)") if what == "filter_components" else no_cpu(what, why)),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
@pytest.mark.parametrize("what", sorted(CALLS))
def test_refusals_word_for_word(what, case):
    function, why = CALLS[what]
    changed, expected = REFUSED[case]
    kind, message = expected(what, why)
    with pytest.raises(kind) as caught:
        function(*triangle(**changed()))
    assert type(caught.value) is kind and str(caught.value) == message


def assert_empty(got, with_colours):
    vertices, colours, faces = got
    assert vertices.is_cuda and vertices.dtype == torch.float32 and tuple(vertices.shape) == (0, 3)
    assert faces.is_cuda and faces.dtype == torch.int32 and tuple(faces.shape) == (0, 3)
    if with_colours:
        assert colours.is_cuda and colours.dtype == torch.uint8 and tuple(colours.shape) == (0, 3)
    else:
        assert colours is None


@pytest.mark.parametrize("with_colours", [True, False], ids=["colours", "bare"])
def test_meshes_without_vertices_or_faces(with_colours):
    _, _, faces = triangle()
    no_vertices = torch.empty((0, 3), device="cuda")
    no_colours = torch.empty((0, 3), dtype=torch.uint8, device="cuda") if with_colours else None
    *got, info = mesh.filter_components(no_vertices, no_colours, faces)                                   # m == 0: the face is invalid
    assert_empty(got, with_colours)
    assert info == dict(components=0, components_kept=0, faces_dropped=1, vertices_dropped=0, largest_component_faces=0, invalid_faces=1,
                        degenerate_faces=0, size_histogram=[0, 0, 0, 0, 0])
    vertices, colours, _ = triangle()
    *got, info = mesh.filter_components(vertices, colours if with_colours else None, torch.empty((0, 3), dtype=torch.int32, device="cuda"))   # k == 0
    assert_empty(got, with_colours)
    assert info == dict(components=0, components_kept=0, faces_dropped=0, vertices_dropped=3, largest_component_faces=0, invalid_faces=0,
                        degenerate_faces=0, size_histogram=[0, 0, 0, 0, 0])
    *got, info = simplify.simplify_mesh(no_vertices, no_colours, faces, cell=0.1)                         # m == 0
    assert_empty(got, with_colours)
    assert info == dict(clusters=0, vertices_in=0, faces_in=1, vertices_out=0, faces_out=0, invalid_faces=1, degenerate_faces=0,
                        nonfinite_vertices=0, collapsed_faces=0, duplicate_faces=0, unused_clusters=0, fallbacks=0)


def test_sample_mesh_still_converts_what_the_others_refuse():
    vertices, colours, faces = triangle()
    want = geometry.sample_mesh(vertices, faces, spacing=0.25, seed=3, colours=colours)
    got = geometry.sample_mesh(vertices.double(), faces.long(), spacing=0.25, seed=3, colours=colours)
    assert want[3]["samples"] > 0 and got[3] == want[3]
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
