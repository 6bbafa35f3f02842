"""Meshes for the component tests (tests/test_mesh_cpu.py, tests/test_mesh_gpu.py): shapes at which a parallel union-find can go
wrong (long chains, many roots, every face on one root), the definition's corner cases, and a fused scene with a floating fragment.
A helper module, not a test file. A case is (faces int32 [k,3], m); its vertices and colours, where a test needs them, come from
attributes(m)."""
import functools
import os

import numpy as np

INT32_MAX = 2 ** 31 - 1
TETRAHEDRON = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]], np.int32)


def strip(k, order):
    """A triangle strip of k faces over k + 2 vertices, the vertex ids along it ascending, descending or in a seeded random order."""
    m = k + 2
    ids = {"ascending": np.arange(m), "descending": np.arange(m)[::-1], "random": np.random.default_rng(11).permutation(m)}[order]
    i = np.arange(k)
    return ids[np.stack([i, i + 1, i + 2], 1)].astype(np.int32), m


def islands(n):
    """n islands of two triangles over four vertices each, the vertex ids shuffled."""
    ids = np.random.default_rng(12).permutation(4 * n)
    base = 4 * np.arange(n)[:, None]
    quads = np.concatenate([base + np.array([[0, 1, 2]]), base + np.array([[1, 3, 2]])], 0)
    return ids[quads].astype(np.int32), 4 * n


def fan(k, hub_last):
    """k faces around one vertex, the one with the largest id (every link meets at a root that keeps moving) or id 0."""
    m = k + 2
    i = np.arange(k)
    if hub_last:
        return np.stack([np.full(k, m - 1), i, i + 1], 1).astype(np.int32), m
    return np.stack([np.zeros(k, np.int64), i + 1, i + 2], 1).astype(np.int32), m


def two_tetrahedra(shared):
    """Two closed tetrahedra: without a common vertex (two components of 4 faces), or with exactly one (one component of 8)."""
    second = TETRAHEDRON + (3 if shared else 4)
    return np.concatenate([TETRAHEDRON, second], 0).astype(np.int32), 7 if shared else 8


def messy():
    """Valid faces between faces with indices out of range (-1, m, INT32_MAX), degenerate faces and vertices that nothing references.
    m = 20: a component {2, 5, 7, 11, 13} of 3 faces, a component {3, 4, 19} of 1 face, and a bridge that only bad faces would build."""
    m = 20
    faces = np.array([[5, 7, 11], [-1, 5, 3], [7, 11, 13], [3, 4, 19], [5, 5, 3], [2, 13, 5], [3, m, 5], [19, 3, 19], [INT32_MAX, 0, 1],
                      [4, 7, 7], [0, 1, -2 ** 31], [9, 9, 9]], np.int32)
    return faces, m


def ties():
    """Components of 4, 4, 2, 2, 2 and 1 faces whose labels do not ascend with their first appearance: the order among equal counts is
    by label. Labels: tetrahedron 10 (ids 10..13), tetrahedron 2 (ids 2..5), pairs 20, 6, 14, a triangle 0 (ids 0, 1, 24)."""
    pair = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    faces = np.concatenate([TETRAHEDRON + 10, pair + 20, TETRAHEDRON + 2, np.array([[24, 1, 0]], np.int32), pair + 6, pair + 14], 0)
    return faces.astype(np.int32), 26


def ratios():
    """Fans of 100, 50, 10 and 9 faces: min_ratio 0.1 keeps three of them, and 10 >= 0.1 * 100 holds in fp64."""
    parts, at = [], 0
    for k in (10, 100, 9, 50):
        f, m = fan(k, hub_last=False)
        parts.append(f + at)
        at += m
    return np.concatenate(parts, 0).astype(np.int32), at + 3                        # three unreferenced vertices at the end


def empty(m=0):
    return np.zeros((0, 3), np.int32), m


@functools.lru_cache(maxsize=None)
def sphere_with_floater():
    """(vertices, colours, faces, number of the sphere's faces): the fused sphere of tests/fusion_cases.py (its extraction may emit
    vertices that no face uses), and after it a copy of 40 of its faces, scaled and shifted away from it, on vertices of their own."""
    from tests.test_fusion_cpu import sphere_mesh
    v, c, f = sphere_mesh()
    part = f[100:140]
    old = np.unique(part)
    v2 = (v[old] * np.float32(0.2) + np.array([0.6, 0.1, -0.2], np.float32)).astype(np.float32)
    f2 = (np.searchsorted(old, part) + len(v)).astype(np.int32)
    return np.concatenate([v, v2], 0), np.concatenate([c, c[old]], 0), np.concatenate([f, f2], 0).astype(np.int32), len(f)


def label_cases():
    """name -> (faces, m): every case the labels and the counts are compared on."""
    sv, _, sf, _ = sphere_with_floater()
    return {
        "strip_ascending": strip(200_000, "ascending"), "strip_descending": strip(200_000, "descending"),
        "strip_random": strip(200_000, "random"), "islands": islands(30_000), "fan_last": fan(100_000, True),
        "fan_first": fan(100_000, False), "tetrahedra_apart": two_tetrahedra(False), "tetrahedra_touching": two_tetrahedra(True),
        "messy": messy(), "ties": ties(), "ratios": ratios(), "empty": empty(), "no_faces": empty(5), "sphere_floater": (sf, len(sv)),
    }


def attributes(m, seed=13):
    """(vertices float32 [m,3], colours uint8 [m,3]): random bit patterns, NaNs and infinities among them; a filter only moves them."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2 ** 32, (m, 3), dtype=np.uint64).astype(np.uint32).view(np.float32), rng.integers(0, 256, (m, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ a fused room with a floater
ROOM = dict(frames=6, h=120, w=160, focal=100.0, frame=1, patch=40, patch_mm=350)
ROOM_FLAGS = ["--min_weight", "1"]
ROOM_MIN_FACES = 1000        # between the floater's face count and the room's: tests/test_mesh_cpu.py asserts it


def write_room_with_floater(folder):
    """fuse_depth.py's arguments for the box room of tests/fusion_cases.py, six frames 60 degrees apart, in which one frame's depth
    image has a square of near depth (0.35 m) written into its centre: a surface that only this frame sees (its neighbours' fields of
    view end 21 degrees from its axis), well in front of the wall, which --min_weight 1 lets into the mesh as a floating shell."""
    from PIL import Image
    from tests import fusion_cases as FC
    r = ROOM
    args = FC.write_room_scene(str(folder), r["frames"], r["h"], r["w"], r["focal"])
    path = os.path.join(str(folder), "depth", f"frame_{r['frame']:03d}.png")
    depth = np.array(Image.open(path)).astype(np.uint16)
    y0, x0 = (r["h"] - r["patch"]) // 2, (r["w"] - r["patch"]) // 2
    depth[y0:y0 + r["patch"], x0:x0 + r["patch"]] = r["patch_mm"]
    Image.fromarray(depth).save(path)
    return args + ROOM_FLAGS


def restated_room_mesh(args, voxel_size=0.02):
    """The mesh fuse_depth.py writes for `args` with --min_weight 1, by tests/tsdf_restated.py on the host: the files are read and the
    volume is placed the way cli.fuse_depth_main does it."""
    import glob
    from PIL import Image
    from acezero_amd.formats import match_poses, read_ace_pose_file, read_depth_png
    from acezero_amd.fusion import _w2c34, bounds_from_frames
    from tests import tsdf_restated as R
    rgb_files, depth_files = sorted(glob.glob(args[1])), sorted(glob.glob(args[4]))
    names, c2w_all, focals_all = read_ace_pose_file(args[0], 1000)
    rows = match_poses(names, rgb_files)
    depth = [read_depth_png(d) for d in depth_files]
    c2w = np.stack([c2w_all[k] for k in rows])
    focals = np.array([focals_all[k] * d.shape[0] / Image.open(f).size[1] for k, d, f in zip(rows, depth, rgb_files)])
    tau = 4.0 * voxel_size
    origin, dims = bounds_from_frames(depth, c2w, focals, voxel_size, tau)
    vol = R.Volume(origin, dims, voxel_size, tau)
    R.integrate(vol, depth, _w2c34(None, c2w, len(depth)), focals, [d.shape[1] / 2.0 for d in depth], [d.shape[0] / 2.0 for d in depth])
    return R.extract(vol.tsdf, vol.weight, None, vol.origin, vol.v, 1.0)
