"""Connected components of a mesh, the selection and the compaction of include/acez.h section P restated on the host: the definition
the HIP kernels of acezero_amd/csrc/mesh_api.hip are compared with, integer for integer (tests/test_mesh_gpu.py), checked on its own
against scipy without a GPU (tests/test_mesh_cpu.py). A helper module, not a test file. It shares nothing with the kernels' algorithm:
the labelling is a sequential union-find that links by size, whatever the ids, and takes the minimum of every set afterwards; the
rest is written from the header's sentences."""
import numpy as np


def classify(faces, m):
    """(valid, invalid, degenerate) bool [k]: invalid = an index outside 0 .. m - 1; degenerate = not invalid, two indices equal."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    invalid = ((f < 0) | (f >= m)).any(1)
    degenerate = ~invalid & ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2]))
    return ~invalid & ~degenerate, invalid, degenerate


def labels(faces, m):
    """int32 [m]: the smallest vertex id of every vertex's component."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valid, _, _ = classify(f, m)
    parent, size = list(range(m)), [1] * m

    def find(v):
        root = v
        while parent[root] != root:
            root = parent[root]
        while parent[v] != root:
            parent[v], v = root, parent[v]
        return root

    for a, b, c in f[valid].tolist():
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                if size[rx] < size[ry]:
                    rx, ry = ry, rx
                parent[ry] = rx
                size[rx] += size[ry]
    root = np.array([find(v) for v in range(m)], np.int64).reshape(m)
    smallest = np.full(m, m, np.int64)
    np.minimum.at(smallest, root, np.arange(m))
    return smallest[root].astype(np.int32)


def sizes(faces, label):
    """(faces_of, vertices_of) int32 [m], indexed by label; vertices count only where the component has a valid face."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    m = len(label)
    valid, _, _ = classify(f, m)
    faces_of = np.bincount(np.asarray(label, np.int64)[f[valid, 0]], minlength=m).astype(np.int32)
    vertices_of = np.bincount(np.asarray(label, np.int64), minlength=m).astype(np.int32)
    vertices_of[faces_of == 0] = 0
    return faces_of, vertices_of


def select(faces_of, min_faces=0, min_ratio=0.0, keep_largest=None):
    """bool [m]: the kept components, by label."""
    faces_of = np.asarray(faces_of, np.int64)
    m = len(faces_of)
    keep = np.zeros(m, bool)
    existing = np.flatnonzero(faces_of > 0).tolist()
    if not existing:
        return keep
    largest = max(int(faces_of[c]) for c in existing)
    ranked = sorted(existing, key=lambda c: (-int(faces_of[c]), c))
    for rank, c in enumerate(ranked):
        n = int(faces_of[c])
        keep[c] = (n >= min_faces and np.float64(n) >= np.float64(min_ratio) * np.float64(largest)
                   and (keep_largest is None or rank < keep_largest))
    return keep


def filter_components(vertices, colours, faces, min_faces=0, min_ratio=0.0, keep_largest=None):
    """(vertices, colours or None, faces int32, info) as acezero_amd.mesh.filter_components defines them."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    m, k = len(v), len(f)
    valid, invalid, degenerate = classify(f, m)
    lab = labels(f, m)
    faces_of, _ = sizes(f, lab)
    keep = select(faces_of, min_faces, min_ratio, keep_largest)
    face_keep = valid.copy()
    face_keep[valid] = keep[lab[f[valid, 0]]]
    used = np.zeros(m, bool)
    used[f[face_keep].reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    out_f = new_id[f[face_keep]].astype(np.int32).reshape(-1, 3)
    info = dict(components=int((faces_of > 0).sum()), components_kept=int(keep.sum()), faces_dropped=int(k - face_keep.sum()),
                vertices_dropped=int(m - used.sum()), largest_component_faces=int(faces_of.max()) if m else 0,
                invalid_faces=int(invalid.sum()), degenerate_faces=int(degenerate.sum()),
                size_histogram=[int(((faces_of >= lo) & (faces_of < hi)).sum()) for lo, hi in ((1, 10), (10, 100), (100, 1000), (1000, 10000),
                                                                                              (10000, 2 ** 31))])
    return v[used], None if colours is None else np.asarray(colours, np.uint8).reshape(-1, 3)[used], out_f, info
