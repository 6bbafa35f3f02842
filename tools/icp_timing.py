"""The ICP loop on the box: one ACCUMULATE, one UPDATE, the pair, and a whole 30-iteration stage of n source
points against n target points at a 5 cm radius -- the clouds of tools/geometry_timing.py, the setting of section 4l's table --
beside acez_geom_nearest on the same buffers (what the fp64 moments cost on top of the search) and beside one iteration of scipy's
k-d tree with 16 workers + numpy on the same machine. HIP events around each call, median of the repetitions, the kernels
alternating in three rounds. `accumulate` runs under the identity, the transform the sources were ordered for; `pair` runs ACCUMULATE
under the transform of the first step, when the sources have moved against the cells they were ordered by.

    python tools/icp_timing.py [--points 1000000] [--radius 0.05] [--reps 10] [--no_tree] [--also name=other_build.so]
                               [--out profiles/icp_timing.json]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/icp_timing.py --trace_stage displaced     (or: aligned)

The source cloud is the 5 mm-noise wall sample moved by 1 degree and 1 cm, so that the loop has something to do. The whole stage is
timed from the call to the read-back, once with the default tolerances (it stops when it has converged; the launches after that are
idle) and once with tolerances of 0 (all 30 iterations run). --also adds other builds of the library (tools/lib_variant.sh) to the
rotation of the nearest kernel, e.g. one from before the search became a shared device function. Prints one JSON line and writes
it to --out. --trace_stage runs nothing but two forced 30-iteration stages, from the displaced sources or from the wall sample itself
(an aligned start), for a kernel trace in a run of its own: the per-kernel times of profiles/icp_kernel_trace.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from acezero_amd import _native as N  # noqa: E402
from acezero_amd import geometry as G  # noqa: E402
from acezero_amd.head import _ptr, _stream  # noqa: E402
from tests import geometry_cases as GC  # noqa: E402
from tools.geometry_timing import wall_samples  # noqa: E402
from tools.rgbd_timing import _time  # noqa: E402


def umeyama(a, b, with_scale=False):
    ma, mb = a.mean(0), b.mean(0)
    A, B = a - ma, b - mb
    U, S, Vt = np.linalg.svd(B.T @ A)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    s = (S * np.diag(D)).sum() / (A * A).sum() if with_scale else 1.0
    T = np.eye(4)
    T[:3, :3] = s * U @ D @ Vt
    T[:3, 3] = mb - T[:3, :3] @ ma
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no_tree", action="store_true")
    ap.add_argument("--also", nargs="*", default=[], help="name=path of further builds of the library: their acez_geom_nearest joins the rotation")
    ap.add_argument("--out", default=os.path.join("profiles", "icp_timing.json"))
    ap.add_argument("--trace_stage", choices=["displaced", "aligned"], default=None, help="only two forced 30-iteration stages, for a kernel trace")
    a = ap.parse_args()
    others = {spec.split("=", 1)[0]: N._load(spec.split("=", 1)[1], lenient=True) for spec in a.also}
    n, r = a.points, a.radius
    tgt_h, rec_h = wall_samples(1, n, 0.002), wall_samples(2, n, 0.005)
    S = GC.similarity(scale=1.0, angle=np.deg2rad(1.0), t=(0.01, -0.005, 0.008))
    p = rec_h.astype(np.float64)
    src_h = ((p - S[:3, 3]) @ S[:3, :3]).astype(np.float32)        # the inverse of the rigid S: R^T (p - t)
    tgt, src = torch.from_numpy(tgt_h).cuda(), torch.from_numpy(src_h).cuda()
    if a.trace_stage:
        start = src if a.trace_stage == "displaced" else torch.from_numpy(rec_h).cuda()
        for _ in range(2):
            T, info = G.icp_stage(start, tgt, r, max_iterations=30, rel_fitness=0.0, rel_rmse=0.0)
        print(a.trace_stage, info["iterations"], info["status"], info["fitness"][-1], info["rmse"][-1])
        return
    g = G.build_grid(tgt, r)
    pivot = [float(v) for v in (g.origin + g.hi) * np.float32(0.5)]
    src_sorted = src[G.order_by_cell(src, g)].contiguous()
    state = torch.zeros(34, dtype=torch.float64, device="cuda")
    state[[0, 5, 10]] = 1.0
    start_state = state.clone()
    partials = torch.empty(((n + 255) // 256, 18), dtype=torch.float64, device="cuda")
    history = torch.zeros((30, 16), dtype=torch.float64, device="cuda")
    d2 = torch.empty(n, dtype=torch.float32, device="cuda")
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    grid_args = (_ptr(g.ref_sorted), _ptr(g.ref_index), _ptr(g.cell_start), g.ref_sorted.shape[0], float(g.origin[0]), float(g.origin[1]),
                 float(g.origin[2]), float(g.cell), *g.dims)

    def nearest(lib=None):
        N.check((lib or N.lib()).acez_geom_nearest(*grid_args, _ptr(src_sorted), n, float(np.float32(r)), _ptr(d2), _ptr(idx), _stream()))

    def accumulate():
        N.check(N.lib().acez_geom_icp_accumulate(*grid_args, _ptr(src_sorted), n, float(np.float32(r)), *pivot, _ptr(state), _ptr(partials), _stream()))

    def update():
        state.copy_(start_state)                                  # a running state at record 0: every repetition does the same work
        N.check(N.lib().acez_geom_icp_update(_ptr(partials), n, *pivot, 0, 0.0, 0.0, 30, _ptr(state), _ptr(history), _stream()))

    def reset():
        state.copy_(start_state)

    def pair():
        accumulate()
        update()

    out = {"points": n, "radius": r, "reps": a.reps, "grid": "x".join(map(str, g.dims)), "partial_rows": int(partials.shape[0])}
    ms = {name: [] for name in ["nearest", "accumulate", "reset_and_update", "reset", "pair"] + [f"nearest_{k}" for k in others]}
    for _ in range(3):                                            # alternate
        ms["nearest"].append(_time(nearest, a.reps))
        for name, lib in others.items():
            ms[f"nearest_{name}"].append(_time(lambda: nearest(lib), a.reps))
        reset()
        ms["accumulate"].append(_time(accumulate, a.reps))
        ms["reset_and_update"].append(_time(update, a.reps))
        ms["reset"].append(_time(reset, a.reps))
        ms["pair"].append(_time(pair, a.reps))
    for name, v in ms.items():
        out[f"{name}_ms"], out[f"{name}_ms_rounds"] = float(np.median(v)), v
    out["update_ms"] = out["reset_and_update_ms"] - out["reset_ms"]
    out["moments_on_top_of_the_search_ms"] = out["accumulate_ms"] - out["nearest_ms"]
    out["pair_without_reset_ms"] = out["pair_ms"] - out["reset_ms"]
    out["found_first_iteration"] = int((idx >= 0).sum().item())
    # 30 launches back to back, as a stage enqueues them, with no synchronisation in between: per launch
    reset()
    out["nearest_30_back_to_back_ms_each"] = _time(lambda: [nearest() for _ in range(30)], 5) / 30
    out["accumulate_30_back_to_back_ms_each"] = _time(lambda: [accumulate() for _ in range(30)], 5) / 30

    def whole_from(cloud, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T, info = G.icp_stage(cloud, tgt, r, max_iterations=30, **kw)
        return (time.perf_counter() - t0) * 1e3, T, info

    def whole(**kw):
        return whole_from(src, **kw)

    whole()                                                       # warm
    runs = runs_default = [whole() for _ in range(5)]
    out["stage_default_tolerances_ms"] = float(np.median([x[0] for x in runs]))
    out["stage_default_tolerances_iterations"], out["stage_default_tolerances_status"] = runs[0][2]["iterations"], runs[0][2]["status"]
    out["stage_final_fitness"], out["stage_final_rmse"] = runs[0][2]["fitness"][-1], runs[0][2]["rmse"][-1]
    out["stage_max_difference_to_the_displacement"] = float(np.abs(runs[0][1] - S).max())
    runs = [whole(rel_fitness=0.0, rel_rmse=0.0) for _ in range(5)]
    out["stage_30_iterations_ms"] = float(np.median([x[0] for x in runs]))
    out["stage_30_iterations_ran"] = runs[0][2]["iterations"]
    # the loop alone, grid and ordering excluded: 30 pairs from the identity, events around them
    loop = []
    for _ in range(5):
        reset()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(30):
            accumulate()
            N.check(N.lib().acez_geom_icp_update(_ptr(partials), n, *pivot, 0, 0.0, 0.0, 30, _ptr(state), _ptr(history), _stream()))
        e1.record()
        torch.cuda.synchronize()
        loop.append(e0.elapsed_time(e1))
    out["loop_30_pairs_ms"] = float(np.median(loop))
    # the same from where a refinement's later stages start: the sources under the alignment the stage above found, ordered by
    # the cells they then lie in (refine_alignment orders every stage's sources anew)
    runs = [whole_from(G.apply_similarity(src, T_found), rel_fitness=0.0, rel_rmse=0.0) for T_found in [runs_default[0][1]] * 5]
    out["stage_30_iterations_from_the_alignment_ms"] = float(np.median([x[0] for x in runs]))
    if not a.no_tree:
        from scipy.spatial import cKDTree
        t0 = time.perf_counter()
        tree = cKDTree(tgt_h)
        out["ckdtree_build_s"] = time.perf_counter() - t0
        T = np.eye(4)
        its = []
        for _ in range(3):
            t0 = time.perf_counter()
            x = (src_h.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
            dist, j = tree.query(x, k=1, distance_upper_bound=r, workers=16)
            ok = np.isfinite(dist)
            T = umeyama(x[ok].astype(np.float64), tgt_h[j[ok]].astype(np.float64)) @ T
            its.append(time.perf_counter() - t0)
        out["ckdtree_16_workers_iteration_s"], out["ckdtree_16_workers_iteration_s_each"] = float(np.median(its)), its
    line = json.dumps({k: (float(f"{x:.4g}") if isinstance(x, float) else x) for k, x in out.items()})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
