"""The ICP loop of include/acez.h section N restated in numpy: ACCUMULATE on tests/geometry_restated.py's brute-force search with the
header's summation order, UPDATE with np.linalg.svd, the stage loop and the coarse-to-fine refinement; the scene and the recovery
case of tests/test_icp_cpu.py and tests/test_icp_gpu.py. A helper module, not a test file. Nothing here imports
acezero_amd.geometry."""
import functools

import numpy as np

from tests import geometry_restated as R
from tests.ordered_sums import block_sums, totals  # noqa: F401  (the header's summation order; the tests call I.block_sums, I.totals)

F = np.float32
TERMS = 18
RUNNING, CONVERGED, DEGENERATE = 0, 1, 2
STATUS = {RUNNING: "max_iterations", CONVERGED: "converged", DEGENERATE: "degenerate"}


# ------------------------------------------------------------------------------------------------------------------ the cases
def scene(n, seed):
    """float32 [n,3]: a floor, two walls and a bump, sampled at random: asymmetric and irregular, so that ICP cannot slide."""
    g = np.random.default_rng(seed)
    k = n // 4
    floor = np.c_[g.uniform(0, 3, k), g.uniform(0, 2, k), np.zeros(k)]
    wall_y = np.c_[g.uniform(0, 3, k), np.zeros(k), g.uniform(0, 2.5, k)]
    wall_x = np.c_[np.zeros(k), g.uniform(0, 2, k), g.uniform(0, 2.5, k)]
    u = g.uniform(0, 1, (n - 3 * k, 2))
    bump = np.c_[1 + 0.8 * u[:, 0], 0.5 + 0.5 * u[:, 1], 0.3 * np.sin(4 * u[:, 0]) + 0.4 + 0.3 * u[:, 1]]
    return np.concatenate([floor, wall_y, wall_x, bump]).astype(F)


def displacement(scale=1.0):
    """4 x 4 float64 S: a 2 degree rotation about (0.3, -0.5, 0.8), times `scale`, plus the shift (0.015, -0.01, 0.02) m."""
    from scipy.spatial.transform import Rotation
    axis = np.array([0.3, -0.5, 0.8])
    S = np.eye(4)
    S[:3, :3] = scale * Rotation.from_rotvec(np.deg2rad(2.0) * axis / np.linalg.norm(axis)).as_matrix()
    S[:3, 3] = [0.015, -0.01, 0.02]
    return S


STAGES = (0.2, 0.1, 0.05)
POINT_BOUND = 4 * 2.0 ** -22          # 4 float32 ulps at 3 m (an ulp in [2, 4) is 2^-22): 9.6e-7 m
T_BOUND = 1e-8


@functools.lru_cache(maxsize=None)
def recovery_case(with_scale):
    """(source, target, S): the target scene(2000, 7); the source every second target point moved by the inverse of S."""
    S = displacement(1.02 if with_scale else 1.0)
    tgt = scene(2000, 7)
    return R.apply_similarity(tgt[::2], np.linalg.inv(S)), tgt, S


def noisy_case():
    """(source, target, radius): the rigid recovery sources with N(0, 2 mm) noise, a fifth of them moved 1 m away."""
    src, tgt, _ = recovery_case(False)
    g = np.random.default_rng(3)
    src = src.astype(np.float64) + g.normal(scale=0.002, size=src.shape)
    src[g.permutation(len(src))[:len(src) // 5]] -= 1.0 / np.sqrt(3.0)              # behind the floor and both walls
    return src.astype(F), tgt, 0.05


# ------------------------------------------------------------------------------------------------------------------ ACCUMULATE
def terms(x, q, d2, found, pivot):
    """float64 [n,18]: per source its transformed point x (float32), its correspondence q (float32), d2 (float32)."""
    p = np.asarray(pivot, F).astype(np.float64)
    with np.errstate(all="ignore"):
        a, b = x.astype(np.float64) - p, q.astype(np.float64) - p
        t = np.zeros((len(x), TERMS))
        t[:, 0] = 1.0
        t[:, 1:4], t[:, 4:7] = a, b
        t[:, 7:16] = (b[:, :, None] * a[:, None, :]).reshape(-1, 9)        # 7 + 3 r + c: b_r * a_c
        t[:, 16] = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
        t[:, 17] = d2.astype(np.float64)
    return np.where(found[:, None], t, 0.0)


def accumulate(src, tgt, radius, T, pivot, nearest=R.nearest):
    """(partials [blocks,18], d2 float32 [n], index int32 [n]) for the sources in the order given."""
    x = R.apply_similarity(src, T)
    d2, idx = nearest(x, tgt, radius)
    found = idx >= 0
    q = np.asarray(tgt, F).reshape(-1, 3)[np.maximum(idx, 0)] if len(tgt) else np.zeros_like(x)
    return block_sums(terms(x, q, d2, found, pivot)), d2, idx


# ---------------------------------------------------------------------------------------------------------------------- UPDATE
def solve(s, pivot, with_scale, T):
    """The Umeyama step on the totals with LAPACK's SVD: the new T (4 x 4), or None if the totals do not determine it."""
    s, p = np.asarray(s, np.float64), np.asarray(pivot, F).astype(np.float64)
    count = s[0]
    if not count >= 3 or not np.isfinite(s).all():
        return None
    Sa, Sb, Sba = s[1:4], s[4:7], s[7:16].reshape(3, 3)
    C = Sba - np.outer(Sb, Sa) / count
    U, sig, Vt = np.linalg.svd(C)
    if not sig[1] > 1e-12 * sig[0]:
        return None
    sign = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0
    Rm = U @ np.diag([1.0, 1.0, sign]) @ Vt
    scale = 1.0
    if with_scale:
        scale = (sig[0] + sig[1] + sign * sig[2]) / (s[16] - Sa @ Sa / count)
        if not (np.isfinite(scale) and scale > 0):
            return None
    D = np.eye(4)
    D[:3, :3] = scale * Rm
    D[:3, 3] = Sb / count + p - scale * Rm @ (Sa / count + p)
    return D @ np.asarray(T, np.float64).reshape(4, 4)


def update(state, tot, n, pivot, with_scale, rel_fitness, rel_rmse, history):
    """One UPDATE on the state dict(T, status, prev) and the list of records; as icp_update of acezero_amd/csrc/icp_solve.h."""
    with np.errstate(all="ignore"):
        count, sum_d2 = tot[0], tot[17]
        fitness, rmse = count / float(n), np.sqrt(sum_d2 / count)
    history.append(dict(T=state["T"].copy(), count=count, sum_d2=sum_d2, fitness=fitness, rmse=rmse))
    prev, state["prev"] = state["prev"], (fitness, rmse)
    if len(history) >= 2 and abs(fitness - prev[0]) < rel_fitness and abs(rmse - prev[1]) < rel_rmse:
        state["status"] = CONVERGED
        return
    T = solve(tot, pivot, with_scale, state["T"])
    if T is None:
        state["status"] = DEGENERATE
    else:
        state["T"] = T


# ------------------------------------------------------------------------------------------------------------------- the loops
def grid_of(tgt, radius):
    """(lo, hi, c, dims) of acezero_amd.geometry's grid over the target for clouds small enough that the cell is never enlarged."""
    tgt = np.asarray(tgt, F).reshape(-1, 3)
    finite = tgt[np.isfinite(tgt).all(1)]
    lo, hi = (finite.min(0), finite.max(0)) if len(finite) else (np.zeros(3, F), np.zeros(3, F))
    c = F(radius) * F(1.0 + 2.0 ** -10)
    dims = [int(v) + 1 for v in np.floor((hi - lo) / c)]
    assert max(dims) <= 1024 and dims[0] * dims[1] * dims[2] <= 2 ** 24
    return lo, hi, c, dims


def source_order(src, tgt, radius):
    """The order icp_stage gives the sources: stable, by the cell of their nearest point of the target's box."""
    lo, hi, c, dims = grid_of(tgt, radius)
    return np.argsort(R.cells(np.minimum(np.maximum(np.asarray(src, F), lo), hi), lo, c, dims), kind="stable")


def pivot_of(tgt, radius):
    lo, hi, _, _ = grid_of(tgt, radius)
    return (lo + hi) * F(0.5)


def icp_stage(src, tgt, radius, max_iterations=30, with_scale=False, rel_fitness=1e-6, rel_rmse=1e-6, nearest=R.nearest):
    """acezero_amd.geometry.icp_stage restated: (T, info)."""
    src = np.asarray(src, F).reshape(-1, 3)
    src = src[source_order(src, tgt, radius)]
    pivot = pivot_of(tgt, radius)
    state, history = dict(T=np.eye(4), status=RUNNING, prev=(0.0, 0.0)), []
    for _ in range(max_iterations):
        if state["status"] != RUNNING:
            break
        partials, _, _ = accumulate(src, tgt, radius, state["T"], pivot, nearest)
        update(state, totals(partials), len(src), pivot, with_scale, rel_fitness, rel_rmse, history)
    info = dict(status=STATUS[state["status"]], iterations=len(history), fitness=[h["fitness"] for h in history],
                rmse=[h["rmse"] for h in history], count=[int(h["count"]) for h in history], sum_d2=[h["sum_d2"] for h in history],
                transforms=[h["T"] for h in history])
    return state["T"], info


def refine_alignment(rec, gt, transform=None, distances=STAGES, max_iterations=30, with_scale=False, nearest=R.nearest):
    """acezero_amd.geometry.refine_alignment restated (without voxels): (T, stage infos)."""
    T = np.eye(4) if transform is None else np.asarray(transform, np.float64)
    infos = []
    for d in distances:
        T_stage, info = icp_stage(R.apply_similarity(rec, T), gt, d, max_iterations, with_scale, nearest=nearest)
        if info["status"] != "degenerate":
            T = T_stage @ T
        infos.append(info)
    return T, infos
