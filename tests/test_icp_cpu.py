"""CPU: the ICP loop of include/acez.h section N on its numpy restatement (tests/icp_restated.py): the restated loop recovers a known
displacement within the bounds the kernels are held to in tests/test_icp_gpu.py; the host instantiation of the device-side update
(acezero_amd/csrc/icp_solve.h, through tests/icp_probe.hip) against the restated update with LAPACK's SVD; the entry points'
argument checks and eval_geometry.py's refusals, none of which needs a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import geometry_cases as GC
from tests import geometry_restated as R
from tests import icp_restated as I

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def probe():
    so = os.path.join(HERE, "_build", "libicp_probe.so")
    src = os.path.join(HERE, "icp_probe.hip")
    deps = [src] + [os.path.join(ROOT, "acezero_amd", "csrc", f) for f in ("icp_solve.h", "device_loop.h", "svd3.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                        "-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.probe_icp_solve.restype = C.c_int
    lib.probe_icp_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.probe_icp_update.restype = None
    lib.probe_icp_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def random_totals(rng, n=60, with_scale=True, noise=0.01):
    """Totals of n exact correspondences b = S a + noise around a pivot, a prior T, and the pieces."""
    pivot = rng.uniform(-2, 2, 3).astype(F)
    S = GC.similarity(scale=rng.uniform(0.7, 1.4) if with_scale else 1.0, axis=rng.normal(size=3), angle=rng.uniform(0, 0.5),
                      t=rng.uniform(-0.3, 0.3, 3))
    x = rng.uniform(-3, 3, (n, 3)).astype(F)
    q = (x.astype(np.float64) @ S[:3, :3].T + S[:3, 3] + rng.normal(scale=noise, size=(n, 3))).astype(F)
    d2 = ((x - q) ** 2).sum(1).astype(F)
    tot = I.totals(I.block_sums(I.terms(x, q, d2, np.ones(n, bool), pivot)))
    T = GC.similarity(scale=1.1, angle=0.2, t=(0.1, 0.2, -0.3))
    return tot, pivot, T, S


def test_scene():
    p = I.scene(2000, 7)
    assert p.dtype == F and p.shape == (2000, 3) and np.array_equal(p, I.scene(2000, 7))
    assert (p[:500, 2] == 0).all() and (p[500:1000, 1] == 0).all() and (p[1000:1500, 0] == 0).all() and (p[1500:] > 0).all()
    assert p.min() == 0 and p[:, 0].max() < 3 and p[:, 1].max() < 2 and p[:, 2].max() < 2.5
    S = I.displacement(1.02)
    assert np.allclose(np.cbrt(np.linalg.det(S[:3, :3])), 1.02) and np.allclose(S[:3, 3], [0.015, -0.01, 0.02])
    angle = np.arccos((np.trace(S[:3, :3]) / 1.02 - 1) / 2)
    assert np.isclose(np.rad2deg(angle), 2.0)


def test_summation_order():
    rng = np.random.default_rng(0)
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        t = rng.normal(size=(n, I.TERMS)) * 10.0 ** rng.integers(-6, 6, (n, 1))
        part = I.block_sums(t)
        assert part.shape == ((n + 255) // 256, I.TERMS)
        # the definition, lane by lane: butterfly per wavefront, wavefronts ascending
        for blk in range(len(part)):
            waves = []
            for w in range(4):
                v = np.zeros((64, I.TERMS))
                rows = t[blk * 256 + w * 64: blk * 256 + (w + 1) * 64]
                v[:len(rows)] = rows
                for s in (32, 16, 8, 4, 2, 1):
                    v = np.stack([v[lane] + v[lane ^ s] for lane in range(64)])
                waves.append(v[0])
            want = ((waves[0] + waves[1]) + waves[2]) + waves[3]
            assert np.array_equal(part[blk].view(np.uint64), want.view(np.uint64))
        tot = I.totals(part)
        assert np.allclose(tot, t.sum(0), rtol=1e-12, atol=1e-9 * np.abs(t).max())
    ones = np.ones((1000, I.TERMS))
    assert np.array_equal(I.block_sums(ones)[:, 0], [256, 256, 256, 232]) and I.totals(I.block_sums(ones))[0] == 1000
    many = I.totals(np.ones((700, I.TERMS)))                       # more partial rows than UPDATE has threads
    assert (many == 700).all()


def test_summation_order_at_both_widths():
    """The one restatement (tests/ordered_sums.py) at the 18 terms of ICP and the 29 of tracking: 1000 rows, workgroups of 256, 256,
    256 and 232, against the definition lane by lane; the totals of those four rows likewise."""
    rng = np.random.default_rng(1)

    def by_lanes(rows, terms):                                     # one workgroup: butterfly per wavefront, wavefronts ascending
        waves = []
        for w in range(4):
            v = np.zeros((64, terms))
            mine = rows[w * 64:(w + 1) * 64]
            v[:len(mine)] = mine
            for s in (32, 16, 8, 4, 2, 1):
                v = np.stack([v[lane] + v[lane ^ s] for lane in range(64)])
            waves.append(v[0])
        return ((waves[0] + waves[1]) + waves[2]) + waves[3]

    for terms in (18, 29):
        t = rng.normal(size=(1000, terms)) * 10.0 ** rng.integers(-6, 6, (1000, 1))
        part = I.block_sums(t)
        assert part.shape == (4, terms)
        for blk in range(4):
            assert np.array_equal(part[blk].view(np.uint64), by_lanes(t[blk * 256:(blk + 1) * 256], terms).view(np.uint64))
        # UPDATE: thread r < 4 holds 0.0 + row r, the other threads 0.0
        assert np.array_equal(I.totals(part).view(np.uint64), by_lanes(0.0 + part, terms).view(np.uint64))


@pytest.mark.parametrize("with_scale", [False, True], ids=["rigid", "with_scale"])
def test_restated_loop_recovers_the_displacement(with_scale):
    src, tgt, S = I.recovery_case(with_scale)
    assert np.abs(src.astype(np.float64) - tgt[::2]).max() > 0.03, "the clouds start well apart"
    T, infos = I.refine_alignment(src, tgt, None, I.STAGES, 30, with_scale)
    print([(i["iterations"], i["status"], i["fitness"][-1], i["rmse"][-1]) for i in infos], np.abs(T - S).max())
    for info in infos:
        assert info["status"] == "converged" and info["fitness"][-1] == 1.0 and info["count"][-1] == len(src)
        assert info["iterations"] == len(info["rmse"]) == len(info["transforms"]) <= 30
    assert infos[1]["iterations"] == 2 and infos[2]["iterations"] == 2
    assert np.abs(T - S).max() <= I.T_BOUND
    worst = np.linalg.norm(R.apply_similarity(src, T).astype(np.float64) - tgt[::2], axis=1).max()
    assert worst <= I.POINT_BOUND, worst


def test_restated_loop_stops():
    src, tgt, _ = I.recovery_case(False)
    T, info = I.icp_stage(src + F(10), tgt, 0.2)
    assert info["status"] == "degenerate" and info["iterations"] == 1 and info["count"] == [0] and np.array_equal(T, np.eye(4))
    T, info = I.icp_stage(src, tgt, 0.2, max_iterations=2)
    assert info["status"] == "max_iterations" and info["iterations"] == 2 and not np.array_equal(T, np.eye(4))
    assert np.array_equal(info["transforms"][0], np.eye(4))
    noisy, tgt, r = I.noisy_case()
    T, info = I.icp_stage(noisy, tgt, r)
    assert 0.7 < info["fitness"][-1] < 0.85 and info["iterations"] >= 3, "a partial overlap: of the moved fifth hardly any finds a target"


@pytest.mark.parametrize("with_scale", [False, True], ids=["rigid", "with_scale"])
def test_host_solve_matches_the_restated_update(probe, with_scale):
    rng = np.random.default_rng(5 + with_scale)
    for trial in range(200):
        tot, pivot, T0, S = random_totals(rng, n=int(rng.integers(3, 80)), with_scale=with_scale, noise=10.0 ** rng.uniform(-6, -1))
        want = I.solve(tot, pivot, with_scale, T0)
        T = np.ascontiguousarray(T0[:3].reshape(-1))
        ok = probe.probe_icp_solve(_p(tot), _p(pivot.astype(np.float64)), int(with_scale), _p(T))
        assert want is not None and ok == 1
        np.testing.assert_allclose(T.reshape(3, 4), want[:3], rtol=1e-9, atol=1e-9 * np.abs(want).max())
    # exact correspondences: the step is S
    tot, pivot, T0, S = random_totals(rng, n=40, with_scale=with_scale, noise=0.0)
    T = np.ascontiguousarray(np.eye(4)[:3].reshape(-1))
    assert probe.probe_icp_solve(_p(tot), _p(pivot.astype(np.float64)), int(with_scale), _p(T)) == 1
    assert np.abs(T.reshape(3, 4) - S[:3]).max() < 1e-6            # the targets were rounded to float32


def test_host_solve_refuses_degenerate_totals(probe):
    rng = np.random.default_rng(9)
    pivot = np.array([0.5, -0.25, 1.0], F)
    x = rng.uniform(-1, 1, (40, 3)).astype(F)
    line = (np.array([0.1, 0.2, 0.3]) + np.linspace(-1, 1, 40)[:, None] * np.array([0.5, -0.25, 1.0])).astype(F)
    d2 = np.full(40, 1e-4, F)

    def tot(a, b, k):
        return I.totals(I.block_sums(I.terms(a[:k], b[:k], d2[:k], np.ones(k, bool), pivot)))

    with_nan = tot(x, x + F(0.01), 40)
    with_nan[9] = np.nan
    with_inf = tot(x, x + F(0.01), 40)
    with_inf[17] = np.inf
    cases = {"two correspondences": tot(x, x + F(0.01), 2), "collinear": tot(line, line + F(0.01), 40), "a NaN total": with_nan,
             "an infinite total": with_inf, "no correspondence": np.zeros(18), "one point 40 times": tot(x[:1].repeat(40, 0), x[:1].repeat(40, 0), 40)}
    T0 = GC.similarity(scale=1.1, angle=0.2, t=(0.1, 0.2, -0.3))[:3].reshape(-1).copy()
    for name, totals in cases.items():
        for with_scale in (0, 1):
            assert I.solve(totals, pivot, with_scale, np.vstack([T0.reshape(3, 4), [0, 0, 0, 1]])) is None, name
            T = T0.copy()
            assert probe.probe_icp_solve(_p(totals), _p(pivot.astype(np.float64)), with_scale, _p(T)) == 0, name
            assert np.array_equal(T.view(np.uint64), T0.view(np.uint64)), name
            # through the whole update: the record is written, status DEGENERATE, T untouched bit for bit
            state = np.zeros(34)
            state[:12] = T0
            history = np.full((3, 16), -1.0)
            probe.probe_icp_update(_p(state), _p(totals), 40, _p(pivot.astype(np.float64)), with_scale, 1e-6, 1e-6, _p(history))
            assert state[12] == 2 and state[13] == 1 and np.array_equal(state[:12].view(np.uint64), T0.view(np.uint64)), name
            assert np.array_equal(history[0, :12], T0) and (history[1:] == -1).all(), name
            assert np.array_equal(state[16:].view(np.uint64), totals.view(np.uint64)), name
    good = tot(x, x + F(0.01), 3)                                # three points in general position are enough
    T = T0.copy()
    assert probe.probe_icp_solve(_p(good), _p(pivot.astype(np.float64)), 0, _p(T)) == 1 and not np.array_equal(T, T0)


def test_host_update_records_and_stops_like_the_restatement(probe):
    """Three updates on totals of a converging sequence: the records, the previous values and the stopping rule (a), which only
    holds from the second record on and leaves T as it is."""
    rng = np.random.default_rng(11)
    tot, pivot, T0, _ = random_totals(rng, n=50, with_scale=False, noise=1e-3)
    n = 64
    state = np.zeros(34)
    state[:12] = np.eye(4)[:3].reshape(-1)
    history = np.zeros((4, 16))
    restated, records = dict(T=np.eye(4), status=I.RUNNING, prev=(0.0, 0.0)), []
    sequence = [tot, tot * 1.0, tot]
    sequence[1] = tot.copy()
    sequence[1][17] *= 1.5                                         # the rmse moves: no convergence at the second record
    for k, t in enumerate(sequence):
        probe.probe_icp_update(_p(state), _p(t), n, _p(pivot.astype(np.float64)), 0, 1e-6, 1e-6, _p(history))
        I.update(restated, t, n, pivot, False, 1e-6, 1e-6, records)
        assert state[13] == k + 1 == len(records) and state[12] == restated["status"]
        np.testing.assert_allclose(state[:12].reshape(3, 4), restated["T"][:3], rtol=1e-9, atol=1e-9 * np.abs(restated["T"]).max())
        rec = records[-1]
        assert history[k, 12] == rec["count"] == 50 and history[k, 13] == rec["sum_d2"]
        assert history[k, 14] == rec["fitness"] == 50 / 64 and history[k, 15] == rec["rmse"] == np.sqrt(t[17] / 50)
        np.testing.assert_allclose(history[k, :12].reshape(3, 4), rec["T"][:3], rtol=1e-9, atol=1e-9 * np.abs(rec["T"]).max())
    assert state[12] == I.RUNNING
    # a fourth with the third's totals: nothing moved -> CONVERGED, T unchanged bit for bit. A first record never converges, even
    # against previous values that happen to match.
    before = state[:12].copy()
    probe.probe_icp_update(_p(state), _p(sequence[2]), n, _p(pivot.astype(np.float64)), 0, 1e-6, 1e-6, _p(history))
    assert state[12] == I.CONVERGED and state[13] == 4 and np.array_equal(state[:12].view(np.uint64), before.view(np.uint64))
    first = np.zeros(34)
    first[:12] = np.eye(4)[:3].reshape(-1)
    first[14], first[15] = 50 / 64, np.sqrt(tot[17] / 50)
    probe.probe_icp_update(_p(first), _p(tot), n, _p(pivot.astype(np.float64)), 0, 1e-6, 1e-6, _p(np.zeros((1, 16))))
    assert first[12] == I.RUNNING and first[13] == 1


def test_argument_validation_without_device():
    from acezero_amd import _native as N
    lib = N.lib()
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data                                          # never dereferenced: every call below is refused before any launch

    def refused(rc, text):
        assert rc == -1 and text in lib.acez_last_error(), (rc, lib.acez_last_error())

    def accumulate(ref=p, ref_index=p, start=p, m=10, o=(0.0, 0.0, 0.0), c=0.1, dims=(4, 4, 4), src=p, n=10, r=0.05, pivot=(0.0, 0.0, 0.0),
                   state=p, partials=p):
        return lib.acez_geom_icp_accumulate(ref, ref_index, start, m, *o, c, *dims, src, n, r, *pivot, state, partials, None)

    def update(partials=p, n=10, pivot=(0.0, 0.0, 0.0), with_scale=0, rel_fitness=1e-6, rel_rmse=1e-6, max_iterations=30, state=p, history=p):
        return lib.acez_geom_icp_update(partials, n, *pivot, with_scale, rel_fitness, rel_rmse, max_iterations, state, history, None)

    for name in ("ref", "ref_index", "start", "src", "state", "partials"):
        refused(accumulate(**{name: None}), b"null pointer")
    refused(accumulate(m=-1), b"count")
    refused(accumulate(m=2 ** 31), b"count")
    refused(accumulate(n=0), b"count")
    refused(accumulate(n=-1), b"count")
    refused(accumulate(n=2 ** 31), b"count")
    refused(accumulate(dims=(0, 4, 4)), b"dimensions")
    refused(accumulate(dims=(4, 1025, 4)), b"dimensions")
    refused(accumulate(dims=(512, 512, 65)), b"too large")
    refused(accumulate(o=(float("nan"), 0.0, 0.0)), b"origin")
    refused(accumulate(c=float("nan")), b"cell edge")
    refused(accumulate(c=0.0, r=0.0), b"cell edge")
    refused(accumulate(r=0.0), b"radius")
    refused(accumulate(r=-0.05), b"radius")
    refused(accumulate(r=float("inf")), b"radius")
    refused(accumulate(c=0.05, r=0.05), b"2^-10")
    refused(accumulate(c=float(F(0.05) * F(1 + 2.0 ** -11)), r=0.05), b"2^-10")
    refused(accumulate(pivot=(0.0, float("inf"), 0.0)), b"pivot")
    for name in ("partials", "state", "history"):
        refused(update(**{name: None}), b"null pointer")
    refused(update(n=0), b"count")
    refused(update(n=2 ** 31), b"count")
    refused(update(pivot=(float("nan"), 0.0, 0.0)), b"pivot")
    refused(update(max_iterations=0), b"max_iterations")
    refused(update(max_iterations=-3), b"max_iterations")
    refused(update(rel_fitness=-1e-9), b"tolerances")
    refused(update(rel_rmse=float("nan")), b"tolerances")
    refused(update(rel_rmse=float("inf")), b"tolerances")
    if not torch.cuda.is_available():                            # what is valid gets as far as the device check, and no further
        for rc in (accumulate(), accumulate(m=0, ref=None, ref_index=None), update(), update(rel_fitness=0.0, rel_rmse=0.0)):
            assert rc == -3 and b"no HIP device" in lib.acez_last_error()


def test_host_tensors_are_refused_and_the_functions_are_exported():
    from acezero_amd import geometry as G
    assert {"icp_stage", "refine_alignment"} <= set(G.__all__)
    pts = torch.zeros(4, 3)
    for call in (lambda: G.icp_stage(pts, pts, 0.1), lambda: G.refine_alignment(pts, pts, distances=[0.1])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_cli_refusals(tmp_path):
    from acezero_amd import cli
    from acezero_amd.formats import write_ply
    pts = GC.uniform(1, 20)
    rec, gt = str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply")
    write_ply(rec, pts, np.zeros((20, 3), np.uint8))
    write_ply(gt, pts, np.zeros((20, 3), np.uint8))
    with pytest.raises(SystemExit, match="--icp_distances must be positive"):
        cli.eval_geometry_main([rec, gt, "--icp", "True", "--icp_distances", "0.1", "0"])
    with pytest.raises(SystemExit, match="--icp_distances must be positive"):
        cli.eval_geometry_main([rec, gt, "--icp", "True", "--icp_distances", "-0.1"])
    with pytest.raises(SystemExit, match="2 values for 3 ICP stages"):
        cli.eval_geometry_main([rec, gt, "--icp", "True", "--icp_voxel_sizes", "0.02", "0.01"])
    with pytest.raises(SystemExit, match="1 values for 2 ICP stages"):
        cli.eval_geometry_main([rec, gt, "--icp", "True", "--icp_distances", "0.1", "0.05", "--icp_voxel_sizes", "0.02"])
    with pytest.raises(SystemExit, match="--icp_max_iterations"):
        cli.eval_geometry_main([rec, gt, "--icp", "True", "--icp_max_iterations", "0"])
    opt = cli.eval_geometry_parser().parse_args([rec, gt])
    assert opt.icp is False and opt.icp_distances is None and opt.icp_voxel_sizes is None and opt.icp_max_iterations == 30
    assert opt.icp_scale is False
