"""CPU: the DEFINITION of the semi-global aggregation (include/acez.h section M) checked on its numpy restatement
(tests/sgm_restated.py), so that the kernels' bit-for-bit parity with it (tests/test_sgm_gpu.py) means something; what the definition
gives on a scene with a textureless band (tests/sgm_cases.py); the new entry points' argument checks, which need no device.

Measured here with the restatement on the band scene (six cameras of 96 x 128 px, 64 planes over 1 .. 3 m, four sources, keep 2,
window radius 2, the unchanged check; 17604 band pixels of 73728):

                                 band pixels with a depth   all pixels with a depth   kept pixels > 2 % off   ... inside the band
    plain sweep                  0.12185 (2145)             0.60040 (44266)           0.03305 (1463)          0.47879 (1027)
    SGM, 4 paths, P1/P2 80/640   0.71785 (12637)            0.78916 (58183)           0.02958 (1721)          0.09164 (1158)

80 / 640 are the defaults of acezero_amd.mvs.sgm_penalties at keep 2, window 2 (1.6 and 12.8 per sample, n = 50). Fused with
tests/tsdf_restated.py at 2 cm voxels, min_weight 2: 194 (plain) and 2026 (SGM) mesh vertices inside the band region
(sgm_cases.in_band_region), the farthest vertex 44.60 mm and 59.03 mm from a plane of the scene. The kernels must agree bit for bit, so
the margins below only guard against edits to the scene."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import mvs_cases as MC
from tests import mvs_restated as R
from tests import sgm_cases as SC
from tests import sgm_restated as SR

PLAIN = dict(band=0.12185, all=0.60040, bad=0.03305, band_bad=0.47879)
SGM = dict(band=0.71785, all=0.78916, bad=0.02958, band_bad=0.09164)
BAND_VERTICES = dict(plain=194, sgm=2026)        # tests/test_sgm_gpu.py imports these
SGM_MESH_BOUND = 1.25 * 0.05903                  # metres
RANGES = [(MC.Z_NEAR, MC.Z_FAR)] * SC.N


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def scalar_path(C_, dy, dx, p1, p2):
    """L_r by the header's sentence, one number at a time; nothing shared with tests/sgm_restated.py."""
    D, h, w = C_.shape
    L = np.zeros((D, h, w), np.int64)
    ys = range(h) if dy >= 0 else range(h - 1, -1, -1)
    xs = range(w) if dx >= 0 else range(w - 1, -1, -1)
    for y in ys:
        for x in xs:
            qy, qx = y - dy, x - dx
            for k in range(D):
                if not (0 <= qy < h and 0 <= qx < w):
                    L[k, y, x] = int(C_[k, y, x])
                    continue
                m = min(int(L[j, qy, qx]) for j in range(D))
                terms = [int(L[k, qy, qx]), m + p2]
                if k - 1 >= 0:
                    terms.append(int(L[k - 1, qy, qx]) + p1)
                if k + 1 <= D - 1:
                    terms.append(int(L[k + 1, qy, qx]) + p1)
                L[k, y, x] = int(C_[k, y, x]) + min(terms) - m
    return L


VOLUMES = [(D, h, w) for D in (2, 3, 5) for (h, w) in ((1, 1), (1, 7), (6, 1), (4, 6))]
PENALTIES = ((3, 20), (7, 7), (1, 32767))


@functools.lru_cache(maxsize=None)
def random_volume(D, h, w):
    return np.random.default_rng(1000 * D + 10 * h + w).integers(0, 60, (D, h, w)).astype(np.int32)


def test_select_without_aggregation_is_the_sweep():
    """The pin's numpy analogue: SELECT on the unaggregated C equals mvs_restated.sweep bit for bit."""
    images, _, _, rows = MC.scene(3)
    g = [R.prefilter(im) for im in images]
    cases = [(g, rows, 1, [0, 2], MC.Z_NEAR, MC.Z_FAR, MC.PLANES, 2, 2), (g, rows, 0, [1, 2], 1.5, 2.0, 2, 2, 1)]
    sizes = [(37, 53), (37, 53), (30, 44), (37, 53)]
    eyes, targets = [(0, 0, 0), (0.12, 0.01, 0), (-0.1, -0.02, 0.01), (0.02, 0, 3.5)], [(0, 0, 2), (0.05, 0, 2), (0, 0.02, 2), (0.02, 0, 6)]
    rimages, rrows = MC.random_frames(3, sizes, [60.0, 60.0, 45.0, 60.0], eyes, targets)
    rg = [R.prefilter(im) for im in rimages]
    cases += [(rg, rrows, 0, [1, 2], 1.0, 3.0, 33, 2, 2), (rg, rrows, 0, [3, 1], 1.0, 3.0, 3, 0, 2), (rg, rrows, 2, [0, 1, 3], 1.0, 3.0, 17, 4, 1)]
    for g_, rows_, ref, src, near, far, D, radius, keep in cases:
        want = R.sweep(g_, rows_, ref, src, near, far, D, radius=radius, keep=keep)
        Cv, n_in = R.cost_volume(g_, rows_, ref, src, near, far, D, radius, 40, keep)
        got = SR.select(Cv, n_in >= keep, near, far)
        assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("direction", range(1, 9))
def test_each_direction_against_a_scalar_loop(direction):
    dy, dx = SR.DIRECTIONS[direction - 1]
    assert SR.DIRECTIONS == ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))
    for D, h, w in VOLUMES:
        Cv = random_volume(D, h, w)
        for p1, p2 in PENALTIES:
            got = SR.path(Cv, direction, p1, p2)
            assert np.array_equal(got, scalar_path(Cv, dy, dx, p1, p2)), (D, h, w, p1, p2)
            assert (got >= Cv).all() and (got <= Cv.astype(np.int64) + p2).all()                 # C <= L_r <= C + P2
            if h == 1 and dy != 0 or w == 1 and dx != 0:
                assert np.array_equal(got, Cv)                                                   # every predecessor is outside


def test_path_bounds_on_a_large_volume():
    Cv = np.random.default_rng(4).integers(0, 32768, (9, 13, 17)).astype(np.int32)
    for direction in range(1, 9):
        for p1, p2 in ((80, 640), (32767, 32767)):
            L = SR.path(Cv, direction, p1, p2)
            assert (L >= Cv).all() and (L <= Cv.astype(np.int64) + p2).all()
    assert SR.aggregate(Cv, 8, 32767, 32767).max() <= 8 * (32767 + 32767)


def test_s_is_the_sum_of_its_paths():
    Cv = random_volume(5, 4, 6)
    single = [SR.path(Cv, r, 3, 20) for r in range(1, 9)]
    assert np.array_equal(SR.aggregate(Cv, 4, 3, 20), sum(single[:4]))
    assert np.array_equal(SR.aggregate(Cv, 8, 3, 20), sum(single))
    assert not np.array_equal(SR.aggregate(Cv, 4, 3, 20), SR.aggregate(Cv, 8, 3, 20))


def test_a_volume_constant_over_the_planes_rejects_every_pixel():
    """All L_r of a pixel tie, so S ties: plane 0 wins, an end plane; and with costs of 0 it is 0 against 0, not unique. (Two planes
    have neither an end-plane rule nor a plane outside the neighbourhood: the far plane is kept, as in section L.)"""
    rng = np.random.default_rng(2)
    for D in (2, 3, 9):
        for base in (np.zeros((5, 7), np.int32), rng.integers(0, 500, (5, 7)).astype(np.int32)):
            Cv = np.broadcast_to(base, (D, 5, 7)).copy()
            for paths in (4, 8):
                S = SR.aggregate(Cv, paths, 10, 80)
                assert (S == S[:1]).all()
                depth, _, plane = SR.select(S, np.ones(S.shape, bool), 1.0, 3.0)
                assert (plane == 0).all()
                assert (depth == 0).all() if D > 2 else (depth == 3.0).all()


@functools.lru_cache(maxsize=None)
def band_estimates():
    """(scene, sources, plain uint16 maps, SGM uint16 maps) of the band scene, by the restatements, at the default penalties."""
    from acezero_amd.mvs import SGM_PATHS, sgm_penalties
    assert SGM_PATHS == 4 and sgm_penalties(SC.KEEP, SC.WINDOW) == (80, 640)
    sc = SC.scene()
    sources = MC.nearest_sources(SC.N, SC.SOURCES)
    plain, _ = R.estimate(sc[0], sc[3], sources, RANGES, SC.PLANES)
    sgm, _ = SR.estimate(sc[0], sc[3], sources, RANGES, SC.PLANES)
    return sc, sources, plain, sgm


def figures(maps, truth, bands):
    q = [o.astype(np.float64) * 0.001 for o in maps]
    off = [(x > 0) & (np.abs(x - t) / t > 0.02) for x, t in zip(q, truth)]
    kept, total = sum(int((x > 0).sum()) for x in q), sum(x.size for x in q)
    band_kept, band_total = sum(int(((x > 0) & b).sum()) for x, b in zip(q, bands)), sum(int(b.sum()) for b in bands)
    return dict(band=band_kept / band_total, all=kept / total, bad=sum(int(o.sum()) for o in off) / kept,
                band_bad=sum(int((o & b).sum()) for o, b in zip(off, bands)) / band_kept)


def test_band_scene_figures():
    (_, truth, _, _, bands), _, plain, sgm = band_estimates()
    assert sum(int(b.sum()) for b in bands) == 17604
    for name, maps, measured in (("plain", plain, PLAIN), ("sgm", sgm, SGM)):
        got = figures(maps, truth, bands)
        print(name, {k: round(v, 5) for k, v in got.items()})
        assert got["band"] >= 0.8 * measured["band"] and got["all"] >= 0.8 * measured["all"]
        assert got["bad"] <= 1.25 * measured["bad"] and got["band_bad"] <= 1.25 * measured["band_bad"]


def test_aggregation_fills_the_band_without_adding_error():
    """Conditions, not measurements: at least 3 x the plain sweep's band coverage (measured 5.9 x), and an overall share of pixels
    beyond 2 % of at most 1.25 x the plain sweep's (measured 0.89 x)."""
    (_, truth, _, _, bands), _, plain, sgm = band_estimates()
    a, b = figures(plain, truth, bands), figures(sgm, truth, bands)
    assert b["band"] >= 3.0 * a["band"]
    assert b["bad"] <= 1.25 * a["bad"]


def test_fused_mesh_fills_the_band():
    """The restated chain estimate -> fuse -> extract on the band scene, plain and aggregated: where BAND_VERTICES and
    SGM_MESH_BOUND come from."""
    from acezero_amd.fusion import bounds_from_frames
    from tests import tsdf_restated as TR
    from tests.test_mvs_cpu import plane_distance
    (_, _, c2w, _, _), _, plain, sgm = band_estimates()
    inside = {}
    for name, out in (("plain", plain), ("sgm", sgm)):
        origin, dims = bounds_from_frames(out, c2w, MC.FOCAL, 0.02, 0.08)
        vol = TR.Volume(origin, dims, 0.02, 0.08)
        TR.integrate(vol, out, np.linalg.inv(c2w), [MC.FOCAL] * SC.N, [MC.W / 2.0] * SC.N, [MC.H / 2.0] * SC.N)
        v, _, f = TR.extract(vol.tsdf, vol.weight, None, vol.origin, vol.v, 2.0)
        inside[name] = int(SC.in_band_region(v).sum())
        print(f"{name}: {len(v)} vertices, {len(f)} faces, {inside[name]} inside the band region, farthest {plane_distance(v).max() * 1000:.2f} mm")
        if name == "sgm":
            assert plane_distance(v).max() <= SGM_MESH_BOUND
    assert inside == BAND_VERTICES
    assert inside["sgm"] >= 3 * inside["plain"]


def test_default_penalties_scale_with_the_samples_of_a_cost():
    from acezero_amd.mvs import sgm_penalties
    assert sgm_penalties(2, 2) == (80, 640) and sgm_penalties(1, 0) == (2, 13) and sgm_penalties(4, 4) == (518, 4147)
    assert sgm_penalties(2, 2, 5, None) == (5, 640) and sgm_penalties(2, 2, None, 30) == (30, 30) and sgm_penalties(2, 2, 9, 11) == (9, 11)
    assert sgm_penalties(1, 2, 500, None) == (500, 500)          # a frame with one source kept: its default P2 (320) gives way to the given P1
    assert sgm_penalties(2, 2, 500, None) == (500, 640)


def test_argument_validation_without_device():
    from acezero_amd import _native as N_
    from tests.test_mvs_cpu import native_rows
    lib = N_.lib()
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data                                          # never dereferenced: every call below is refused before any launch
    rows = [R.Row(np.eye(4), 40.0, 4.0, 3.0, 6, 8) for _ in range(3)]
    table, n_pixels = native_rows(rows)
    src = (C.c_int32 * 8)(1, 2, 1, 2, 1, 2, 1, 2)

    def refused(rc, text):
        assert rc == -1 and text in lib.acez_last_error(), lib.acez_last_error()

    def volume(g=p, n_pixels=144, frames=table, n_frames=3, ref=0, sources=src, n_sources=2, near=1.0, far=3.0, planes=16, radius=2, T=40, keep=1,
               vol=p, n_volume=768):
        return lib.acez_mvs_volume(g, n_pixels, frames, n_frames, ref, sources, n_sources, near, far, planes, radius, T, keep, vol, n_volume, None)

    def aggregate(vol=p, s=p, n_volume=768, h=6, w=8, planes=16, paths=4, direction=0, p1=10, p2=80):
        return lib.acez_mvs_aggregate(vol, s, n_volume, h, w, planes, paths, direction, p1, p2, None)

    def select(vol=p, s=p, n_volume=768, n_pixels=144, frames=table, n_frames=3, ref=0, near=1.0, far=3.0, planes=16, q=5, depth=p):
        return lib.acez_mvs_select(vol, s, n_volume, n_pixels, frames, n_frames, ref, near, far, planes, q, depth, None, None, None)

    for call in (volume, aggregate, select):
        refused(call(vol=None), b"null pointer")
        refused(call(n_volume=767), b"volume smaller")           # 6 x 8 x 16 elements
        refused(call(n_volume=-1), b"volume smaller")
        refused(call(planes=1), b"plane count")
        refused(call(planes=1025), b"plane count")
    for call in (volume, select):
        refused(call(frames=None), b"null pointer")
        refused(call(n_pixels=143 if call is volume else 47), b"past the end")   # the selection reads the reference's row alone
        refused(call(n_pixels=-1), b"negative buffer length")
        refused(call(n_frames=0), b"frame count")
        refused(call(ref=3), b"reference index")
        refused(call(ref=-1), b"reference index")
        refused(call(near=0.0), b"0 < near < far")
        refused(call(near=3.0), b"0 < near < far")
        refused(call(far=float("inf")), b"0 < near < far")
        refused(call(near=float("nan")), b"0 < near < far")
    # section L's refusals of the sweep hold for the volume
    refused(volume(g=None), b"null pointer")
    refused(volume(sources=None), b"null pointer")
    refused(volume(n_sources=0), b"source count")
    refused(volume(n_sources=9), b"source count")
    src[1] = 3
    refused(volume(), b"source index")
    src[1] = 2
    refused(volume(radius=-1), b"window radius")
    refused(volume(radius=5), b"window radius")
    refused(volume(T=0), b"truncation")
    refused(volume(T=256), b"truncation")
    refused(volume(keep=0), b"keep")
    refused(volume(keep=3), b"keep")
    # the volume's 15 bits: keep * (2w + 1)^2 * T
    refused(volume(n_sources=8, keep=2, radius=4, T=203), b"exceeds 32767")          # 2 * 81 * 203 = 32886
    refused(volume(n_sources=8, keep=8, radius=4, T=51), b"exceeds 32767")           # 8 * 81 * 51 = 33048
    refused(volume(n_sources=8, keep=6, radius=4, T=255), b"exceeds 32767")
    # (2 * 81 * 202 = 32724 and 8 * 81 * 50 = 32400 fit: tests/test_sgm_gpu.py runs such a case)
    refused(aggregate(s=None), b"null pointer")
    for paths in (0, 1, 5, 7, 9, 16, -4):
        refused(aggregate(paths=paths), b"paths must be 4 or 8")
    refused(aggregate(direction=-1), b"direction")
    refused(aggregate(direction=5), b"direction")
    refused(aggregate(paths=8, direction=9), b"direction")
    refused(aggregate(p1=0), b"penalties")
    refused(aggregate(p1=81), b"penalties")
    refused(aggregate(p2=32768), b"penalties")
    refused(aggregate(p1=-5, p2=-1), b"penalties")
    refused(aggregate(h=0), b"frame size")
    refused(aggregate(w=32769, n_volume=1 << 40), b"frame size")
    refused(aggregate(h=7), b"volume smaller")
    refused(select(depth=None), b"null pointer")
    refused(select(q=-1), b"uniqueness")
    refused(select(q=101), b"uniqueness")
    for field, value, text in (("offset", 97, b"past the end"), ("w", 0, b"frame size"), ("focal", 0.0, b"focal"), ("ppx", float("inf"), b"non-finite")):
        saved = getattr(table[0], field)
        setattr(table[0], field, value)
        for call in (volume, select):
            refused(call(), text)
        setattr(table[0], field, saved)
    table[2].m[7] = float("inf")                                 # a source's row: the volume reads it, the selection does not
    refused(volume(), b"non-finite")


def test_cli_refusals(tmp_path):
    from acezero_amd import cli
    pose_file, images = MC.write_scene(str(tmp_path), 3)
    base = [pose_file, images, str(tmp_path / "depth"), "--depth_range", "1", "3"]
    for extra, text in ((["--sgm_paths", "8"], "need --aggregation sgm"),
                        (["--sgm_p1", "10"], "need --aggregation sgm"),
                        (["--aggregation", "none", "--sgm_p2", "10"], "need --aggregation sgm"),
                        (["--aggregation", "sgm", "--sgm_p1", "0"], "1 <= P1 <= P2 <= 32767"),
                        (["--aggregation", "sgm", "--sgm_p1", "700", "--sgm_p2", "640"], "1 <= P1 <= P2 <= 32767"),
                        (["--aggregation", "sgm", "--sgm_p1", "32768"], "1 <= P1 <= P2 <= 32767"),
                        (["--aggregation", "sgm", "--sgm_p2", "32768"], "1 <= P1 <= P2 <= 32767")):
        with pytest.raises(SystemExit, match=text):
            cli.estimate_depth_main(base + extra)
    for extra in (["--aggregation", "median"], ["--aggregation", "sgm", "--sgm_paths", "6"]):
        with pytest.raises(SystemExit):
            cli.estimate_depth_main(base + extra)                # argparse's own refusal
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match="needs a GPU"):     # as without the flag
            cli.estimate_depth_main(base + ["--aggregation", "sgm", "--sgm_paths", "8", "--sgm_p1", "20", "--sgm_p2", "300"])
