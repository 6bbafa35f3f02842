"""CPU: pins tests/warp_restated.py, the float64 reference of the view-warp kernels that tests/test_buffer_warp_gpu.py compares the
device with, on every case of tests/warp_cases.py: it equals torch's float64 affine_grid / grid_sample with reflection padding (and
session.warp_views' jitter and mask expressions in float64) to 1e-12 of the value range; its float32 evaluation stays within the
recorded ratio r of the bound's bracket (so the k = 4 max(1, r) of the GPU test cannot widen silently); and the cases keep away from
the mask's limits and reach every flip count of the reflection."""
import numpy as np
import pytest
import torch

from tests import warp_cases as cases
from tests import warp_restated as R

ALL = [(n, j) for n in cases.GEOMETRIES for j in (False, True)]


def _means(c, dt):
    if c["jitter"] is None:
        return None
    return np.array([R.jitter_mean(c["images"][i], b, dt) for i, b in zip(c["index"], c["jitter"][:, 0])], dt)


@pytest.mark.parametrize("name,with_jitter", ALL)
def test_restatement_equals_torch_float64(name, with_jitter):
    c = cases.case(name, with_jitter)
    H, W, hs, ws = c["H"], c["W"], c["hs"], c["ws"]
    B = len(c["index"])
    src = torch.from_numpy(c["images"][c["index"]]).double()[:, None]
    theta = torch.from_numpy(c["theta"]).double().view(B, 2, 3)
    grid = torch.nn.functional.affine_grid(theta, (B, 1, hs, ws), align_corners=False)
    means = _means(c, np.float64)
    if with_jitter:                                                      # session.warp_views' expressions, in float64
        br = torch.from_numpy(c["jitter"][:, 0]).double().reshape(B, 1, 1, 1)
        ct = torch.from_numpy(c["jitter"][:, 1]).double().reshape(B, 1, 1, 1)
        g = ((src * 0.25 + 0.4) * br).clamp(0, 1)
        m = g.mean(dim=(1, 2, 3), keepdim=True)
        assert np.abs(m.reshape(B).numpy() - means).max() <= 1e-14
        g = ((g - m) * ct + m).clamp(0, 1)
        src = (g - 0.4) / 0.25
    want = torch.nn.functional.grid_sample(src, grid, mode="bilinear", padding_mode="reflection", align_corners=False)[:, 0].numpy()
    got, L, tapmax = R.warp(c["images"], c["index"], c["theta"], c["jitter"], means, hs, ws)
    span = float(c["images"].max() - c["images"].min())
    assert np.abs(got - want).max() <= 1e-12 * span
    assert (L >= 0).all() and (tapmax <= np.abs(c["images"]).max() * 4 + 1e-9).all()
    # the mask rule of session.warp_views on the same grid, at full resolution and at the cells the nearest-neighbour resize reads
    ix, iy = ((grid[..., 0] + 1) * W - 1) / 2, ((grid[..., 1] + 1) * H - 1) / 2
    rule = ((ix > -1) & (ix < W) & (iy > -1) & (iy < H)).numpy()
    from acezero_amd.encoder import output_size
    assert cases.mask_sizes(c)[0] == output_size(hs, ws)                 # the feature map production asks the mask for
    for mh, mw in cases.mask_sizes(c):
        ys, xs = R.mask_pixels(hs, ws, mh, mw)
        m, dist = R.mask(c["theta"], H, W, hs, ws, mh, mw)
        assert np.array_equal(m, rule[:, ys][:, :, xs])
        yf, xf = R.mask_pixels_f32(hs, ws, mh, mw)                       # the kernel's float32 pick reads the same pixels
        assert np.array_equal(ys, yf) and np.array_equal(xs, xf)
        near = dist < cases.mask_tau(c)[:, None, None]
        assert near.mean() <= cases.MASK_NEAR_LIMIT, (mh, mw, int(near.sum()))
    for v, nm in enumerate(c["names"]):
        if nm.startswith("zoom_in"):
            assert R.mask(c["theta"][v:v + 1], H, W, hs, ws, hs, ws)[0].all()


@pytest.mark.parametrize("name", ["special", "odd", "small"])
def test_zoom_out_reaches_every_flip_count(name):
    c = cases.case(name, False)
    v = c["names"].index("zoom_out")
    ix, iy = R.source_coords(c["theta"][v:v + 1], c["H"], c["W"], c["hs"], c["ws"])
    assert set(np.unique(R.reflect_flips(ix, c["W"]))) == {0, 1, 2, 3}
    assert {0, 1, 2} <= set(np.unique(R.reflect_flips(iy, c["H"])))
    assert (ix < -0.5).any() and (iy < -0.5).any()                       # both sides of the frame


def test_reflect_clip_on_known_points():
    """size 4, mirrors at -0.5 and 3.5, worked by hand: 4.5 -> 2.5; 9 -> -2 -> 1; 13 -> -6 -> 5 -> 2; -2 -> 1; -6 -> 5 -> 2; -10 -> 9 -> -2 -> 1;
    3.75 -> 3.25 and -0.75 -> -0.25 leave [0, 3] and are clipped."""
    x = np.array([0.0, 1.25, 3.0, 4.5, 9.0, 13.0, -2.0, -6.0, -10.0, 3.75, -0.75, 3.5, -0.5])
    want = np.array([0.0, 1.25, 3.0, 2.5, 1.0, 2.0, 1.0, 2.0, 1.0, 3.0, 0.0, 3.0, 0.0])
    assert np.array_equal(R.reflect_clip(x, 4), want)
    assert np.array_equal(R.reflect_clip(x, 4, np.float32), want.astype(np.float32))
    assert np.array_equal(R.reflect_flips(x, 4), [0, 0, 0, 1, 2, 3, 0, 1, 2, 1, 0, 1, 0])


def test_float32_restatement_stays_inside_the_recorded_ratio():
    """r of tests/warp_cases.py: the float32 evaluation of the restatement (the kernels' operation order) against the float64 one, as a
    multiple of the bracket of the GPU test's bound, over every pixel and every view mean of every case."""
    r_pix, r_mean = 0.0, 0.0
    for name, with_jitter in ALL:
        c = cases.case(name, with_jitter)
        m32 = _means(c, np.float32)
        if with_jitter:
            d = np.abs(m32.astype(np.float64) - _means(c, np.float64))
            r_mean = max(r_mean, float(d.max() / cases.mean_bracket(c)))
        v64, L, tapmax = R.warp(c["images"], c["index"], c["theta"], c["jitter"], m32, c["hs"], c["ws"], tau=cases.mask_tau(c))   # the same means in both
        v32, _, _ = R.warp(c["images"], c["index"], c["theta"], c["jitter"], m32, c["hs"], c["ws"], np.float32)
        assert v32.dtype == np.float32
        d, br = np.abs(v32.astype(np.float64) - v64), cases.pixel_bracket(c, L, tapmax)
        assert (d[br == 0] == 0).all()                                   # four taps that are exactly 0
        ratio = d / np.where(br > 0, br, 1.0)
        at = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print(f"{name} jitter={with_jitter}: r_pixel {ratio.max():.3f} at {c['names'][at[0]]} {tuple(int(i) for i in at[1:])}")
        r_pix = max(r_pix, float(ratio.max()))
    print(f"r_pixel {r_pix:.6f} r_mean {r_mean:.6f}")                    # (shown with pytest -s)
    assert r_pix <= cases.R_PIXEL and r_mean <= cases.R_MEAN
    assert r_pix >= 0.5 * cases.R_PIXEL and r_mean >= 0.5 * cases.R_MEAN   # the record is the measurement, not a loose ceiling
    assert cases.K_PIXEL == 4.0 * max(1.0, cases.R_PIXEL) and cases.K_MEAN == 4.0 * max(1.0, cases.R_MEAN)
