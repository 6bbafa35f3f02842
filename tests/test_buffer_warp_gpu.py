"""acez_buffer_warp_views (warp_mean_kernel, warp_views_kernel, warp_mask_kernel of buffer_api.hip) through the C ABI with caller-built
affine maps, against tests/warp_restated.py in float64 -- the reference tests/test_warp_restated_cpu.py pins against torch's float64
affine_grid / grid_sample -- on the cases of tests/warp_cases.py: the production frame at both scales, odd sizes, a frame smaller than
the mean kernel's workgroup, identity, quarter and half turns, 45 degrees, a zoom-out that reflects up to three times, a zoom-in, every
jitter pair (none, neutral, mild, saturating brightness, zero contrast, strong contrast), repeated and non-monotone frame indices.

Bounds (tests/warp_cases.py; r measured on the restatement alone, float32 against float64, asserted on the CPU):
  pixels  |gpu - ref| <= k (L eps32 max(H, W) g + eps32 max|tap|)   r = 2.00 (recorded ceiling 2.01), k = 4 max(1, r) = 8.04
  mean    |gpu - ref| <= k eps32 (H W / 1024 + 22)                  r = 0.038 (ceiling 0.04),         k = 4
  mask    a cell may differ only if its float64 source coordinate is within tau = k_pixel eps32 max(H, W) g of -1, W, -1 or H
with g the largest absolute entry of the map's linear part (at least 1), L the largest difference between horizontally and between
vertically adjacent taps of the cell (of every cell within tau of the coordinate: next to a cell border the device may read the
neighbouring cell), max|tap| the largest absolute value of the view's source frame after jitter (the jitter ends in (g - 0.4) / 0.25,
whose rounding does not shrink with the tap). No pixel is exempt. The reference is evaluated with the device's own per-view means, so
a mean inside its bound cannot widen the pixels'."""
import ctypes as C

import numpy as np
import pytest
import torch

from acezero_amd import _native as N
from tests import warp_cases as cases
from tests import warp_restated as R

pytestmark = pytest.mark.gpu

GUARD = 64   # poisoned elements behind every output


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _call(c, mh, mw):
    """One call on case c with an mh x mw mask. Returns (views [B,hs,ws], mask [B,mh,mw], means [B] or None) as numpy."""
    B, hs, ws = len(c["index"]), c["hs"], c["ws"]
    dev = "cuda"
    img = torch.from_numpy(c["images"]).to(dev).contiguous()
    idx = torch.from_numpy(c["index"]).to(dev)
    th = torch.from_numpy(c["theta"]).to(dev)
    jt = torch.from_numpy(c["jitter"]).to(dev).contiguous() if c["jitter"] is not None else None
    out = torch.full((B * hs * ws + GUARD,), float("nan"), device=dev)
    msk = torch.full((B * mh * mw + GUARD,), 77, dtype=torch.uint8, device=dev)
    scr = torch.full((B + GUARD,), float("nan"), device=dev)
    N.check(N.lib().acez_buffer_warp_views(_p(img), img.shape[0], c["H"], c["W"], _p(idx), _p(th), _p(jt), B, hs, ws, _p(out), _p(msk), mh, mw,
                                           _p(scr), None))
    torch.cuda.synchronize()
    out, msk, scr = out.cpu().numpy(), msk.cpu().numpy(), scr.cpu().numpy()
    assert np.isnan(out[B * hs * ws:]).all() and (msk[B * mh * mw:] == 77).all() and np.isnan(scr[B:]).all()   # nothing behind the outputs
    if jt is None:
        assert np.isnan(scr).all()                                       # the mean kernel does not run
    assert set(np.unique(msk[:B * mh * mw])) <= {0, 1}
    return out[:B * hs * ws].reshape(B, hs, ws), msk[:B * mh * mw].reshape(B, mh, mw), (scr[:B] if jt is not None else None)


@pytest.mark.parametrize("with_jitter", [False, True])
@pytest.mark.parametrize("name", cases.GEOMETRIES)
def test_warp_matches_the_float64_restatement_per_pixel(name, with_jitter):
    c = cases.case(name, with_jitter)
    H, W, hs, ws = c["H"], c["W"], c["hs"], c["ws"]
    (fh, fw), full = cases.mask_sizes(c)
    views, mask_f, means = _call(c, fh, fw)
    views2, mask_full, _ = _call(c, *full)
    assert np.array_equal(views, views2)                                 # (the second call only asks for another mask size)
    worst_mean = 0.0
    if with_jitter:
        ref_m = np.array([R.jitter_mean(c["images"][i], b) for i, b in zip(c["index"], c["jitter"][:, 0])])
        d = np.abs(means.astype(np.float64) - ref_m)
        worst_mean = float(d.max() / (cases.K_MEAN * cases.mean_bracket(c)))
        assert worst_mean <= 1.0, (worst_mean, c["names"][int(d.argmax())])
    ref, L, tapmax = R.warp(c["images"], c["index"], c["theta"], c["jitter"], means, hs, ws, tau=cases.mask_tau(c))
    assert np.isfinite(views).all()
    ratio = np.abs(views.astype(np.float64) - ref) / (cases.K_PIXEL * cases.pixel_bracket(c, L, tapmax))
    at = np.unravel_index(int(ratio.argmax()), ratio.shape)
    excused = 0
    for got, (mh, mw) in ((mask_f, (fh, fw)), (mask_full, full)):
        want, dist = R.mask(c["theta"], H, W, hs, ws, mh, mw)
        differ = (got != 0) != want
        excused += int(differ.sum())
        assert (dist[differ] < np.broadcast_to(cases.mask_tau(c)[:, None, None], dist.shape)[differ]).all(), (mh, mw, int(differ.sum()))
    for v, nm in enumerate(c["names"]):
        if nm.startswith("zoom_in"):
            assert mask_f[v].all() and mask_full[v].all()
    print(f"warp {name} jitter={with_jitter}: worst pixel error / bound {ratio.max():.3f} at {c['names'][at[0]]} {tuple(int(i) for i in at[1:])}, "
          f"mean error / bound {worst_mean:.3f}, mask cells excused {excused}")
    assert ratio.max() <= 1.0, (float(ratio.max()), c["names"][at[0]], at[1:])
