"""Per-pixel parity of feature / coordinate maps against an oracle.

Global bounds (relative L2, max-abs over a whole map) dilute a local defect -- a wrong border column, one ragged 256-row M-tile, a
block of channels in one tile -- among ~10^5 correct pixels. Here every pixel is judged on its own:

    err_p = ||got_p - ref_p|| / max(||ref_p||, median_q ||ref_q||)

(the norm over the channel axis; the median floor keeps near-zero pixels from turning a last-place flip into a large relative error),
and the worst pixel decides. For 16-bit outputs the fraction of elements bitwise equal to the oracle is reported too: it tells which
rounding form ran when two oracles differ only in where they round.
"""
from dataclasses import dataclass

import torch


@dataclass
class PixelParity:
    worst: float          # max over pixels of err_p
    where: tuple          # (frame, y, x) of the worst pixel
    p999: float           # 99.9th percentile of err_p
    equal: float          # fraction of elements bitwise equal to the oracle

    def __str__(self):
        return "worst %.3e at (frame, y, x) = %s, p99.9 %.3e, bitwise equal %.4f" % (self.worst, self.where, self.p999, self.equal)


def pixel_errors(got, ref):
    """got, ref: [n, C, h, w]. Returns err_p [n, h, w] (float64)."""
    assert got.shape == ref.shape and got.dim() == 4, (got.shape, ref.shape)
    g = got.detach().cpu().double()
    r = ref.detach().cpu().double()
    dn = (g - r).norm(dim=1)
    rn = r.norm(dim=1)
    floor = float(rn.flatten().median())
    return dn / rn.clamp(min=max(floor, 1e-30))


def pixel_parity(got, ref):
    e = pixel_errors(got, ref)
    n, h, w = e.shape
    i = int(e.flatten().argmax())
    where = (i // (h * w), (i // w) % h, i % w)
    flat = e.flatten().float()
    p999 = float(torch.quantile(flat, 0.999)) if flat.numel() <= 16_000_000 else float(flat.max())
    equal = float((got.detach().cpu().float() == ref.detach().cpu().float()).double().mean())
    return PixelParity(float(e.flatten()[i]), where, p999, equal)


def assert_pixel_parity(got, ref, bound, what=""):
    """Fails on the worst pixel, naming it. Returns the PixelParity record for further checks."""
    pp = pixel_parity(got, ref)
    print("%s %s" % (what, pp))       # the measured figure, shown with -s or on failure
    assert pp.worst < bound, "%s per-pixel error above %.1e: %s" % (what, bound, pp)
    return pp


def global_errors(got, ref):
    """The suite's older whole-map bounds: relative L2, and max-abs over max |ref|."""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((g - r).norm() / r.norm()), float((g - r).abs().max() / r.abs().max())
