"""The per-pixel criterion (tests/pixel_parity.py) against the whole-map bounds it supplements: defects confined to one border column,
one 256-row M-tile or one K stage of one tile pass the suite's older global bounds (relative L2 4e-3, max-abs 0.03 of max |ref|: the
bf16 encoder bounds of tests/test_encoder_gpu.py) on a production-sized chunk, and fail the per-pixel bound of the GPU tests."""
import functools

import pytest
import torch

from acezero_amd import synth
from oracle import encoder_oracle
from tests.pixel_parity import global_errors, pixel_errors, pixel_parity
from tests.test_encoder_forms_gpu import PIXEL

GLOBAL = (4e-3, 0.03)
REPEAT = 16            # 4 distinct 120 x 160 frames, repeated: a 64-frame chunk of 19 200 pixels (the encoder is frame-independent)


@functools.lru_cache(maxsize=None)
def _chunk(dtype):
    sd = encoder_oracle.init_weights(seed=4099)
    img = torch.from_numpy(synth.make_gray_images(seed=77, n=4, h=120, w=160))
    o = encoder_oracle.EncoderOracle(sd, dtype)
    x, res = o._trunk(img)
    ref = o._tail(x, res, (True,))[0]
    # one 32-channel K stage of res2_conv3 (input channels 64..95 of the centre tap) left out
    sd2 = dict(o.sd)
    w = sd2["res2_conv3.weight"].clone()
    w[:, 64:96, 1, 1] = 0
    sd2["res2_conv3.weight"] = w
    o2 = encoder_oracle.EncoderOracle(sd2, dtype)
    dropped = o2._tail(x, res, (True,))[0]
    return ref.repeat(REPEAT, 1, 1, 1), dropped.repeat(REPEAT, 1, 1, 1)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _from_rows(r, like):
    n, c, h, w = like.shape
    return r.view(n, h, w, c).permute(0, 3, 1, 2)


def _defect(kind, ref, dropped):
    got = ref.clone()
    n, c, h, w = ref.shape
    if kind == "border_column":
        got[5, :, :, w - 1] *= 1.01
    elif kind == "m_tile":
        # 256-row tile 37: rows 9472..9727 in (frame, y, x) order, straddling frames 31 and 32
        rows = _rows(got).clone()
        rows[37 * 256:38 * 256] *= 1.005
        got = _from_rows(rows, ref)
    elif kind == "k_stage":
        # one tile (rows 5120..5375) that skipped one 32-wide K stage of its 3 x 3 layer
        rows, rd = _rows(got).clone(), _rows(dropped)
        rows[20 * 256:21 * 256] = rd[20 * 256:21 * 256]
        got = _from_rows(rows, ref)
    return got


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["border_column", "m_tile", "k_stage"])
def test_local_defects_pass_global_bounds_and_fail_per_pixel(kind, dtype):
    ref, dropped = _chunk(dtype)
    got = _defect(kind, ref, dropped)
    got = got.to(torch.bfloat16 if dtype == "bf16" else torch.float16).float()     # a kernel stores 16-bit values
    rel, mx = global_errors(got, ref)
    assert rel < GLOBAL[0] and mx < GLOBAL[1], (rel, mx)
    pp = pixel_parity(got, ref)
    assert pp.worst > PIXEL[dtype], pp


def test_identical_maps_pass_and_the_worst_pixel_is_located():
    ref, _ = _chunk("bf16")
    pp = pixel_parity(ref, ref)
    assert pp.worst == 0.0 and pp.equal == 1.0
    got = ref.clone()
    got[9, 100:132, 7, 11] = 0
    pp = pixel_parity(got, ref)
    assert pp.where == (9, 7, 11) and pp.worst > 0.1
    assert pp.equal == 1.0 - 32 / ref.numel()
    # the floor: a pixel of near-zero norm is judged relative to the median pixel norm, not to itself
    ref2 = ref[:1].clone()
    ref2[0, :, 0, 0] = 1e-9
    got2 = ref2.clone()
    got2[0, 0, 0, 0] += 1e-6
    assert float(pixel_errors(got2, ref2).max()) < 1e-5
