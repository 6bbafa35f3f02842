"""The encoder's kernel forms at the sizes where the default tiling picks them, per pixel against the oracle of the form that ran.

launch_convgemm picks a form from the row count M = frames * ho * wo (480 x 640: 4800 rows per frame): res2_conv3 + res2_skip fused
(conv3x3r, SKIP) from 7 frames on, res1_conv1 + res1_conv2 back to back (B2B) and res1_conv3 with its residual (HAS_ADD) on conv3x3r
from 14 frames on, below that two launches. The fused SKIP form adds the unrounded skip product to res2_conv3's accumulators and rounds
once, so its oracle is EncoderOracle(..., fused_skip=True); B2B and HAS_ADD round where the unfused stores do. Every comparison is per
pixel (tests/pixel_parity.py) and records the fraction of elements bitwise equal to the oracle: that fraction is clearly higher against
the oracle of the form that ran, which pins the form.

Oracle frames are encoded once per (dtype, image set, frame) and shared by the tests of this module and tests/test_head_maps_gpu.py.
"""
import functools

import pytest
import torch

from acezero_amd import synth
from oracle import encoder_oracle
from tests.pixel_parity import assert_pixel_parity, global_errors, pixel_parity

pytestmark = pytest.mark.gpu

# Worst per-pixel error against the oracle of the form that ran. Measured on an MI355X over every case of this module and of
# tests/test_encoder_gpu.py: bf16 2.94e-3, fp16 3.91e-4 (both a 1-frame pass against the unfused oracle); bounds ~1.3x that.
PIXEL = {"bf16": 4e-3, "fp16": 5e-4}
# worst per-pixel difference between a frame encoded in a 64-frame chunk and alone (measured: bf16 2.69e-3, fp16 3.55e-4)
BATCH = {"bf16": 4e-3, "fp16": 5e-4}
# the bitwise-equal fraction against the form-matched oracle exceeds the other form's by at least this much (measured: bf16 0.10-0.11,
# fp16 0.07-0.09)
FORM_MARGIN = 0.04
CHECK = (0, 1, 31, 63)      # frame 1 starts at row 4800, 18.75 256-row tiles in


@functools.lru_cache(maxsize=None)
def weights():
    return encoder_oracle.init_weights(seed=4099)


@functools.lru_cache(maxsize=None)
def images(h, w, n):
    return torch.from_numpy(synth.make_gray_images(seed=1000 + w, n=n, h=h, w=w))


@functools.lru_cache(maxsize=None)
def oracle_frame(dtype, h, w, n, k):
    """(unfused, fused_skip) oracle features [1, 512, ho, wo] of frame k of images(h, w, n)."""
    return tuple(encoder_oracle.EncoderOracle(weights(), dtype).forward_variants(images(h, w, n), frames=[k]))


def oracle_frames(dtype, h, w, n, frames, fused):
    return torch.cat([oracle_frame(dtype, h, w, n, k)[1 if fused else 0] for k in frames])


def encode(dtype, img, max_frames, tile=None, monkeypatch=None):
    from acezero_amd.encoder import Encoder
    if tile is not None:
        monkeypatch.setenv("ACEZ_CONV_TILE", tile)   # read when the context is created
    h, w = img.shape[-2:]
    enc = Encoder(weights(), max_frames=max_frames, max_h=h, max_w=w, dtype=dtype)
    try:
        return enc(img)
    finally:
        enc.close()


def _forms(out, dtype, h, w, n, frames):
    ref_u = oracle_frames(dtype, h, w, n, frames, False)
    ref_f = oracle_frames(dtype, h, w, n, frames, True)
    return pixel_parity(out, ref_u), pixel_parity(out, ref_f), ref_u, ref_f


N_PROD = 70   # the production chunk is frames 0..63; the chunking test encodes all 70


@functools.lru_cache(maxsize=None)
def production_chunk(dtype):
    """Features of frames CHECK of a 64-frame 480 x 640 chunk at the default tiling (product library)."""
    out = encode(dtype, images(480, 640, N_PROD)[:64], 64)
    return out[list(CHECK)].cpu()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_production_chunk_runs_the_fused_skip_form(dtype):
    out = production_chunk(dtype)
    pu, pf, ref_u, ref_f = _forms(out, dtype, 480, 640, N_PROD, CHECK)
    print("\n[%s] 64 x 480x640 vs fused_skip oracle: %s\n[%s] 64 x 480x640 vs unfused oracle: %s" % (dtype, pf, dtype, pu))
    assert_pixel_parity(out, ref_f, PIXEL[dtype], "production chunk vs fused_skip oracle:")
    assert pf.equal > pu.equal + FORM_MARGIN, (pf, pu)
    if dtype == "fp16":
        # the plain fp16 oracle is pinned to the reference's autocast: the reference bounds hold for the fused form as well
        rel, mx = global_errors(out, ref_u)
        print("[fp16] vs autocast-pinned oracle: rel L2 %.3e, max-abs %.3e" % (rel, mx))
        assert rel < 5e-4 and mx < 4e-3, (rel, mx)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_single_frame_pass_runs_unfused_and_stays_near_the_chunk(dtype):
    img = images(480, 640, N_PROD)
    out = torch.cat([encode(dtype, img[k:k + 1], 1).cpu() for k in CHECK])
    pu, pf, ref_u, _ = _forms(out, dtype, 480, 640, N_PROD, CHECK)
    print("\n[%s] 1-frame passes vs unfused oracle: %s (vs fused_skip: %s)" % (dtype, pu, pf))
    assert_pixel_parity(out, ref_u, PIXEL[dtype], "1-frame pass vs unfused oracle:")
    assert pu.equal > pf.equal + FORM_MARGIN, (pu, pf)
    # features depend on the batch around a frame (documented): bounded, not bitwise
    pb = assert_pixel_parity(out, production_chunk(dtype), BATCH[dtype], "1-frame pass vs 64-frame chunk:")
    print("[%s] 1-frame pass vs 64-frame chunk: %s" % (dtype, pb))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("w, fused", [(760, True), (768, False)])   # wo = 95: the 448-row patch slot is exactly full; wo = 96: fallback
def test_conv3x3r_width_limit(w, fused, dtype):
    n = 12                  # 68 400 rows at wo = 95: SKIP, B2B and HAS_ADD all on conv3x3r
    out = encode(dtype, images(480, w, n), n)
    chk = (0, n - 1)
    out = out[list(chk)].cpu()
    pu, pf, ref_u, ref_f = _forms(out, dtype, 480, w, n, chk)
    print("\n[%s] 12 x 480x%d vs unfused: %s | vs fused_skip: %s" % (dtype, w, pu, pf))
    assert out.shape[-1] == w // 8
    assert_pixel_parity(out, ref_f if fused else ref_u, PIXEL[dtype], "480x%d:" % w)
    if fused:
        assert pf.equal > pu.equal + FORM_MARGIN, (pf, pu)
    else:
        assert pu.equal > pf.equal + FORM_MARGIN, (pu, pf)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("h", [48, 33])     # ho = 6, 5: every 256-row tile straddles frames, ragged last tile
def test_forced_conv3x3r_at_the_width_limit(h, dtype, monkeypatch, diag_lib):
    n, w = 3, 760
    img = images(h, w, n)
    out = encode(dtype, img, n, tile="3", monkeypatch=monkeypatch).cpu()
    ref_u, ref_f = encoder_oracle.EncoderOracle(weights(), dtype).forward_variants(img)
    pf, pu = pixel_parity(out, ref_f), pixel_parity(out, ref_u)
    print("\n[%s] forced conv3x3r %dx%d vs fused_skip: %s | vs unfused: %s" % (dtype, h, w, pf, pu))
    assert_pixel_parity(out, ref_f, PIXEL[dtype], "forced conv3x3r %dx%d:" % (h, w))
    assert pf.equal > pu.equal + FORM_MARGIN, (pf, pu)


def test_chunking_runs_each_chunk_in_its_own_form():
    """Encoder(max_frames=64) on 70 frames: a chunk of 64 (fused SKIP), then a chunk of 6 (28 800 rows: every layer unfused)."""
    dtype = "bf16"
    img = images(480, 640, N_PROD)
    full = encode(dtype, img, 64)
    # the first chunk is the production chunk itself
    assert torch.equal(full[list(CHECK)].cpu(), production_chunk(dtype))
    out = full[[63, 64, 69]].cpu()
    del full
    ref = torch.cat([oracle_frame(dtype, 480, 640, N_PROD, 63)[1], oracle_frame(dtype, 480, 640, N_PROD, 64)[0],
                     oracle_frame(dtype, 480, 640, N_PROD, 69)[0]])
    pp = assert_pixel_parity(out, ref, PIXEL[dtype], "70 frames in chunks of 64:")
    print("\n[bf16] 70 frames, frames 63 (fused) / 64, 69 (unfused): %s" % pp)
    p2u, p2f, _, _ = _forms(out[1:], dtype, 480, 640, N_PROD, (64, 69))
    assert p2u.equal > p2f.equal + FORM_MARGIN, (p2u, p2f)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_ten_frame_chunk_mixes_fused_skip_with_unfused_layers(dtype):
    """48 000 rows: res2_conv3 + res2_skip on conv3x3r (SKIP), res1's layers in two launches; the last frame ends in a ragged tile."""
    n = 10
    out = encode(dtype, images(480, 640, N_PROD)[:n], n)
    chk = (1, 9)
    out = out[list(chk)].cpu()
    pu, pf, ref_u, ref_f = _forms(out, dtype, 480, 640, N_PROD, chk)
    print("\n[%s] 10-frame chunk vs fused_skip: %s | vs unfused: %s" % (dtype, pf, pu))
    assert_pixel_parity(out, ref_f, PIXEL[dtype], "10-frame chunk:")
    assert pf.equal > pu.equal + FORM_MARGIN, (pf, pu)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_forced_80_row_tiles_flip_the_form_ordering(dtype, monkeypatch, diag_lib):
    """Dispatch sensitivity: with every layer forced onto the 80-row kernels (no conv3x3r, no fusion) the production chunk's
    bitwise-equal ordering flips to the unfused oracle -- the production-chunk assertion sees which form runs."""
    out = encode(dtype, images(480, 640, N_PROD)[:64], 64, tile="80", monkeypatch=monkeypatch)
    out = out[list(CHECK)].cpu()
    pu, pf, ref_u, _ = _forms(out, dtype, 480, 640, N_PROD, CHECK)
    print("\n[%s] ACEZ_CONV_TILE=80 64 x 480x640 vs unfused: %s | vs fused_skip: %s" % (dtype, pu, pf))
    assert_pixel_parity(out, ref_u, PIXEL[dtype], "forced 80-row tiles:")
    assert pu.equal > pf.equal + FORM_MARGIN, (pu, pf)
