"""The head on whole frames (acez_head_forward_maps -> head_maps_kernel, passes of >= 32 768 rows) per pixel against HeadOracle, in the
planar [frames, 3, h, w] layout that Regressor.forward and session registration read; batch invariance of a frame's coordinates, bitwise;
and the production chain (64 frames of 480 x 640 through encoder and head) against the form-matched oracles."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import head_oracle
from tests.pixel_parity import assert_pixel_parity

pytestmark = pytest.mark.gpu

H, W = 60, 80                       # 4800 rows per frame: the 1/8 map of a 480 x 640 frame
MEAN = torch.tensor([1.0, -2.0, 0.5])
# Worst per-pixel error of the coordinates (minus the mean) against the rounding-matched oracle. Measured on an MI355X over every case
# here: bf16 7.1e-3, fp16 1.22e-3 (two head blocks, softplus regime); the production chain 2.3e-3 / 3.4e-4. Bounds ~1.2-1.4x that.
PIXEL = {"bf16": 1e-2, "fp16": 1.5e-3}


def _feats(dtype, n_frames, seed=11):
    """[n_frames * 4800, 512] 16-bit feature rows on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    f = torch.randn(n_frames * H * W, 512, generator=g, device="cuda") * 0.5
    return f.to(torch.bfloat16 if dtype == "bf16" else torch.float16)


def _frames_cpu(rows, frames):
    """fp32 CPU copies of the rows of `frames`: [len(frames), 4800, 512]."""
    return rows.view(-1, H * W, 512)[list(frames)].float().cpu()


# Homogeneous output: s3 = fc3's fourth channel is moved into one of two regimes by scaling that row of fc3 and its bias. "softplus": s3
# spreads over ~21.6 +- 5, across the threshold of F.softplus's "big" branch (beta * s3 > 20); "clamp": s3 over ~100 +- 10, across the
# min_inv_scale clamp (softplus + max_inv_scale > 100). In both, h = s3 + 0.25 stays >= ~10, so a last-place flip in fc2's output moves a
# coordinate by no more than it moves s3 relative to itself (a spread over 0..100 puts pixels at h ~ 1, where it is amplified 100x).
REGIMES = {"softplus": (21.6, 5.0), "clamp": (100.0, 10.0)}


@functools.lru_cache(maxsize=None)
def _params(nb, homog):
    flat = head_oracle.init_params(7 + nb, nb, bool(homog)).clone()
    if homog:
        centre, spread = REGIMES[homog]
        w3 = flat.numel() - 4 - 4 * 512
        f = _feats("bf16", 1, seed=99)[:2000].float().cpu()
        s3 = head_oracle.HeadOracle(flat, MEAN, nb, True, mode="fp32").forward(f)[0][:, 3] - flat[-1]
        a = 2.0 ** round(float(np.log2(spread / float(s3.std()))))
        flat[w3 + 3 * 512:w3 + 4 * 512] *= a
        flat[-1] = centre - a * float(s3.median())
    return flat


def _maps(tr, rows, n_frames):
    out = torch.empty((n_frames, 3, H, W), dtype=torch.float32, device="cuda")
    from acezero_amd import _native as N
    N.check(tr.lib.acez_head_forward_maps(tr._h, C.c_void_p(rows.data_ptr()), n_frames, H, W, C.c_void_p(out.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out


def _trainer(dtype, nb, homog, max_batch):
    from acezero_amd.head import HeadTrainer
    tr = HeadTrainer(MEAN, num_head_blocks=nb, use_homogeneous=bool(homog), max_batch=max_batch, dtype=dtype, iterations=1, inference_only=True)
    tr.load_flat(_params(nb, homog))
    return tr


def _oracle_maps(dtype, nb, homog, feats_frames, mode=None):
    """HeadOracle coordinates of [k, 4800, 512] frames -> [k, 3, H, W], and (with homogeneous output) the branch fractions."""
    orc = head_oracle.HeadOracle(_params(nb, homog), MEAN, nb, bool(homog), mode=mode or dtype)
    s, _ = orc.forward(feats_frames.reshape(-1, 512))
    X, aux = orc.dehomogenise(s)
    frac = None
    if homog:
        h, clamped, bx = aux
        frac = {"big": float((bx > 20).double().mean()), "clamped": float(clamped.double().mean())}
    return X.view(-1, H, W, 3).permute(0, 3, 1, 2), frac


def _rel_maps(X):
    return X - MEAN.view(1, 3, 1, 1)


@pytest.mark.parametrize("homog", ["softplus", "clamp", False])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_planar_maps_match_oracle_per_pixel(dtype, nb, homog):
    rows = _feats(dtype, 64)
    tr = _trainer(dtype, nb, homog, 64 * H * W)
    try:
        m8 = _maps(tr, rows[:8 * H * W], 8).cpu()           # 38 400 rows: one whole-frame pass
        m64 = _maps(tr, rows, 64).cpu()                     # 307 200 rows
    finally:
        tr.close()
    chk8, chk64 = [0, 3, 7], [0, 63]
    ref, frac = _oracle_maps(dtype, nb, homog, _frames_cpu(rows, sorted(set(chk8 + chk64))))
    pos = {k: i for i, k in enumerate(sorted(set(chk8 + chk64)))}
    print("\n[%s nb=%d homog=%s] branches %s" % (dtype, nb, homog, frac))
    if homog:
        # the regime's de-homogenisation branch is really exercised, on some pixels and not on all
        assert 0.0 < frac["big" if homog == "softplus" else "clamped"] < 1.0, frac
    r8 = ref[[pos[k] for k in chk8]]
    r64 = ref[[pos[k] for k in chk64]]
    p8 = assert_pixel_parity(_rel_maps(m8[chk8]), _rel_maps(r8), PIXEL[dtype], "8-frame pass:")
    p64 = assert_pixel_parity(_rel_maps(m64[chk64]), _rel_maps(r64), PIXEL[dtype], "64-frame pass:")
    # every frame of the planar output was written (no frame or channel left at its initial contents)
    assert torch.isfinite(m64).all()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_frame_coordinates_do_not_depend_on_the_batch(dtype):
    """A frame's map is bitwise the same in a 64-frame pass, in a 7-frame pass that puts it at another row offset mod 128, and in a
    16-frame pass cut by max_batch = 40 000 into chunks of 40 000 and 36 800 rows (frame 8 is cut in two). A 1-frame pass (below
    32 768 rows: the per-layer path) is bounded per pixel only."""
    nb, homog = 1, "softplus"
    rows = _feats(dtype, 64, seed=23)
    fpx = H * W
    tr = _trainer(dtype, nb, homog, 64 * fpx)
    try:
        m64 = _maps(tr, rows, 64).cpu()
        m7 = _maps(tr, rows[5 * fpx:12 * fpx], 7).cpu()       # frames 5..11: frame 8 at row 14 400, frame 10 at 24 000 (both 64 mod 128)
    finally:
        tr.close()
    tr = _trainer(dtype, nb, homog, 40000)
    try:
        m16 = _maps(tr, rows[:16 * fpx], 16).cpu()           # frame 8 = rows 38 400..43 199, cut at 40 000
    finally:
        tr.close()
    tr = _trainer(dtype, nb, homog, fpx)
    try:
        m1 = _maps(tr, rows[10 * fpx:11 * fpx], 1).cpu()
    finally:
        tr.close()
    for k in (8, 10):
        assert torch.equal(m64[k], m7[k - 5]), k
        assert torch.equal(m64[k], m16[k]), k
    ref, _ = _oracle_maps(dtype, nb, homog, _frames_cpu(rows, [10]))
    p1 = assert_pixel_parity(_rel_maps(m1), _rel_maps(ref), PIXEL[dtype], "1-frame pass:")
    p64 = assert_pixel_parity(_rel_maps(m64[[10]]), _rel_maps(ref), PIXEL[dtype], "64-frame pass:")
    print("\n[%s] frame 10: 1-frame pass %s | 64-frame pass %s" % (dtype, p1, p64))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_production_chain_per_pixel(dtype):
    """Regressor(max_frames=64) on 64 frames of 480 x 640 (encoder chunk with the fused SKIP form, head on whole frames) against the
    fused_skip encoder oracle followed by HeadOracle; in fp16 also against the un-rounded fp32 oracles at 2e-3 of the coordinate scale."""
    from acezero_amd.network import Regressor
    from oracle import encoder_oracle
    from tests.test_encoder_forms_gpu import N_PROD, images, oracle_frame, weights
    from tests.test_pipeline_gpu import _head_state_dict
    hsd, flat = _head_state_dict()
    img = images(480, 640, N_PROD)[:64]
    net = Regressor.create_from_split_state_dict(weights(), hsd, max_frames=64, max_h=480, max_w=640, dtype=dtype)
    chk = [0, 1, 31, 63]
    sc = net(img)[chk].cpu()
    mean = MEAN.view(1, 3, 1, 1)
    feats = torch.cat([oracle_frame(dtype, 480, 640, N_PROD, k)[1] for k in chk])
    rows = feats.permute(0, 2, 3, 1).reshape(-1, 512)
    Xo = head_oracle.HeadOracle(flat, MEAN, 1, True, mode=dtype).scene_coordinates(rows).view(len(chk), H, W, 3).permute(0, 3, 1, 2)
    pp = assert_pixel_parity(sc - mean, Xo - mean, PIXEL[dtype], "production chain:")
    print("\n[%s] production chain vs fused_skip encoder oracle + HeadOracle: %s" % (dtype, pp))
    if dtype == "fp16":
        scale = (Xo - mean).abs().max().item()
        sub = [0, 3]     # frames 0 and 63
        img32 = img[[chk[i] for i in sub]]
        rows32 = encoder_oracle.EncoderOracle(weights(), "fp32").features_rows(img32)
        X32 = head_oracle.HeadOracle(flat, MEAN, 1, True, mode="fp32").scene_coordinates(rows32).view(len(sub), H, W, 3).permute(0, 3, 1, 2)
        err32 = (sc[sub] - X32).abs().max().item()
        print("[fp16] vs fp32 oracles: max err %.3e of scale %.3e" % (err32, scale))
        assert err32 < 2e-3 * scale, (err32, scale)
