"""CPU: the frame table of fusion and stereo (acezero_amd/frames.py): packing, rows and the cut into calls are host logic, run here on
the CPU device. Every expected value is written out from the definition (include/acez.h section K: the acez_tsdf_frame row)."""
import numpy as np
import pytest
import torch

from acezero_amd import _native as N
from acezero_amd.frames import calls, frame_rows, pack

CPU = torch.device("cpu")
SIZES = [(60, 80), (80, 60), (60, 80), (80, 60), (60, 80)]       # tests/test_fusion_gpu.py's mixed frames
FOCALS = [70.0, 65.0, 40.0, 900.0, 70.0]
OFFSETS = [0, 4800, 9600, 14400, 19200]                           # running sums of h * w


def mixed_depths():
    rng = np.random.default_rng(11)
    return [rng.integers(0, 65536, size, dtype=np.uint16) for size in SIZES]


def poses(n):
    """n rigid camera -> world poses, float64 [n,4,4]: a rotation about a skew axis and a translation, both growing with the frame."""
    out = np.tile(np.eye(4), (n, 1, 1))
    for f in range(n):
        a = 0.3 + 0.4 * f
        rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        rx = np.array([[1, 0, 0], [0, np.cos(0.5 * a), -np.sin(0.5 * a)], [0, np.sin(0.5 * a), np.cos(0.5 * a)]])
        out[f, :3, :3], out[f, :3, 3] = rz @ rx, (0.1 * f, -0.2, 1.0 + f)
    return out


def test_a_list_of_mixed_sizes_is_concatenated():
    depths = mixed_depths()
    flat, sizes, offsets = pack(depths, np.uint16, (), CPU)
    assert sizes == SIZES and offsets == OFFSETS
    assert flat.dtype == torch.int16 and flat.shape == (24000,)
    assert np.array_equal(flat.numpy().view(np.uint16), np.concatenate([d.reshape(-1) for d in depths]))
    small = [np.zeros(s, np.uint8) + k for k, s in enumerate([(2, 3), (4, 1), (1, 5)])]       # frames of unequal areas
    flat, sizes, offsets = pack(small, np.uint8, (), CPU)
    assert sizes == [(2, 3), (4, 1), (1, 5)] and offsets == [0, 6, 10] and flat.tolist() == [0] * 6 + [1] * 4 + [2] * 5
    rgb = [np.full(s + (3,), k, np.uint8) for k, s in enumerate(SIZES)]
    flat, sizes, offsets = pack(rgb, np.uint8, (3,), CPU)
    assert sizes == SIZES and offsets == OFFSETS and flat.shape == (72000,)                     # offsets count pixels, not bytes
    flat, sizes, offsets = pack([], np.uint16, (), CPU)
    assert flat.shape == (0,) and sizes == [] and offsets == []


def test_a_tensor_is_taken_as_it_lies():
    stack = np.stack([d for d, s in zip(mixed_depths(), SIZES) if s == (60, 80)] * 2)[:5]       # 5 frames of 60 x 80
    for tensor in (torch.from_numpy(stack.view(np.int16)), torch.from_numpy(stack)):           # the bits as int16, or uint16 itself
        flat, sizes, offsets = pack(tensor, np.uint16, (), CPU)
        assert sizes == [(60, 80)] * 5 and offsets == [0, 4800, 9600, 14400, 19200]
        assert flat.dtype == torch.int16 and np.array_equal(flat.numpy().view(np.uint16), stack.reshape(-1))


def test_uint16_depth_travels_as_the_same_bits_in_int16():
    flat, _, _ = pack([np.array([[0, 1, 0x7FFF, 0x8000, 0xFFFF]], np.uint16)], np.uint16, (), CPU)
    assert flat.dtype == torch.int16 and flat.tolist() == [0, 1, 32767, -32768, -1]


def test_wrong_types_and_shapes_are_refused():
    for images, dtype, trailing in (([np.zeros((4, 5), np.float32)], np.uint16, ()),            # dtype
                                    ([np.zeros((4, 5), np.uint8)], np.uint16, ()),
                                    ([np.zeros((4, 5, 3), np.uint16)], np.uint16, ()),          # trailing shape
                                    ([np.zeros((4, 5), np.uint8)], np.uint8, (3,)),
                                    ([np.zeros((4, 5, 4), np.uint8)], np.uint8, (3,)),
                                    (torch.zeros((2, 4, 5), dtype=torch.float32), np.uint16, ()),
                                    (torch.zeros((2, 4, 5), dtype=torch.uint8), np.uint16, ()),
                                    (torch.zeros((2, 4, 5), dtype=torch.uint8), np.uint8, (3,)),
                                    (torch.zeros((2, 4, 5, 3), dtype=torch.uint8), np.uint8, ())):
        with pytest.raises(TypeError, match="expected"):
            pack(images, dtype, trailing, CPU)


def test_principal_point_defaults_to_the_image_centre():
    w2c = np.tile(np.eye(4)[:3], (5, 1, 1))
    rows = frame_rows(SIZES, OFFSETS, world_to_cam=w2c, focals=FOCALS)
    assert len(rows) == 5
    assert [(r.ppx, r.ppy) for r in rows] == [(40.0, 30.0), (30.0, 40.0), (40.0, 30.0), (30.0, 40.0), (40.0, 30.0)]      # (w / 2, h / 2)
    assert [(r.h, r.w, r.offset) for r in rows] == [(60, 80, 0), (80, 60, 4800), (60, 80, 9600), (80, 60, 14400), (60, 80, 19200)]
    assert [r.focal for r in rows] == FOCALS
    rows = frame_rows(SIZES, OFFSETS, world_to_cam=w2c, focals=525.0, ppx=31.5, ppy=[1.0, 2.0, 3.0, 4.0, 5.0])
    assert [r.focal for r in rows] == [525.0] * 5 and [r.ppx for r in rows] == [31.5] * 5                                # a scalar broadcasts
    assert [r.ppy for r in rows] == [1.0, 2.0, 3.0, 4.0, 5.0]                                                            # a list is per frame
    rows = frame_rows(SIZES[:2], OFFSETS[:2], world_to_cam=w2c[:2], focals=FOCALS[:2], length=4)                         # spare rows stay zero
    assert len(rows) == 4 and rows[1].w == 60 and rows[2].w == 0 and rows[3].focal == 0.0


def test_pose_rows_are_world_to_camera_in_float32():
    c2w = poses(5)
    w2c = np.linalg.inv(c2w)
    want = w2c[:, :3].astype(np.float32)                          # inverted in float64, rounded once
    assert (want != np.linalg.inv(c2w.astype(np.float32))[:, :3]).any(), "the poses do not tell a float32 inverse from a float64 one"
    for given in (dict(world_to_cam=w2c), dict(world_to_cam=torch.from_numpy(w2c[:, :3])), dict(cam_to_world=c2w),
                  dict(cam_to_world=torch.from_numpy(c2w)), dict(cam_to_world=c2w[:, :3])):
        rows = frame_rows(SIZES, OFFSETS, focals=FOCALS, **given)
        got = np.array([list(r.m) for r in rows], np.float32)
        assert got.tobytes() == want.reshape(5, 12).tobytes()     # row-major 3 x 4
    with pytest.raises(ValueError, match="exactly one"):
        frame_rows(SIZES, OFFSETS, focals=FOCALS)
    with pytest.raises(ValueError, match="exactly one"):
        frame_rows(SIZES, OFFSETS, world_to_cam=w2c, cam_to_world=c2w, focals=FOCALS)


def test_calls_cut_the_frames_and_restart_the_offsets():
    depths, c2w = mixed_depths(), poses(5)
    rgb = [np.full(s + (3,), k, np.uint8) for k, s in enumerate(SIZES)]
    want_m = np.linalg.inv(c2w)[:, :3].astype(np.float32).reshape(5, 12)
    cut = list(calls(depths, None, c2w, FOCALS, None, [9.0, 8.0, 7.0, 6.0, 5.0], rgb, 2, CPU))
    assert [n for *_, n in cut] == [2, 2, 1]
    first = 0
    for d_depth, d_rgb, rows, d_rows, n in cut:
        assert len(rows) == n and d_rows.numel() == n * 80 and d_rows.dtype == torch.uint8          # sizeof(acez_tsdf_frame) == 80
        assert [r.offset for r in rows] == [0, 4800][:n]
        assert [(r.h, r.w) for r in rows] == SIZES[first:first + n] and [r.focal for r in rows] == FOCALS[first:first + n]
        assert [r.ppx for r in rows] == [w / 2.0 for _, w in SIZES[first:first + n]]
        assert [r.ppy for r in rows] == [9.0, 8.0, 7.0, 6.0, 5.0][first:first + n]
        assert np.array([list(r.m) for r in rows], np.float32).tobytes() == want_m[first:first + n].tobytes()
        assert np.array_equal(d_depth.numpy().view(np.uint16), np.concatenate([d.reshape(-1) for d in depths[first:first + n]]))
        assert d_rgb.shape == (3 * 4800 * n,) and d_rgb[0] == first and d_rgb[-1] == first + n - 1
        first += n
    (d_depth, d_rgb, rows, _, n), = calls(depths, np.linalg.inv(c2w), None, FOCALS, None, None, None, 256, CPU)
    assert n == 5 and d_rgb is None and [r.offset for r in rows] == OFFSETS
    assert N.TSDF_MAX_FRAMES == 256
    for bad in (0, 257):
        with pytest.raises(ValueError, match="frames_per_call"):
            next(calls(depths, None, c2w, FOCALS, None, None, None, bad, CPU))
    with pytest.raises(ValueError, match="focals"):
        next(calls(depths, None, c2w, None, None, None, None, 2, CPU))
    with pytest.raises(ValueError, match="depth image's size"):
        next(calls(depths, None, c2w, FOCALS, None, None, rgb[1:] + rgb[:1], 2, CPU))
