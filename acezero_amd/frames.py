"""The frame table that fusion and stereo hand to their entry points (include/acez.h sections K, K2, L, M: acez_tsdf_frame rows), and
the packed image buffer the rows' offsets point into. Host logic only: pack() uploads to whatever torch device it is given."""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from ._device import no_cpu


def _w2c34(world_to_cam, cam_to_world, n):
    """float32 [n,3,4] world -> camera rows; a camera -> world input is inverted in float64 and rounded once."""
    if (world_to_cam is None) == (cam_to_world is None):
        raise ValueError("give exactly one of world_to_cam and cam_to_world")
    src = world_to_cam if cam_to_world is None else cam_to_world
    m = np.asarray(src.detach().cpu().numpy() if torch.is_tensor(src) else src, np.float64).reshape(n, -1, 4)
    if cam_to_world is not None:
        full = np.tile(np.eye(4), (n, 1, 1))
        full[:, :m.shape[1]] = m
        m = np.linalg.inv(full)
    return np.ascontiguousarray(m[:, :3].astype(np.float32))


def _per_frame(value, n):
    return np.broadcast_to(np.asarray(value, np.float64), (n,))


def pack(images, dtype, trailing, device):
    """One tensor [n,h,w(,3)] or a list of per-frame arrays whose sizes may differ -> (flat tensor on `device`, [(h, w)], element
    offsets). dtype: np.uint8, or np.uint16, which travels as the same bits in int16 (torch has no arithmetic on uint16 and needs
    none here); trailing: () or (3,)."""
    if torch.is_tensor(images):
        if images.dtype in (torch.uint16, torch.int16) and dtype == np.uint16:
            images = images.view(torch.int16)
        elif not (images.dtype == torch.uint8 and dtype == np.uint8):
            raise TypeError(f"expected a {np.dtype(dtype).name} tensor, got {images.dtype}")
        if images.dim() != 3 + len(trailing) or tuple(images.shape[3:]) != trailing:
            raise TypeError(f"expected a tensor [n,h,w{',3' if trailing else ''}], got {tuple(images.shape)}")
        n, h, w = images.shape[:3]
        return images.to(device).contiguous().reshape(-1), [(h, w)] * n, [i * h * w for i in range(n)]
    arrays = [np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a) for a in images]
    sizes, offsets, at = [], [], 0
    for a in arrays:
        if a.dtype != dtype or a.ndim != 2 + len(trailing) or tuple(a.shape[2:]) != trailing:
            raise TypeError(f"expected {np.dtype(dtype).name} [h,w{',3' if trailing else ''}] arrays, got {a.dtype} {a.shape}")
        sizes.append(a.shape[:2])
        offsets.append(at)
        at += a.shape[0] * a.shape[1]
    flat = np.concatenate([a.reshape(-1) for a in arrays]) if arrays else np.zeros(0, dtype)
    if dtype == np.uint16:
        flat = flat.view(np.int16)
    return torch.from_numpy(flat).to(device), sizes, offsets


def _fill_rows(sizes, offsets, w2c, focals, ppx, ppy, length=None):
    """frame_rows() on arguments that are per frame already: w2c float32 [n,3,4], focals [n], ppx / ppy [n] or None."""
    rows = (N.TsdfFrame * (len(sizes) if length is None else length))()
    for f, (h, w) in enumerate(sizes):
        row = rows[f]
        row.m[:] = w2c[f].reshape(12).tolist()
        row.focal = float(focals[f])
        row.ppx = float(ppx[f]) if ppx is not None else w / 2.0
        row.ppy = float(ppy[f]) if ppy is not None else h / 2.0
        row.h, row.w, row.offset = int(h), int(w), int(offsets[f])
    return rows


def frame_rows(sizes, offsets, world_to_cam=None, cam_to_world=None, focals=None, ppx=None, ppy=None, length=None):
    """The table of the frames pack() laid out: a ctypes array of `length` (default: the number of frames) TsdfFrame rows. focals, ppx,
    ppy: pixels, one number or one per frame; the principal point defaults to the image centre (w / 2, h / 2)."""
    n = len(sizes)
    ppx, ppy = (None if p is None else _per_frame(p, n) for p in (ppx, ppy))
    return _fill_rows(sizes, offsets, _w2c34(world_to_cam, cam_to_world, n), _per_frame(focals, n), ppx, ppy, length)


def device_rows(length, device):
    """The device scratch an entry point copies `length` rows into."""
    return torch.empty(length * C.sizeof(N.TsdfFrame), dtype=torch.uint8, device=device)


def calls(depth_u16, world_to_cam, cam_to_world, focals, ppx, ppy, rgb, frames_per_call, device):
    """The frames of a fusion call cut into runs of frames_per_call, each packed on its own (its offsets start at 0): yields
    (d_depth, d_rgb or None, table rows, device scratch for them, number of frames)."""
    n = len(depth_u16)
    if not 1 <= int(frames_per_call) <= N.TSDF_MAX_FRAMES:
        raise ValueError(f"frames_per_call must be in 1 .. {N.TSDF_MAX_FRAMES}")
    if focals is None:
        raise ValueError("focals is required")
    w2c = _w2c34(world_to_cam, cam_to_world, n)
    focals = _per_frame(focals, n)
    ppx = None if ppx is None else _per_frame(ppx, n)
    ppy = None if ppy is None else _per_frame(ppy, n)
    for images in (depth_u16, rgb):
        if torch.is_tensor(images) and images.device.type != device.type:
            raise no_cpu("TSDFVolume.integrate", "TSDF fusion is a HIP kernel")
    for lo in range(0, n, int(frames_per_call)):
        part = slice(lo, min(n, lo + int(frames_per_call)))
        d_depth, sizes, offsets = pack(depth_u16[part], np.uint16, (), device)
        d_rgb = None
        if rgb is not None:
            d_rgb, rgb_sizes, _ = pack(rgb[part], np.uint8, (3,), device)
            if rgb_sizes != sizes:
                raise ValueError("every colour image must have its depth image's size")
        rows = _fill_rows(sizes, offsets, w2c[part], focals[part], None if ppx is None else ppx[part], None if ppy is None else ppy[part])
        yield d_depth, d_rgb, rows, device_rows(len(sizes), device), len(sizes)
