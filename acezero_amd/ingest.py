"""Image folders onto the GPU (--gpu_ingest True): the files are decoded by a pool of threads, and resize, grey conversion and
normalisation run as the HIP kernels of csrc/ingest_api.hip (acez_ingest_frames) on the decoded uint8 RGB frames.

load_frames_device / load_session_frames_device return what cli.load_frames / cli.load_session_frames return -- the same files,
size classes, factors and errors, frames that are bit for bit the host path's -- with the float32 frames resident on the device
(ReconstructionSession moves what it is given to its device, so it takes them unchanged) and the resized uint8 RGB frames copied
back to the host. The host path stays the default; this one never falls back to it: without a device it raises."""
import concurrent.futures
import ctypes as C
import glob
import os

import numpy as np
import torch

from . import _native as N

CHUNK_FRAMES = 64               # frames of one acez_ingest_frames call, at most
CHUNK_BYTES = 256 << 20         # bytes of one pinned staging buffer, at most
MAX_WORKERS = 16
_norm = {}                      # device -> the normalisation table on it


def normalisation_table():
    """float32 [256]: cli.load_frames' own expression (g / 255, then (g - 0.4) / 0.25, in float32 numpy) applied to every grey value."""
    return (np.arange(256, dtype=np.float32) / 255.0 - 0.4) / 0.25


def pool_size(workers):
    return max(1, min(int(workers), MAX_WORKERS, len(os.sched_getaffinity(0))))


def resized_size(w, h, image_resolution):
    """(resize factor, resized height, resized width) of a w x h image: cli.load_frames' arithmetic (dataset.py:227-237)."""
    sc = image_resolution / min(w, h)
    nw, nh = (image_resolution, int(h * sc)) if w <= h else (int(w * sc), image_resolution)
    return sc, nh, nw


def axis_coeffs(in_size, out_size):
    """The library's resize table of one axis (acez_ingest_coeffs; host only): (ksize, int32 [out, 2] bounds, int32 [out, ksize] taps)."""
    lib = N.lib()
    ks = C.c_int(0)
    N.check(lib.acez_ingest_coeffs(int(in_size), int(out_size), C.byref(ks), None, None))
    bounds = np.zeros((int(out_size), 2), np.int32)
    taps = np.zeros((int(out_size), ks.value), np.int32)
    N.check(lib.acez_ingest_coeffs(int(in_size), int(out_size), C.byref(ks), bounds.ctypes.data, taps.ctypes.data))
    return ks.value, bounds, taps


def table_bytes(H, W, nh, nw):
    """Size of acez_ingest_frames' table block for H x W -> nh x nw frames."""
    lib = N.lib()
    kx, ky = C.c_int(0), C.c_int(0)
    N.check(lib.acez_ingest_coeffs(int(W), int(nw), C.byref(kx), None, None))
    N.check(lib.acez_ingest_coeffs(int(H), int(nh), C.byref(ky), None, None))
    return 4 * (nw * (2 + kx.value) + nh * (2 + ky.value))


def _decode(f, out=None):
    from PIL import Image
    try:
        a = np.asarray(Image.open(f).convert("RGB"), np.uint8)           # the host path's decode call
    except Exception as e:
        raise SystemExit(f"{f}: cannot decode image ({e})")
    if out is None:
        return a
    if a.shape != out.shape:
        raise SystemExit(f"{f}: decoded to {a.shape[:2]}, its header announced {out.shape[:2]}")
    np.copyto(out, a)
    return out


def decode_frames(files, workers=12):
    """Decode image files to uint8 [H, W, 3] RGB arrays in a pool of threads (Pillow's decoders release the GIL), in file order.
    A file that cannot be decoded raises SystemExit naming it."""
    files = list(files)
    with concurrent.futures.ThreadPoolExecutor(max_workers=pool_size(workers)) as pool:
        return list(pool.map(_decode, files))


def ingest_frames(src, nh, nw, want_rgb=True, out_grey=None):
    """One acez_ingest_frames call on the current stream. src: device uint8 [n, H, W, 3]. Returns (float32 [n, 1, nh, nw], uint8
    [n, nh, nw, 3] or None), both on src's device; out_grey: a contiguous float32 [n, 1, nh, nw] device tensor to write instead."""
    if not src.is_cuda:
        raise RuntimeError("ingest_frames needs device frames: the resize is HIP only (no CPU fallback)")
    assert src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3 and src.is_contiguous()
    n, H, W = (int(v) for v in src.shape[:3])
    dev = src.device
    with torch.cuda.device(dev):
        tmp = torch.empty((n, H, nw, 3), dtype=torch.uint8, device=dev)
        nbytes = table_bytes(H, W, nh, nw)
        tables = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        if dev not in _norm:
            _norm[dev] = torch.from_numpy(normalisation_table()).to(dev)
        norm = _norm[dev]
        rgb = torch.empty((n, nh, nw, 3), dtype=torch.uint8, device=dev) if want_rgb else None
        grey = torch.empty((n, 1, nh, nw), dtype=torch.float32, device=dev) if out_grey is None else out_grey
        assert grey.is_contiguous() and grey.dtype == torch.float32 and tuple(grey.shape) == (n, 1, nh, nw) and grey.device == dev
        N.check(N.lib().acez_ingest_frames(src.data_ptr(), n, H, W, int(nh), int(nw), tmp.data_ptr(), tables.data_ptr(), nbytes, norm.data_ptr(),
                                           rgb.data_ptr() if want_rgb else None, grey.data_ptr(),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        # tmp and tables go back to torch's caching allocator here; it hands a block out again only to work on this same stream
    return grey, rgb


def _chunks(positions, frame_bytes, chunk_frames):
    per = max(1, min(int(chunk_frames), CHUNK_BYTES // max(frame_bytes, 1)))
    return [positions[i:i + per] for i in range(0, len(positions), per)]


def load_frames_device(rgb_glob, image_resolution=480, files=None, return_rgb=False, size_classes=False, workers=12, device=None,
                       chunk_frames=CHUNK_FRAMES):
    """cli.load_frames with threaded decoding and the resize on the device: the same return value (see there), with the float32 frame
    tensors on `device` (default: the current one) and bit for bit the host path's; rgb is host uint8 numpy as there.

    Every size class passes check_frame_size, and a second size without size_classes is refused, from the image headers, before any
    frame is decoded. Frames are then grouped by SOURCE size and go through in chunks of at most chunk_frames frames and 256 MB: one
    pinned staging buffer, one upload and one acez_ingest_frames call per chunk, while the pool decodes the next chunk into a second
    staging buffer."""
    from PIL import Image
    from .session import check_frame_size
    if not torch.cuda.is_available():
        raise RuntimeError("load_frames_device needs a GPU: resize and grey conversion are HIP kernels (no CPU fallback; the host "
                           "path is cli.load_frames)")
    dev = torch.device("cuda") if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"load_frames_device runs on a GPU, not on {dev} (the host path is cli.load_frames)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if files is None:
        files = sorted(glob.glob(rgb_glob))
    if not files:
        raise SystemExit(f"no files match {rgb_glob!r}")
    factors, shapes, sources = [], {}, {}
    for i, f in enumerate(files):                                        # headers only
        try:
            with Image.open(f) as im:
                w, h = im.size
        except Exception as e:
            raise SystemExit(f"{f}: cannot decode image ({e})")
        sc, nh, nw = resized_size(w, h, image_resolution)
        if (nh, nw) not in shapes:
            if shapes and not size_classes:
                size = next(iter(shapes))
                raise SystemExit(f"{f}: resized frame is {(nh, nw)}, the first one {size}: frames of ONE size were expected (load_frames("
                                 "size_classes=True) takes a mix; the entry points do)")
            try:
                check_frame_size(nh, nw)
            except RuntimeError as e:
                raise SystemExit(str(e))
            shapes[(nh, nw)] = []
        shapes[(nh, nw)].append(i)
        sources.setdefault((h, w), []).append(i)
        factors.append(sc)
    slot = {}                                                            # file position -> (resized shape, index in its class)
    for shape, pos in shapes.items():
        for j, i in enumerate(pos):
            slot[i] = (shape, j)
    with torch.cuda.device(dev):
        frames = {shape: torch.empty((len(pos), 1) + shape, dtype=torch.float32, device=dev) for shape, pos in shapes.items()}
        work = [((h, w), part) for (h, w), pos in sources.items() for part in _chunks(pos, h * w * 3, chunk_frames)]
        staging = [None, None]                                           # two pinned buffers: one uploads while the pool fills the other
        uploaded = [None, None]                                          # the event after the last upload out of each
        rgbs = [None] * len(files)
        rgb_parts = []
        stream = torch.cuda.current_stream(dev)
        with concurrent.futures.ThreadPoolExecutor(max_workers=pool_size(workers)) as pool:

            def submit(k):
                (h, w), part = work[k]
                b = k % 2
                if uploaded[b] is not None:
                    uploaded[b].synchronize()                            # the buffer's last upload has left it
                need = len(part) * h * w * 3
                if staging[b] is None or staging[b].numel() < need:
                    staging[b] = torch.empty(need, dtype=torch.uint8, pin_memory=True)
                host = staging[b][:need].view(len(part), h, w, 3)
                view = host.numpy()
                return host, [pool.submit(_decode, files[i], view[j]) for j, i in enumerate(part)]

            pending = submit(0)
            for k, ((h, w), part) in enumerate(work):
                host, futures = pending
                try:
                    for fu in futures:
                        fu.result()
                except BaseException:
                    for fu in futures:
                        fu.cancel()
                    raise
                src = host.to(dev, non_blocking=True)
                uploaded[k % 2] = torch.cuda.Event()
                uploaded[k % 2].record(stream)
                if k + 1 < len(work):
                    pending = submit(k + 1)                              # decoded while this chunk uploads and runs
                shape, j0 = slot[part[0]]
                direct = all(slot[i] == (shape, j0 + j) for j, i in enumerate(part))   # the chunk is one run of its class
                grey, rgb = ingest_frames(src, shape[0], shape[1], want_rgb=return_rgb,
                                          out_grey=frames[shape][j0:j0 + len(part)] if direct else None)
                if not direct:
                    frames[shape].index_copy_(0, torch.tensor([slot[i][1] for i in part], device=dev), grey)
                if return_rgb:
                    rgb_parts.append((part, rgb))
        for part, rgb in rgb_parts:                                      # 1.2 MB per 640 x 480 frame back to the host
            host = rgb.cpu().numpy()
            for j, i in enumerate(part):
                rgbs[i] = host[j]
        torch.cuda.current_stream(dev).synchronize()
    if not size_classes:
        out = (files, next(iter(frames.values())), factors[-1])
        return out + (np.stack(rgbs),) if return_rgb else out
    classes = [(np.array(pos, np.int64), frames[shape]) for shape, pos in shapes.items()]
    out = (files, classes, np.array(factors, np.float64))
    return out + (rgbs,) if return_rgb else out


def load_session_frames_device(rgb_glob, image_resolution=480, files=None, return_rgb=False, workers=12, device=None):
    """cli.load_session_frames on the device path: a folder of one size comes back as load_frames_device returns it, a folder of mixed
    sizes as load_frames_device(size_classes=True) returns it."""
    out = load_frames_device(rgb_glob, image_resolution, files=files, return_rgb=return_rgb, size_classes=True, workers=workers, device=device)
    if len(out[1]) > 1:
        return out
    files, classes, factors = out[:3]
    one = (files, classes[0][1], float(factors[-1]))
    return one + (np.stack(out[3]),) if return_rgb else one
