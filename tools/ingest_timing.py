"""Image ingest: the host path (images.load_frames, one Python loop over Pillow) against the device path (acezero_amd.ingest: threaded
decode, HIP resize + grey + normalise) on N synthetic 1920 x 1080 JPEGs written to a temporary folder. Prints a table and one JSON
line, all in milliseconds per frame:
  host            images.load_frames over the N files, wall clock (decode + resize + grey + normalise on one thread)
  device[w]       ingest.load_frames_device with w decode threads over the same files, wall clock to the final synchronise
  decode[w]       ingest.decode_frames with w threads alone, wall clock
  upload          one pinned chunk of 32 decoded frames host -> device, HIP events
  kernels         acez_ingest_frames on that chunk once resident (tables + two launches), HIP events; with the bytes the two
                  passes move per frame this gives the achieved bytes/s
Every timed shape is warmed up first; wall-clock figures are the median of --reps runs, event figures of --event-reps. Before
anything is timed the device frames are compared with the host frames bit for bit.

    python tools/ingest_timing.py [--n 200] [--reps 3] [--event-reps 20]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, RES = 1080, 1920, 480
WORKERS = (1, 4, 16)
CHUNK = 32


def write_jpegs(folder, n):
    """n seeded synthetic frames: smooth structure plus mild noise (a JPEG of pure noise is neither typical in size nor in decode time)."""
    from PIL import Image
    rng = np.random.default_rng(2089)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([127 + 100 * np.sin(xx / 97 + c) * np.cos(yy / 61 - c) for c in range(3)], -1)
    base += rng.normal(0, 6, base.shape).astype(np.float32)
    for i in range(n):
        img = np.roll(base, (17 * i, 29 * i), (0, 1)) + (i % 16)
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(folder, f"frame_{i:05d}.jpg"), quality=90)
    return os.path.join(folder, "frame_*.jpg")


def wall_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


def event_ms(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200, help="number of synthetic 1920 x 1080 JPEGs")
    ap.add_argument("--reps", type=int, default=3, help="repeats of every wall-clock figure")
    ap.add_argument("--event-reps", type=int, default=20, help="repeats of every HIP-event figure")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_timing.py measures on a GPU; there is nothing to time without one")
    from acezero_amd import images, ingest
    out = {"n": a.n, "source": [H, W], "image_resolution": RES, "cpus": len(os.sched_getaffinity(0)), "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as folder:
        glob_ = write_jpegs(folder, a.n)
        files = sorted(os.path.join(folder, f) for f in os.listdir(folder))
        warm = files[:min(len(files), 2 * CHUNK)]
        # the same frames first (and the warm-up of both paths)
        _, hf, _, hrgb = images.load_frames(None, RES, files=warm, return_rgb=True)
        _, df, _, drgb = ingest.load_frames_device(None, RES, files=warm, return_rgb=True, workers=16)
        assert torch.equal(df.cpu(), hf) and np.array_equal(drgb, hrgb), "device frames differ from the host frames"
        nh, nw = hf.shape[2:]
        out["resized"] = [int(nh), int(nw)]
        out["host_ms"], raw = wall_ms(lambda: images.load_frames(glob_, RES), max(1, a.reps - 1))
        out["host_ms"] /= a.n
        out["host_ms_runs"] = [round(t / a.n, 3) for t in raw]
        out["device_ms"], out["decode_ms"], out["device_ms_runs"] = {}, {}, {}
        for w in WORKERS:
            ingest.load_frames_device(None, RES, files=warm, workers=w)
            med, raw = wall_ms(lambda: ingest.load_frames_device(glob_, RES, workers=w), a.reps)
            out["device_ms"][str(w)] = med / a.n
            out["device_ms_runs"][str(w)] = [round(t / a.n, 3) for t in raw]
            med, _ = wall_ms(lambda: ingest.decode_frames(files, w), max(1, a.reps - 1))
            out["decode_ms"][str(w)] = med / a.n
        out["pool_size"] = {str(w): ingest.pool_size(w) for w in WORKERS}
        # one chunk: upload and kernels apart
        k = min(CHUNK, len(files))
        host = torch.empty((k, H, W, 3), dtype=torch.uint8, pin_memory=True)
        view = host.numpy()
        for j, arr in enumerate(ingest.decode_frames(files[:k], 16)):
            np.copyto(view[j], arr)
        dev = torch.empty_like(host, device="cuda")
        for _ in range(3):
            dev.copy_(host, non_blocking=True)
            ingest.ingest_frames(dev, nh, nw)
        torch.cuda.synchronize()
        med, _ = event_ms(lambda: dev.copy_(host, non_blocking=True), a.event_reps)
        out["upload_ms"] = med / k
        out["upload_GBps"] = host.numel() / (med * 1e-3) / 1e9
        med, _ = event_ms(lambda: ingest.ingest_frames(dev, nh, nw), a.event_reps)
        out["kernels_ms"] = med / k
        # bytes the two passes move per frame: source read, uint8 intermediate written and read, RGB and float32 grey written
        traffic = H * W * 3 + 2 * H * nw * 3 + nh * nw * 3 + nh * nw * 4
        out["kernel_bytes_per_frame"] = traffic
        out["kernels_GBps"] = traffic * k / (med * 1e-3) / 1e9
        med, _ = event_ms(lambda: ingest.ingest_frames(dev, nh, nw, want_rgb=False), a.event_reps)
        out["kernels_no_rgb_ms"] = med / k
    print(f"{a.n} JPEGs {W} x {H} -> {nw} x {nh}, ms per frame ({out['device']}, {out['cpus']} CPUs)")
    print(f"  host load_frames              {out['host_ms']:8.3f}")
    for w in WORKERS:
        print(f"  device, {w:2d} workers (pool {out['pool_size'][str(w)]:2d})  {out['device_ms'][str(w)]:8.3f}   decode alone {out['decode_ms'][str(w)]:8.3f}   "
              f"speed-up {out['host_ms'] / out['device_ms'][str(w)]:5.2f} x")
    print(f"  upload (pinned, {k} frames)    {out['upload_ms']:8.3f}   {out['upload_GBps']:.1f} GB/s")
    print(f"  kernels                       {out['kernels_ms']:8.3f}   {out['kernels_GBps']:.0f} GB/s   without RGB output {out['kernels_no_rgb_ms']:.3f}")
    print(json.dumps({k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in out.items()}))


if __name__ == "__main__":
    main()
