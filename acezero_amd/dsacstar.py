"""Drop-in for the reference's `dsacstar` extension module (dsacstar/dsacstar.cpp:898-903).

    import acezero_amd.dsacstar as dsacstar
    inliers = dsacstar.forward_rgb(scene_coordinates_1x3xHxW, out_pose_4x4, hypotheses, threshold, focal, ppX, ppY,
                                   inlier_alpha, max_reproj, subsampling, seed, max_tries)

Same positional arguments, in-place `out_pose` (cam->world) and integer return as register_mapping.py:229-242 uses
them. The work runs on the GPU through libacez.so (acez_register_rgb_host / acez_register_rgb_device); there is no
CPU path. The reference's ThreadRand is seeded once per process and its streams continue across calls
(thread_rand.cpp:13-30); the equivalent here is a per-process call counter used as the frame id of the
counter-based stream, so that successive frames draw different samples but every (seed, call index) is
reproducible. `register_batch` is the batched, device-resident entry the MI355X pipeline should use instead.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N

_ctx = {}
_calls = 0
_verbose = False


def set_verbose(on=True):
    """The reference prints eight progress lines per frame (dsacstar.cpp:101-174); silent by default here, opt-in for parity of the
    console output (stage names as in the reference; the stages run inside one kernel, so there is one time for all of them)."""
    global _verbose
    _verbose = bool(on)
MAX_REF_STEPS = 100  # dsacstar.cpp:47


def _context(max_frames, h, w, device):
    """-> (handle, library that owns it). One cached context per device AND library build: inside N.diag_library() the module-wide
    library is the diagnostics build, and a handle must only ever be driven through the library that created it."""
    L = N.lib()
    key = (device, L._name)
    c = _ctx.get(key)
    if c is None or c["frames"] < max_frames or c["h"] < h or c["w"] < w:
        mf, mh, mw = max(max_frames, c["frames"] if c else 1), max(h, c["h"] if c else 0), max(w, c["w"] if c else 0)
        hnd = C.c_void_p()
        N.check(L.acez_ransac_create(C.byref(hnd), mf, mh, mw, device))   # raises before the old context is touched
        if c is not None:
            del _ctx[key]
            L.acez_ransac_destroy(c["h_"])                                  # waits for the launches still using it
        c = {"h_": hnd, "frames": mf, "h": mh, "w": mw, "lib": L}
        _ctx[key] = c
    return c["h_"], c["lib"]


def _params(hyps, thr, alpha, max_reproj, sub, max_tries):
    return N.RansacParams(int(hyps), int(max_tries), float(thr), float(alpha), float(max_reproj), int(sub), MAX_REF_STEPS, 0)


def _check_1x3(name, t):
    if t.dim() != 4 or t.shape[0] != 1 or t.shape[1] != 3 or t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be a float32 tensor of shape 1x3xHxW")


def _check_call(name, outPose):
    """The checks both single-frame entries make after their input shapes; -> the frame id of this call (the shared counter)."""
    global _calls
    if outPose.dim() != 2 or tuple(outPose.shape) != (4, 4) or outPose.dtype != torch.float32:
        raise RuntimeError("outPose must be a float32 tensor of shape 4x4")
    if not torch.cuda.is_available():
        raise RuntimeError(f"dsacstar.{name}: no GPU visible; the MI355X implementation has no CPU path")
    _calls += 1
    return _calls - 1


def _host_call(entry, inputs, outPose, *args):
    """The host-buffer entry `entry`(ctx, (data, strides) of each [1,3,H,W] input, H, W, *args, pose, inliers, no mask) of the
    current device's context; the cam->world pose goes to outPose. -> the inlier count."""
    H, W = int(inputs[0].shape[2]), int(inputs[0].shape[3])
    ctx, L = _context(1, H, W, torch.cuda.current_device())
    pose = np.zeros(16, np.float32)
    inliers = C.c_int32(0)
    strided = [a for t in inputs for a in (C.c_void_p(t.data_ptr()), *t.stride()[1:])]
    N.check(getattr(L, entry)(ctx, *strided, H, W, *args, pose.ctypes.data_as(C.c_void_p), C.byref(inliers), None))
    outPose.copy_(torch.from_numpy(pose.reshape(4, 4)))
    return int(inliers.value)


def _device_call(entry, inputs, args, frame_ids, want_masks):
    """The device entry `entry`(ctx, inputs, n, H, W, *args, frame ids, poses, inliers, masks, stream) on the current stream of the
    inputs' device: inputs are contiguous CUDA [n,3,H,W] tensors. -> (poses [n,4,4], inliers [n], masks [n,H,W] or None)."""
    n, _, H, W = inputs[0].shape
    dev = inputs[0].device
    ctx, L = _context(n, H, W, dev.index)
    ids = (C.c_uint64 * n)(*[int(x) for x in frame_ids]) if frame_ids is not None else None
    poses = torch.empty(n, 4, 4, dtype=torch.float32, device=dev)
    inl = torch.empty(n, dtype=torch.int32, device=dev)
    masks = torch.empty(n, H, W, dtype=torch.uint8, device=dev) if want_masks else None
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        N.check(getattr(L, entry)(ctx, *[C.c_void_p(t.data_ptr()) for t in inputs], n, H, W, *args, ids, C.c_void_p(poses.data_ptr()),
                                  C.c_void_p(inl.data_ptr()), C.c_void_p(masks.data_ptr()) if masks is not None else None, stream))
    return poses, inl, masks


def _debug_fetch(entry, n, hyps, device, samples):
    """The per-hypothesis results of the last call of one kind, from the cached context of `device` (default: the current one)."""
    dev = torch.cuda.current_device() if device is None else device
    L = N.lib()
    out = {"samples": np.zeros((n, hyps, 3), np.int32)} if samples else {}
    out.update(hyp_poses=np.zeros((n, hyps, 6)), scores=np.zeros((n, hyps)), best=np.zeros(n, np.int32), refined=np.zeros((n, 6)))
    N.check(getattr(L, entry)(_ctx[(dev, L._name)]["h_"], n, hyps, *[a.ctypes.data_as(C.c_void_p) for a in out.values()]))
    return out


def reset_call_counter(value=0):
    global _calls
    _calls = int(value)


def forward_rgb(sceneCoordinates, outPose, ransacHypotheses, inlierThreshold, focalLength, ppointX, ppointY, inlierAlpha,
                maxReproj, subSampling, randomSeed, max_hypotheses_tries):
    sc = sceneCoordinates
    _check_1x3("sceneCoordinates", sc)
    frame_id = _check_call("forward_rgb", outPose)
    prm = _params(ransacHypotheses, inlierThreshold, inlierAlpha, maxReproj, subSampling, max_hypotheses_tries)
    intr = N.Intrinsics(float(focalLength), float(ppointX), float(ppointY))
    import time
    t0 = time.perf_counter()
    if _verbose:
        print("Sampling " + str(int(ransacHypotheses)) + " hypotheses.", flush=True)
    if sc.is_cuda:
        poses, inl, _ = register_batch(sc[0][None], [intr], prm, randomSeed, [frame_id], want_masks=False)
        outPose.copy_(poses[0].to(outPose.device))
        count = int(inl[0].item())
    else:
        count = _host_call("acez_register_rgb_host", [sc], outPose, C.byref(prm), C.byref(intr), C.c_uint64(int(randomSeed)),
                           C.c_uint64(frame_id))
    if _verbose:
        print(f"Calculating scores. / Drawing final hypothesis. / Refining winning pose: done in {(time.perf_counter() - t0) * 1e3:.2f}ms. "
              f"Inliers: {count}", flush=True)
    return count


def register_batch(scene_coords, intrinsics, params, seed, frame_ids=None, want_masks=True):
    """scene_coords: CUDA float32 [n,3,H,W]; intrinsics: list of (focal, ppx, ppy) or N.Intrinsics.
    Returns (poses [n,4,4] f32, inliers [n] i32, masks [n,H,W] u8 or None), all CUDA tensors; asynchronous."""
    assert scene_coords.is_cuda and scene_coords.dtype == torch.float32 and scene_coords.dim() == 4 and scene_coords.shape[1] == 3
    sc = scene_coords.contiguous()
    if not isinstance(params, N.RansacParams):
        params = _params(**params)
    arr = (N.Intrinsics * sc.shape[0])()
    for i, it in enumerate(intrinsics):
        arr[i] = it if isinstance(it, N.Intrinsics) else N.Intrinsics(float(it[0]), float(it[1]), float(it[2]))
    return _device_call("acez_register_rgb_device", [sc], (C.byref(params), arr, C.c_uint64(int(seed))), frame_ids, want_masks)


def debug_fetch(n, hyps, device=None):
    return _debug_fetch("acez_ransac_debug_fetch", n, hyps, device, samples=False)


# ---------------------------------------------------------------------------------------------------- RGB-D (forward_rgbd)
MAX_HYPOTHESES_TRIES = 16  # dsacstar.cpp:48, the tries of the reference's RGB-D sampling
# the defaults of an RGB-D call's acez_ransac_params: thr and max_reproj are centimetres (3D distance), sub is unused
_RGBD_DEFAULTS = dict(max_tries=MAX_HYPOTHESES_TRIES, sub=8)


def camera_coordinates(depth, focal, ppx, ppy, stride=8):
    """Camera coordinates at the feature-map cell centres (stride x + stride / 2) from depth [n,h,w] (metres, 0 = none): float32
    [n,3,h,w] on depth's device. focal / ppx / ppy: one value, or one per frame. The mapping buffer's formula
    (ReconstructionSession._fill_buffer, dataset.py:347-388): eye = ((px - ppx) / f * d, (py - ppy) / f * d, d) in float32, so that
    mapping and registration agree on every cell."""
    d = torch.as_tensor(depth, dtype=torch.float32)
    if d.dim() == 2:
        d = d[None]
    n, h, w = d.shape
    dev = d.device

    def per_frame(v):
        return torch.as_tensor(np.broadcast_to(np.asarray(v, np.float32), (n,)).copy()).to(dev).view(n, 1, 1)
    f, cx, cy = per_frame(focal), per_frame(ppx), per_frame(ppy)
    px = (torch.arange(w, device=dev, dtype=torch.float32) * stride + stride // 2).view(1, 1, w)
    py = (torch.arange(h, device=dev, dtype=torch.float32) * stride + stride // 2).view(1, h, 1)
    return torch.stack([(px - cx) / f * d, (py - cy) / f * d, d], dim=1).contiguous()


def forward_rgbd(sceneCoordinates, cameraCoordinates, outPose, ransacHypotheses, inlierThreshold, inlierAlpha, maxDistError):
    """The reference's commented-out binding (dsacstar.cpp:493-640,901): 1x3xHxW scene and camera coordinates (metres), in-place
    cam->world `outPose`, inlierThreshold / maxDistError in centimetres; returns the inlier count. As in forward_rgb, the per-process
    call counter keys the random stream (the reference's ThreadRand::init() continues one stream across calls)."""
    sc, cc = sceneCoordinates, cameraCoordinates
    _check_1x3("sceneCoordinates", sc)
    _check_1x3("cameraCoordinates", cc)
    if tuple(sc.shape) != tuple(cc.shape):
        raise RuntimeError("sceneCoordinates and cameraCoordinates must have the same shape")
    frame_id = _check_call("forward_rgbd", outPose)
    prm = _params(ransacHypotheses, inlierThreshold, inlierAlpha, maxDistError, **_RGBD_DEFAULTS)
    if sc.is_cuda or cc.is_cuda:
        dev = sc.device if sc.is_cuda else cc.device
        poses, inl, _ = register_batch_rgbd(sc[0][None].to(dev), cc[0][None].to(dev), prm, 0, [frame_id], want_masks=False)
        outPose.copy_(poses[0].to(outPose.device))
        return int(inl[0].item())
    return _host_call("acez_register_rgbd_host", [sc, cc], outPose, C.byref(prm), C.c_uint64(0), C.c_uint64(frame_id))


def register_batch_rgbd(scene_coords, camera_coords, params, seed, frame_ids=None, want_masks=True):
    """scene_coords, camera_coords: CUDA float32 [n,3,H,W] (metres); params: N.RansacParams or dict(hyps, thr, alpha, max_reproj
    [, max_tries]) with thr / max_reproj in centimetres. Returns (poses [n,4,4] f32 cam->world, inliers [n] i32, masks [n,H,W] u8 or
    None), all CUDA tensors; asynchronous."""
    for t in (scene_coords, camera_coords):
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] == 3
    assert tuple(scene_coords.shape) == tuple(camera_coords.shape) and scene_coords.device == camera_coords.device
    if not isinstance(params, N.RansacParams):
        params = _params(**{**_RGBD_DEFAULTS, **params})
    return _device_call("acez_register_rgbd_device", [scene_coords.contiguous(), camera_coords.contiguous()],
                        (C.byref(params), C.c_uint64(int(seed))), frame_ids, want_masks)


def debug_fetch_rgbd(n, hyps, device=None):
    """Per-hypothesis results of the last RGB-D call: sampled triples (map indices y*W+x), (rvec, tvec), scores, best, refined."""
    return _debug_fetch("acez_ransac_rgbd_debug_fetch", n, hyps, device, samples=True)
