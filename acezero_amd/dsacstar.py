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


def _as_params(params, defaults=None):
    """params as N.RansacParams: itself, or built from a dict of _params' arguments over `defaults`."""
    return params if isinstance(params, N.RansacParams) else _params(**{**(defaults or {}), **params})


def _intrinsics_array(intrinsics, n):
    """n acez_intrinsics from a list of (focal, ppx, ppy) or N.Intrinsics."""
    arr = (N.Intrinsics * n)()
    for i, it in enumerate(intrinsics):
        arr[i] = it if isinstance(it, N.Intrinsics) else N.Intrinsics(float(it[0]), float(it[1]), float(it[2]))
    return arr


def _check_1x3(**tensors):
    """The tensor arguments of a single-frame entry, by name: each a float32 1x3xHxW, all of one shape."""
    names = list(tensors)
    for name, t in tensors.items():
        if t.dim() != 4 or t.shape[0] != 1 or t.shape[1] != 3 or t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be a float32 tensor of shape 1x3xHxW")
    if any(tuple(t.shape) != tuple(tensors[names[0]].shape) for t in tensors.values()):
        raise RuntimeError(f"{', '.join(names[:-1])} and {names[-1]} must have the same shape")


def _take_frame_ids(n):
    """-> the next n values of the call counter all entries share."""
    global _calls
    _calls += n
    return list(range(_calls - n, _calls))


def _next_frame_id(name):
    """-> the frame id of this call (the shared counter), after checking that a GPU is visible."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"dsacstar.{name}: no GPU visible; the MI355X implementation has no CPU path")
    return _take_frame_ids(1)[0]


def _check_batch(*tensors):
    """The inputs of a batched entry: CUDA float32 [n,3,H,W] tensors of one shape on one device."""
    for t in tensors:
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] == 3
        assert tuple(t.shape) == tuple(tensors[0].shape) and t.device == tensors[0].device


def _check_call(name, outPose):
    """The checks both forward entries make after their input shapes; -> the frame id of this call (the shared counter)."""
    if outPose.dim() != 2 or tuple(outPose.shape) != (4, 4) or outPose.dtype != torch.float32:
        raise RuntimeError("outPose must be a float32 tensor of shape 4x4")
    return _next_frame_id(name)


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
    _check_1x3(sceneCoordinates=sc)
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
    _check_batch(scene_coords)
    sc = scene_coords.contiguous()
    args = (C.byref(_as_params(params)), _intrinsics_array(intrinsics, sc.shape[0]), C.c_uint64(int(seed)))
    return _device_call("acez_register_rgb_device", [sc], args, frame_ids, want_masks)


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


def camera_coordinates_device(depth, focal, ppx, ppy, stride=8):
    """camera_coordinates as ONE launch (acez_camera_coordinates): depth CUDA float32 [n,h,w], focal one value or one per frame, ppx /
    ppy the frames' shared principal point. float32 [n,3,h,w] on depth's device, asynchronous on its current stream; bit for bit
    camera_coordinates' values where there is depth, +0 in all three channels where there is none (depth == 0)."""
    assert depth.is_cuda and depth.dtype == torch.float32 and depth.dim() == 3
    d = depth.contiguous()
    n, h, w = d.shape
    dev = d.device
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    f = torch.from_numpy(np.broadcast_to(np.asarray(focal, np.float32), (n,)).copy()).to(dev)
    with torch.cuda.device(dev):
        N.check(N.lib().acez_camera_coordinates(C.c_void_p(d.data_ptr()), C.c_void_p(f.data_ptr()), float(ppx), float(ppy), n, h, w, int(stride),
                                                C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def forward_rgbd(sceneCoordinates, cameraCoordinates, outPose, ransacHypotheses, inlierThreshold, inlierAlpha, maxDistError):
    """The reference's commented-out binding (dsacstar.cpp:493-640,901): 1x3xHxW scene and camera coordinates (metres), in-place
    cam->world `outPose`, inlierThreshold / maxDistError in centimetres; returns the inlier count. As in forward_rgb, the per-process
    call counter keys the random stream (the reference's ThreadRand::init() continues one stream across calls)."""
    sc, cc = sceneCoordinates, cameraCoordinates
    _check_1x3(sceneCoordinates=sc, cameraCoordinates=cc)
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
    _check_batch(scene_coords, camera_coords)
    return _device_call("acez_register_rgbd_device", [scene_coords.contiguous(), camera_coords.contiguous()],
                        (C.byref(_as_params(params, _RGBD_DEFAULTS)), C.c_uint64(int(seed))), frame_ids, want_masks)


def debug_fetch_rgbd(n, hyps, device=None):
    """Per-hypothesis results of the last RGB-D call: sampled triples (map indices y*W+x), (rvec, tvec), scores, best, refined."""
    return _debug_fetch("acez_ransac_rgbd_debug_fetch", n, hyps, device, samples=True)


# ---------------------------------------------------------------------------------------------------- backward passes
PROB_THRESH = 0.001  # dsacstar_derivative.h:36: hypotheses below it are neither refined nor differentiated


def _backward_device_call(entry, inputs, gt_poses, mid_args, seed, frame_ids, weights, out_grad):
    """The device entry `entry`(ctx, inputs, gt, n, H, W, *mid_args, *weights, seed, frame ids, grad, loss, stream) on the current
    stream of the inputs' device; mid_args: the params and, for RGB, the intrinsics. -> (gradient or out_grad with it added, loss)."""
    n, _, H, W = inputs[0].shape
    dev = inputs[0].device
    gt = torch.as_tensor(gt_poses, dtype=torch.float32).reshape(n, 4, 4).to(dev).contiguous()
    if out_grad is None:
        out_grad = torch.zeros(n, 3, H, W, dtype=torch.float32, device=dev)
    assert out_grad.is_cuda and out_grad.dtype == torch.float32 and out_grad.is_contiguous() and tuple(out_grad.shape) == (n, 3, H, W)
    loss = torch.empty(n, dtype=torch.float64, device=dev)
    inputs = [t.contiguous() for t in inputs]
    ctx, L = _context(n, H, W, dev.index)
    ids = (C.c_uint64 * n)(*[int(x) for x in frame_ids]) if frame_ids is not None else None
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        N.check(getattr(L, entry)(ctx, *[C.c_void_p(t.data_ptr()) for t in inputs], C.c_void_p(gt.data_ptr()), n, H, W, *mid_args,
                                  *[float(x) for x in weights], C.c_uint64(int(seed)), ids, C.c_void_p(out_grad.data_ptr()),
                                  C.c_void_p(loss.data_ptr()), stream))
    return out_grad, loss


def _backward_host_call(entry, inputs, og, gt, mid_args, seed, frame_id, weights):
    """The host-buffer entry `entry`(ctx, (data, strides) of each [1,3,H,W] input, gt, H, W, *mid_args, *weights, seed, frame id,
    (data, strides) of og, loss) of the current device's context: the gradient is added to og. -> the expected loss."""
    H, W = int(og.shape[2]), int(og.shape[3])
    ctx, L = _context(1, H, W, torch.cuda.current_device())
    gt16 = np.ascontiguousarray(gt.cpu().numpy(), np.float32)
    out = C.c_double(0.0)
    strided = [a for t in inputs for a in (C.c_void_p(t.data_ptr()), *t.stride()[1:])]
    N.check(getattr(L, entry)(ctx, *strided, gt16.ctypes.data_as(C.c_void_p), H, W, *mid_args, *[float(x) for x in weights],
                              C.c_uint64(int(seed)), C.c_uint64(frame_id), C.c_void_p(og.data_ptr()), *og.stride()[1:], C.byref(out)))
    return float(out.value)


def _backward_single(kind, inputs, og, gtPose, mid_args, seed, weights):
    """backward_rgb / backward_rgbd after their input checks: on the device of the first CUDA tensor among the inputs and og, or
    through the host-buffer entry if all are host tensors. The gradient is added to og. -> the expected loss."""
    gt = torch.as_tensor(gtPose, dtype=torch.float32)
    if tuple(gt.shape) != (4, 4):
        raise RuntimeError("gtPose must be a 4x4 tensor")
    frame_id = _next_frame_id(f"backward_{kind}")
    dev = next((t.device for t in (*inputs, og) if t.is_cuda), None)
    if dev is None:
        return _backward_host_call(f"acez_register_{kind}_backward_host", inputs, og, gt, mid_args, seed, frame_id, weights)
    grad, loss = _backward_device_call(f"acez_register_{kind}_backward_device", [t.to(dev) for t in inputs], gt, mid_args, seed,
                                       [frame_id], weights, None)
    og.add_(grad.to(og.device))
    return float(loss[0].item())


def register_batch_rgbd_backward(scene_coords, camera_coords, gt_poses, params, seed, frame_ids=None, w_loss_rot=1.0,
                                 w_loss_trans=1.0, soft_clamp=100.0, out_grad=None):
    """The DSAC* RGB-D backward pass of n frames: scene_coords, camera_coords CUDA float32 [n,3,H,W] (metres), gt_poses [n,4,4]
    cam->world; params as register_batch_rgbd's. The hypotheses are those register_batch_rgbd draws for the same (seed, frame ids).
    Returns (grad [n,3,H,W] f32, expected loss [n] f64), CUDA tensors; the gradient is added to out_grad if one is given (a
    contiguous CUDA float32 [n,3,H,W]) and that tensor is returned. Asynchronous."""
    _check_batch(scene_coords, camera_coords)
    return _backward_device_call("acez_register_rgbd_backward_device", [scene_coords, camera_coords], gt_poses,
                                 (C.byref(_as_params(params, _RGBD_DEFAULTS)),), seed, frame_ids, (w_loss_rot, w_loss_trans, soft_clamp),
                                 out_grad)


def backward_rgbd(sceneCoordinates, cameraCoordinates, outSceneCoordinatesGrad, gtPose, ransacHypotheses, inlierThreshold, wLossRot,
                  wLossTrans, softClamp, inlierAlpha, maxDistError, randomSeed):
    """The reference's commented-out binding (dsacstar.cpp:642-895): 1x3xHxW scene and camera coordinates (metres), 4x4 cam->world
    gtPose; the gradient of the expected pose loss is ADDED to outSceneCoordinatesGrad (1x3xHxW float32) and the expected loss is
    returned. inlierThreshold / maxDistError in centimetres. The frame id is the call counter forward_rgbd uses, the seed randomSeed."""
    sc, cc, og = sceneCoordinates, cameraCoordinates, outSceneCoordinatesGrad
    _check_1x3(sceneCoordinates=sc, cameraCoordinates=cc, outSceneCoordinatesGrad=og)
    prm = _params(ransacHypotheses, inlierThreshold, inlierAlpha, maxDistError, **_RGBD_DEFAULTS)
    return _backward_single("rgbd", [sc, cc], og, gtPose, (C.byref(prm),), randomSeed, (wLossRot, wLossTrans, softClamp))


def register_batch_backward(scene_coords, intrinsics, gt_poses, params, seed, frame_ids=None, w_loss_rot=1.0, w_loss_trans=1.0,
                            soft_clamp=100.0, out_grad=None):
    """The DSAC* RGB backward pass of n frames: scene_coords CUDA float32 [n,3,H,W], intrinsics and params as register_batch's, gt_poses
    [n,4,4] cam->world. The hypotheses are those register_batch draws for the same (seed, frame ids). Returns (grad [n,3,H,W] f32,
    expected loss [n] f64), CUDA tensors; the gradient is added to out_grad if one is given. Asynchronous."""
    _check_batch(scene_coords)
    mid_args = (C.byref(_as_params(params)), _intrinsics_array(intrinsics, scene_coords.shape[0]))
    return _backward_device_call("acez_register_rgb_backward_device", [scene_coords], gt_poses, mid_args, seed, frame_ids,
                                 (w_loss_rot, w_loss_trans, soft_clamp), out_grad)


def backward_rgb(sceneCoordinates, outSceneCoordinatesGrad, gtPose, ransacHypotheses, inlierThreshold, focalLength, ppointX, ppointY,
                 wLossRot, wLossTrans, softClamp, inlierAlpha, maxReproj, subSampling, randomSeed):
    """The reference's commented-out binding (dsacstar.cpp:208-490): 1x3xHxW scene coordinates, 4x4 cam->world gtPose; the gradient
    of the expected pose loss is ADDED to outSceneCoordinatesGrad (1x3xHxW float32) and the expected loss is returned. The frame id
    is the call counter forward_rgb uses, the seed randomSeed; the tries are forward_rgb's default (16)."""
    sc, og = sceneCoordinates, outSceneCoordinatesGrad
    _check_1x3(sceneCoordinates=sc, outSceneCoordinatesGrad=og)
    prm = _params(ransacHypotheses, inlierThreshold, inlierAlpha, maxReproj, subSampling, MAX_HYPOTHESES_TRIES)
    intr = _intrinsics_array([(focalLength, ppointX, ppointY)], 1)   # one frame's: the device entry's array, the host entry's pointer
    return _backward_single("rgb", [sc], og, gtPose, (C.byref(prm), intr), randomSeed, (wLossRot, wLossTrans, softClamp))


def _mask_words_rgb(cells):
    return ((cells + 255) // 256) * 4   # one word per wavefront and row of 256 threads (mask_words of the RGB backward workspace)


def _mask_words_rgbd(cells):
    return ((cells + 511) // 512) * 8   # one word per wavefront and row of 512 threads (mask_words of the RGB-D one)


def _debug_fetch_backward(entry, n, hyps, h, w, n_samples, words, device):
    dev = torch.cuda.current_device() if device is None else device
    L = N.lib()
    out = dict(samples=np.zeros((n, hyps, n_samples), np.int32), hyp_poses=np.zeros((n, hyps, 6)), scores=np.zeros((n, hyps)),
               probs=np.zeros((n, hyps)), losses=np.zeros((n, hyps)), ref_poses=np.zeros((n, hyps, 6)),
               masks=np.zeros((n, hyps, words), np.uint64), entropy=np.zeros(n))
    N.check(getattr(L, entry)(_ctx[(dev, L._name)]["h_"], n, hyps, h, w, *[a.ctypes.data_as(C.c_void_p) for a in out.values()]))
    out["masks"] = np.unpackbits(out["masks"].view(np.uint8), axis=-1, bitorder="little").astype(bool)
    return out


def debug_fetch_rgbd_backward(n, hyps, h, w, device=None):
    """Per-hypothesis results of the last RGB-D backward call: samples, hyp_poses, scores, probs, losses, ref_poses, masks (bool
    [n,hyps,valid cells] over the valid cells in scan order), entropy."""
    return _debug_fetch_backward("acez_ransac_rgbd_backward_debug_fetch", n, hyps, h, w, 3, _mask_words_rgbd(h * w), device)


def debug_fetch_rgb_backward(n, hyps, h, w, device=None):
    """Per-hypothesis results of the last RGB backward call: samples (4 scan indices x*h+y), hyp_poses, scores, probs, losses,
    ref_poses, masks (bool [n,hyps,h*w] over all cells in scan order), entropy."""
    out = _debug_fetch_backward("acez_ransac_rgb_backward_debug_fetch", n, hyps, h, w, 4, _mask_words_rgb(h * w), device)
    out["masks"] = out["masks"][:, :, :h * w]
    return out


class _ExpectedPoseLoss(torch.autograd.Function):
    """batch_fn: register_batch_backward or register_batch_rgbd_backward; second: what it takes after the coordinates."""
    @staticmethod
    def forward(ctx, batch_fn, coords, second, gt_poses, params, seed, frame_ids, w_rot, w_trans, clamp):
        g, loss = batch_fn(coords.detach(), second, gt_poses, params, seed, frame_ids, w_rot, w_trans, clamp)
        ctx.save_for_backward(g)
        return loss.to(coords.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        return (None, g * grad_out.to(g.dtype).view(-1, 1, 1, 1)) + (None,) * 8


def expected_pose_loss_rgbd(coords, camera_coords, gt_poses, hypotheses=64, threshold=10.0, w_loss_rot=1.0, w_loss_trans=1.0,
                            soft_clamp=100.0, inlier_alpha=100.0, max_dist=100.0, seed=0, frame_ids=None):
    """Differentiable DSAC* RGB-D loss: the expected pose loss per frame, float32 [n] on the coordinates' device, whose .backward()
    puts the backward pass's gradient into coords.grad. coords, camera_coords: CUDA [n,3,H,W] (metres); gt_poses [n,4,4] cam->world.
    frame_ids default to the next values of the call counter forward_rgbd uses, so successive calls draw fresh hypotheses."""
    frame_ids = _take_frame_ids(coords.shape[0]) if frame_ids is None else list(frame_ids)
    prm = _params(hypotheses, threshold, inlier_alpha, max_dist, **_RGBD_DEFAULTS)
    return _ExpectedPoseLoss.apply(register_batch_rgbd_backward, coords, camera_coords, gt_poses, prm, seed, frame_ids, w_loss_rot,
                                   w_loss_trans, soft_clamp)


def expected_pose_loss_rgb(coords, intrinsics, gt_poses, hypotheses=64, threshold=10.0, w_loss_rot=1.0, w_loss_trans=1.0,
                           soft_clamp=100.0, inlier_alpha=100.0, max_reproj=100.0, subsampling=8, seed=0, frame_ids=None,
                           max_tries=MAX_HYPOTHESES_TRIES):
    """Differentiable DSAC* RGB loss: the expected pose loss per frame, float32 [n], whose .backward() puts the backward pass's
    gradient into coords.grad. coords: CUDA [n,3,H,W]; intrinsics: one (focal, ppx, ppy) per frame; gt_poses [n,4,4] cam->world.
    frame_ids default to the next values of the call counter forward_rgb uses."""
    frame_ids = _take_frame_ids(coords.shape[0]) if frame_ids is None else list(frame_ids)
    prm = _params(hypotheses, threshold, inlier_alpha, max_reproj, subsampling, max_tries)
    return _ExpectedPoseLoss.apply(register_batch_backward, coords, list(intrinsics), gt_poses, prm, seed, frame_ids, w_loss_rot,
                                   w_loss_trans, soft_clamp)
