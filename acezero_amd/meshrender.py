"""A triangle mesh rendered into the frames' cameras: one model depth map per image, with face ids, normals and colours on request
(include/acez.h section R; render_mesh.py and fuse_depth.py --model_depth_dir are the command lines).

    planes = render_mesh(vertices, faces, cam_to_world=poses, focals=f, sizes=[(h, w)] * n, max_depth=4.0, outputs=("depth_u16", "normal"))
    planes["depth_u16"][k]                                           # uint16 [h,w] of frame k: what write_depth_png writes
    both, model_only, measured_only, sum_abs, within = depth_agreement(planes["depth_u16"][k], sensor_u16, tolerance_units=10)

The mesh lives in HBM; the rasterisation and the resolve are HIP kernels (acezero_amd/csrc/meshrender_api.hip). There is no CPU
fallback. depth_agreement is integer arithmetic on torch tensors: exact and order-free on either device."""
import logging

import numpy as np
import torch

from . import _native as N
from .frames import _fill_rows, _per_frame, _w2c34, device_rows
from ._device import ptr as _ptr, stream as _stream
from .mesh import check_mesh

__all__ = ["render_mesh", "depth_agreement", "PLANES"]

WHY = "mesh rendering is a HIP kernel"
# plane -> (dtype, trailing shape)
PLANES = {"depth": (torch.float32, ()), "face": (torch.int32, ()), "depth_u16": (torch.uint16, ()), "normal": (torch.uint8, (3,)),
          "colour": (torch.uint8, (3,))}
_logger = logging.getLogger("acezero_amd")


def render_mesh(vertices, faces, cam_to_world=None, world_to_cam=None, focals=None, ppx=None, ppy=None, sizes=None, colours=None,
                min_depth=0.05, max_depth=10.0, depth_unit=0.001, outputs=("depth_u16",), frames_per_call=N.TSDF_MAX_FRAMES, info=None):
    """Rasterise the mesh (device tensors: vertices float32 [m,3], world, OpenCV convention; faces int32 [k,3]; colours uint8 [m,3] for
    the "colour" plane) into n cameras. sizes: (h, w), one pair or one per frame; focals, ppx, ppy: pixels of that frame, one number or
    one per frame; the principal point defaults to (w / 2, h / 2) and the pixel index is the image coordinate, as in TSDFVolume.integrate.
    Returns {plane: [one device tensor per frame]} for the planes named in outputs: "depth" float32 [h,w] (0: nothing hit), "face"
    int32 (-1), "depth_u16" uint16 (rint(depth / depth_unit), 0 beyond 65535), "normal" uint8 [h,w,3] (128 + rint(127 n), the face's
    camera-space normal towards the camera; 0 0 0: nothing hit) and "colour" uint8 [h,w,3]. Sequences are cut into calls of at most
    frames_per_call (256) frames; the result does not depend on the cut. A face index outside the vertices is refused
    (ACEZ_ERR_INVALID). info, a dict, receives guard_dropped: the triangle-frames dropped because a vertex projected 2^21 px or more
    off the principal point (a warning is logged if there are any: the maps may have a hole there)."""
    outputs = tuple(outputs)
    for name in outputs:
        if name not in PLANES:
            raise ValueError(f"unknown plane {name!r}: choose from {sorted(PLANES)}")
    if "colour" in outputs and colours is None:
        raise ValueError("the colour plane needs vertex colours")
    vertices, colours, faces = check_mesh(vertices, colours if "colour" in outputs else None, faces, "render_mesh", WHY)
    if focals is None or sizes is None:
        raise ValueError("focals and sizes are required")
    if not 1 <= int(frames_per_call) <= N.TSDF_MAX_FRAMES:
        raise ValueError(f"frames_per_call must be in 1 .. {N.TSDF_MAX_FRAMES}")
    src = world_to_cam if cam_to_world is None else cam_to_world
    n = 0 if src is None else len(src)
    w2c = _w2c34(world_to_cam, cam_to_world, n)
    sizes = np.asarray(sizes, np.int64)
    sizes = [tuple(int(s) for s in row) for row in np.broadcast_to(sizes.reshape(-1, 2), (n, 2))]
    focals = _per_frame(focals, n)
    ppx, ppy = (None if p is None else _per_frame(p, n) for p in (ppx, ppy))
    dev, m, k = vertices.device, vertices.shape[0], faces.shape[0]
    if k and bool(((faces < 0) | (faces >= m)).any()):                # the faces live on the device: acez_meshrender_check_faces' test there
        raise N.AcezError("ACEZ_ERR_INVALID: invalid argument: face index outside the vertices")
    planes = {name: [] for name in outputs}
    statuses = []
    for lo in range(0, n, int(frames_per_call)):
        part = slice(lo, min(n, lo + int(frames_per_call)))
        offsets, at = [], 0
        for h, w in sizes[part]:
            offsets.append(at)
            at += h * w
        rows = _fill_rows(sizes[part], offsets, w2c[part], focals[part], None if ppx is None else ppx[part], None if ppy is None else ppy[part])
        count = len(offsets)
        d_rows = device_rows(count, dev)
        keys = torch.empty(at, dtype=torch.int64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        need = set(outputs) | {"depth"}
        flat = {name: torch.empty((at, *PLANES[name][1]), dtype=PLANES[name][0], device=dev) for name in need}
        with torch.cuda.device(dev):
            N.check(N.lib().acez_meshrender(_ptr(vertices), _ptr(colours), m, _ptr(faces), k, rows, count, _ptr(d_rows), float(min_depth),
                                            float(max_depth), float(depth_unit), _ptr(keys), at, _ptr(flat["depth"]), _ptr(flat.get("face")),
                                            _ptr(flat.get("depth_u16")), _ptr(flat.get("normal")), _ptr(flat.get("colour")), at, _ptr(status),
                                            _stream()))
        statuses.append(status)
        for name in outputs:
            for (h, w), o in zip(sizes[part], offsets):
                planes[name].append(flat[name][o:o + h * w].reshape(h, w, *PLANES[name][1]))
    dropped = int(torch.cat(statuses).sum().item()) if statuses else 0
    if info is not None:
        info["guard_dropped"] = dropped
    if dropped:
        _logger.warning(f"render_mesh: {dropped} triangle-frames were dropped because a vertex projects 2^21 px or more off the principal "
                        f"point; the maps may have holes there")
    return planes


def _units(t):
    """A uint16 (or int16-carried) map as int32 0 .. 65535."""
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(t, np.uint16)))
    if t.dtype == torch.uint16:
        t = t.view(torch.int16)
    if t.dtype != torch.int16:
        raise TypeError(f"expected a uint16 depth map, got {t.dtype}")
    return t.to(torch.int32) & 0xFFFF


def depth_agreement(model_u16, measured_u16, tolerance_units):
    """Two uint16 depth maps of one frame, 0 = no value, compared in their units: (both_valid, model_only, measured_only, sum of
    |delta| over the pixels valid in both, the number of those with |delta| <= tolerance_units), Python ints. Integer arithmetic on
    whichever device the maps are on (the measured map moves to the model's)."""
    a = _units(model_u16)
    b = _units(measured_u16).to(a.device)
    if a.shape != b.shape:
        raise ValueError(f"the maps differ in size: {tuple(a.shape)} and {tuple(b.shape)}")
    both = (a > 0) & (b > 0)
    delta = torch.where(both, (a - b).abs(), torch.zeros_like(a)).long()
    out = torch.stack([both.sum(), ((a > 0) & (b == 0)).sum(), ((a == 0) & (b > 0)).sum(), delta.sum(),
                       (both & (delta <= int(tolerance_units))).sum()])
    return tuple(int(x) for x in out.cpu().tolist())


def agreement_line(counts, depth_unit):
    """(both-valid share of the pixels valid in either map, mean |delta| in millimetres over the pixels valid in both, share of those
    within the tolerance) from depth_agreement's counts (or their sums over frames); nan where a share has no pixels."""
    both, model_only, measured_only, sum_abs, within = counts
    either = both + model_only + measured_only
    nan = float("nan")
    return (both / either if either else nan, 1000.0 * depth_unit * sum_abs / both if both else nan, within / both if both else nan)


def render_to_folder(vertices, faces, colours, cam_to_world, focals, sizes, stems, depth_dir, min_depth, max_depth, depth_unit,
                     normals_dir=None, colour_dir=None, compare=None, tolerance=0.01, report=None, frames_per_write=64):
    """The pipeline of render_mesh.py and of fuse_depth.py --model_depth_dir: the mesh (device tensors) rendered into the n cameras at
    `sizes`, frame k written as depth_dir/stems[k].png (16-bit, formats.write_depth_png) and, where a folder is given, its normal and
    colour images as 8-bit RGB PNGs. compare: a list of measured uint16 [h,w] maps of the same sizes and unit; the agreement is then
    returned as log lines (one per frame, one for the folder) and, in `report` (a dict), as numbers. tolerance: metres. Frames are
    rendered and written frames_per_write at a time, so that a long sequence holds only that many maps."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from .formats import write_depth_png
    n = len(stems)
    outputs = ("depth_u16",) + (("normal",) if normals_dir is not None else ()) + (("colour",) if colour_dir is not None else ())
    folders = {"depth_u16": depth_dir, "normal": normals_dir, "colour": colour_dir}
    for name in outputs:
        os.makedirs(folders[name], exist_ok=True)
    units = max(0, int(round(tolerance / depth_unit)))
    lines, per_frame, total, dropped = [], [], [0] * 5, 0
    cam_to_world = np.asarray(cam_to_world, np.float64).reshape(n, 4, 4)
    with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as pool:
        for lo in range(0, n, frames_per_write):
            part = slice(lo, min(n, lo + frames_per_write))
            info = {}
            planes = render_mesh(vertices, faces, cam_to_world=cam_to_world[part], focals=np.asarray(focals)[part], sizes=sizes[part],
                                 colours=colours if colour_dir is not None else None, min_depth=min_depth, max_depth=max_depth,
                                 depth_unit=depth_unit, outputs=outputs, info=info)
            dropped += info["guard_dropped"]
            if compare is not None:
                for k, model in zip(range(lo, lo + len(planes["depth_u16"])), planes["depth_u16"]):
                    counts = depth_agreement(model, compare[k], units)
                    share, mean_mm, within = agreement_line(counts, depth_unit)
                    per_frame.append(dict(frame=stems[k], both_valid=counts[0], model_only=counts[1], measured_only=counts[2],
                                          sum_abs_units=counts[3], within_tolerance=counts[4], both_valid_share=share, mean_abs_mm=mean_mm,
                                          within_share=within))
                    lines.append(f"{stems[k]}: valid in both maps {100.0 * share:.2f} % of the pixels valid in either, mean |model - measured| "
                                 f"{mean_mm:.3f} mm, within {1000.0 * units * depth_unit:.1f} mm {100.0 * within:.2f} %")
                    total = [a + b for a, b in zip(total, counts)]
            host = {name: [t.cpu().numpy() for t in planes[name]] for name in outputs}
            names = [s + ".png" for s in stems[part]]
            list(pool.map(write_depth_png, [os.path.join(depth_dir, s) for s in names], host["depth_u16"]))
            for name in outputs[1:]:
                list(pool.map(lambda job: Image.fromarray(job[1]).save(job[0]), zip([os.path.join(folders[name], s) for s in names], host[name])))
    if compare is not None:
        share, mean_mm, within = agreement_line(total, depth_unit)
        lines.append(f"All {n} frames: valid in both maps {100.0 * share:.2f} % of the pixels valid in either, mean |model - measured| "
                     f"{mean_mm:.3f} mm, within {1000.0 * units * depth_unit:.1f} mm {100.0 * within:.2f} %")
        if report is not None:
            report.update(frames=per_frame, tolerance_units=units, depth_unit=depth_unit,
                          total=dict(both_valid=total[0], model_only=total[1], measured_only=total[2], sum_abs_units=total[3],
                                     within_tolerance=total[4], both_valid_share=share, mean_abs_mm=mean_mm, within_share=within))
    if report is not None:
        report["guard_dropped"] = dropped
    return lines
