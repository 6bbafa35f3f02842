"""Host-side image and depth loading for the command lines, the library and the tools: what the reference's CamLocDataset does
between a file and the encoder's input (decode, resize, grey, normalise), the focal lengths that go with the frames, and the depth
maps at the feature-map cells. acezero_amd.ingest is the device twin of the frame loaders. session_frames gives the entry points
one record of a session's frames and focals, whether the folder holds one frame size or several."""
import math
from collections import namedtuple
from pathlib import Path

import numpy as np


def _default_encoder_path(path):
    return Path(__file__).resolve().parent.parent / "ace_encoder_pretrained.pt" if str(path) == "<path>" else Path(path)


def frame_size_classes(rgb_glob):
    """The sorted file list grouped by image size (header reads only): {(W, H): [positions in the sorted list]}. One size means
    one resize factor and one resized shape for load_frames. The reference's batch-size-1 loaders take any mix (dataset.py:278-417)."""
    import glob
    from PIL import Image
    files = sorted(glob.glob(rgb_glob))
    if not files:
        raise SystemExit(f"no files match {rgb_glob!r}")
    classes = {}
    for i, f in enumerate(files):
        with Image.open(f) as im:
            classes.setdefault(im.size, []).append(i)
    return files, classes


def load_frames(rgb_glob, image_resolution=480, files=None, return_rgb=False, size_classes=False):
    """Minimal stand-in for CamLocDataset's image path without augmentation (dataset.py:189-195,227-237,146-160): decode,
    resize so that the short side is `image_resolution` (PIL bilinear, as torchvision does for PIL images), grey, normalise.
    Focal lengths on the command line and in pose files refer to the ORIGINAL image size and are multiplied by the frame's resize
    factor (dataset.py:289-290). Every size class (frames of one resized shape) passes check_frame_size before any of its frames
    is decoded.

    Default: all frames must have one size. Returns (files, float32 [n,1,H,W], resize factor[, uint8 rgb [n,H,W,3]]).
    size_classes=True: any mix of sizes (the reference's batch-size-1 loaders take one, dataset.py:278-417). Returns (files,
    classes, factors[, rgb]): classes = [(positions in the sorted file list, float32 [k,1,H_c,W_c]), ...] in the order of their
    first frame, factors = float64 [n] resize factor of every frame, rgb = a list of n uint8 [H_i,W_i,3] arrays -- what
    ReconstructionSession takes for a folder of mixed sizes."""
    import glob
    import torch
    from PIL import Image
    from .session import check_frame_size
    if files is None:
        files = sorted(glob.glob(rgb_glob))                             # dataset_io.get_files_from_glob sorts
    if not files:
        raise SystemExit(f"no files match {rgb_glob!r}")
    frames, factors, rgbs, shapes = [], [], [], {}
    for i, f in enumerate(files):
        im = Image.open(f)
        w, h = im.size
        sc = image_resolution / min(w, h)
        nw, nh = (image_resolution, int(h * sc)) if w <= h else (int(w * sc), image_resolution)
        if (nh, nw) not in shapes:
            if shapes and not size_classes:
                size = next(iter(shapes))
                raise SystemExit(f"{f}: resized frame is {(nh, nw)}, the first one {size}: frames of ONE size were expected (load_frames("
                                 "size_classes=True) takes a mix; the entry points do)")
            try:
                check_frame_size(nh, nw)                                 # before the class's frames are decoded
            except RuntimeError as e:
                raise SystemExit(str(e))
            shapes[(nh, nw)] = []
        shapes[(nh, nw)].append(i)
        small = im.convert("RGB").resize((nw, nh), Image.BILINEAR)
        g = np.asarray(small.convert("L"), np.float32) / 255.0
        if return_rgb:
            rgbs.append(np.asarray(small, np.uint8))
        frames.append((g - 0.4) / 0.25)
        factors.append(sc)
    if not size_classes:
        out = (files, torch.from_numpy(np.stack(frames)[:, None]), factors[-1])
        return out + (np.stack(rgbs),) if return_rgb else out
    classes = [(np.array(pos, np.int64), torch.from_numpy(np.stack([frames[i] for i in pos])[:, None])) for pos in shapes.values()]
    out = (files, classes, np.array(factors, np.float64))
    return out + (rgbs,) if return_rgb else out


def load_session_frames(rgb_glob, image_resolution=480, files=None, return_rgb=False):
    """load_frames for the entry points: a folder of one size comes back exactly as load_frames returns it (files, [n,1,H,W],
    resize factor[, rgb [n,H,W,3]]), a folder of mixed sizes as load_frames(size_classes=True) returns it (files, classes, per-frame
    factors[, per-frame rgb list])."""
    out = load_frames(rgb_glob, image_resolution, files=files, return_rgb=return_rgb, size_classes=True)
    if len(out[1]) > 1:
        return out
    files, classes, factors = out[:3]
    one = (files, classes[0][1], float(factors[-1]))
    return one + (np.stack(out[3]),) if return_rgb else one


def initial_focals(frames, factors, external=None, heuristic=False, file_focals=None):
    """Per-frame initial focal lengths in resized pixels of a folder of size classes (`frames`, `factors` as load_frames(size_classes=True)
    returns them): an external focal or the pose file's focals (original-image pixels) times the frame's factor (dataset.py:289-290),
    else 70% of the resized frame's diagonal (dataset.py:269-274)."""
    n = len(factors)
    out = np.zeros(n, np.float64)
    for pos, t in frames:
        h, w = t.shape[2:]
        for i in pos:
            if external is not None and external > 0:
                out[i] = external * factors[i]
            elif heuristic or file_focals is None or not len(file_focals):
                out[i] = math.sqrt(w ** 2 + h ** 2) * 0.7
            else:
                out[i] = file_focals[i] * factors[i]
    return out


def focals_in_original_units(focal, frel, factors):
    """Per-frame focal lengths for pose files, in each frame's ORIGINAL-image pixels: the session's nominal focal x the frame's ratio
    (ReconstructionSession.frel), divided by the frame's resize factor (dataset.py:289-290 the other way round)."""
    return focal * np.asarray(frel, np.float64) / np.asarray(factors, np.float64)


def check_single_focal(focals_original):
    """ace_zero.py:301-302 hands ONE focal (original-image pixels) from round to round and asserts that every frame has it."""
    if not np.allclose(focals_original, focals_original[0]):
        raise SystemExit("ace_zero.py supports a single focal length (ace_zero.py:301-302): the frames' focal lengths differ in original-image "
                         "pixels (pass --use_external_focal_length, or map the frames of each camera separately)")


def check_calibration_focals(focals):
    """refine_calibration.py:14-15: calibration refinement learns ONE focal; every frame must start from the same one."""
    if not np.allclose(focals, focals[0]):
        raise SystemExit("All images must have the same focal length for calibration refinement")


def load_depth_maps(depth_glob, n, frame_hw):
    """--depth_files (dataset.py:299-304,333,359): 16-bit millimetres -> metres, nearest resize to the frame, value at the
    feature-map pixel centres (offset 4, stride 8). frame_hw = (H, W) of every frame: float32 [n, ceil(H/8), ceil(W/8)]; or a list
    of n per-frame (H_i, W_i) (a folder of mixed sizes): a list of n float32 [ceil(H_i/8), ceil(W_i/8)] maps."""
    import glob
    import torch
    files = sorted(glob.glob(depth_glob))
    if len(files) != n:
        raise SystemExit(f"{len(files)} depth files for {n} images")
    one = depth_map_at_cells
    if isinstance(frame_hw, list):
        return [torch.from_numpy(one(f, int(h), int(w))) for f, (h, w) in zip(files, frame_hw)]
    H, W = frame_hw
    return torch.from_numpy(np.stack([one(f, H, W) for f in files]) if n else np.zeros((0, (H + 7) // 8, (W + 7) // 8), np.float32))


def depth_map_at_cells(path, H, W):
    """One depth file (16-bit millimetres) -> metres, nearest resize to the H x W frame, value at the feature-map pixel centres
    (offset 4, stride 8): float32 [ceil(H/8), ceil(W/8)]."""
    from PIL import Image
    d = np.asarray(Image.open(path).resize((W, H), Image.NEAREST), np.float32) / 1000.0
    sub = d[4::8, 4::8]
    out = np.zeros(((H + 7) // 8, (W + 7) // 8), np.float32)
    out[:sub.shape[0], :sub.shape[1]] = sub
    return out


def frame_shapes(frames, n):
    """(H, W) of every frame of a folder of size classes."""
    hw = [None] * n
    for pos, t in frames:
        for i in pos:
            hw[i] = tuple(t.shape[2:])
    return hw


class SessionFrames(namedtuple("SessionFrames", ["files", "frames", "factors", "rgb", "mixed", "frame_focals", "focal", "hw"])):
    """session_frames' result: files, frames, factors and rgb (None unless asked for) as the loader returns them, for one frame size
    or (mixed) several; frame_focals: what ReconstructionSession takes as focals= (None for one size); focal: the nominal initial
    focal in resized pixels (mixed: frame 0's); hw: what load_depth_maps takes."""

    def original_focals(self, focal, frel):
        """Every frame's focal in its own ORIGINAL-image pixels (pose files) from the session's nominal focal and its frel."""
        return focals_in_original_units(focal, frel, self.factors) if self.mixed else np.full(len(self.files), focal / self.factors)


def session_frames(load, rgb_glob, image_resolution, files=None, external=None, heuristic=False, file_focals=(), return_rgb=False):
    """The frames of a session (load: load_session_frames or its device twin) and their focals from `external` (None: not given) or
    file_focals, both in original-image pixels. One size: ONE resize factor, the last frame's, converts every focal: external x
    factor, else (heuristic, or no file focals) 70% of the diagonal (dataset.py:269-274), else the file's focal x factor
    (dataset.py:289-290), which all entries must share. Several sizes: initial_focals, every frame with its own factor."""
    import torch
    files, frames, factors, *rgb = load(rgb_glob, image_resolution, files=files, return_rgb=return_rgb)
    rgb = rgb[0] if rgb else None
    if not torch.is_tensor(frames):                                      # a folder of several frame sizes: its size classes
        frame_focals = initial_focals(frames, factors, external=external, heuristic=heuristic, file_focals=file_focals)
        return SessionFrames(files, frames, factors, rgb, True, frame_focals, float(frame_focals[0]), frame_shapes(frames, len(files)))
    H, W = frames.shape[2:]
    if external is not None:
        focal = external * factors
    elif heuristic or not len(file_focals):
        focal = math.sqrt(W ** 2 + H ** 2) * 0.7
    else:
        assert np.allclose(file_focals, file_focals[0]), "a single focal length is supported"
        focal = file_focals[0] * factors
    return SessionFrames(files, frames, factors, rgb, False, None, focal, frames.shape[2:])
