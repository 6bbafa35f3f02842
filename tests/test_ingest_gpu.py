"""GPU: the ingest kernels (acez_ingest_frames) against Pillow and cli.load_frames, bit for bit; the device loader against the host
loader on a folder of mixed sizes; an entry-point scenario with and without --gpu_ingest."""
import numpy as np
import pytest
import torch

from acezero_amd import cli, ingest
from tests import ingest_restated as R

pytestmark = pytest.mark.gpu


def _save(path, rgb):
    from PIL import Image
    Image.fromarray(rgb).save(path, compress_level=1)


_reference = {}


def _host_reference(tmp_path_factory, h, w, res):
    """Six frames of one case (three different noise frames, all 0, all 255, one more noise frame) through cli.load_frames itself:
    (uint8 [6, h, w, 3] sources, uint8 [6, nh, nw, 3] Pillow's resized RGB, float32 [6, 1, nh, nw] load_frames' frames). Computed once."""
    if (h, w, res) not in _reference:
        d = tmp_path_factory.mktemp(f"ingest_{h}_{w}_{res}")
        noise = R.frames(h, w, "noise", n=4, seed=7)
        src = np.concatenate([noise[:3], R.frames(h, w, "zeros"), R.frames(h, w, "full"), noise[3:]])
        for i in range(len(src)):
            _save(d / f"f{i}.png", src[i])
        _, frames, _, rgb = cli.load_frames(str(d / "f*.png"), image_resolution=res, return_rgb=True)
        assert tuple(frames.shape[2:]) == R.resized_size(h, w, res)
        _reference[(h, w, res)] = (src, rgb, frames)
    return _reference[(h, w, res)]


@pytest.mark.parametrize("with_rgb", [True, False])
@pytest.mark.parametrize("h,w,res", R.CASES)
def test_kernels_equal_pillow_and_load_frames(tmp_path_factory, h, w, res, with_rgb):
    src, want_rgb, want_grey = _host_reference(tmp_path_factory, h, w, res)
    nh, nw = want_grey.shape[2:]
    for lo in (0, 3):                                                    # three different frames per call: a wrong frame stride shows
        d_src = torch.from_numpy(src[lo:lo + 3]).cuda()
        grey, rgb = ingest.ingest_frames(d_src, nh, nw, want_rgb=with_rgb)
        assert grey.dtype == torch.float32 and tuple(grey.shape) == (3, 1, nh, nw)
        assert torch.equal(grey.cpu(), want_grey[lo:lo + 3])
        if with_rgb:
            assert np.array_equal(rgb.cpu().numpy(), want_rgb[lo:lo + 3])
        else:
            assert rgb is None


def test_all_255_stays_255_and_all_0_stays_0(tmp_path_factory):
    """Rounding and the clip at the top of the range: taps that sum to a little over 2^22 must not wrap."""
    _, want_rgb, _ = _host_reference(tmp_path_factory, 480, 640, 16)
    assert (want_rgb[3] == 0).all() and (want_rgb[4] == 255).all()
    d_src = torch.from_numpy(np.concatenate([R.frames(480, 640, "zeros"), R.frames(480, 640, "full")])).cuda()
    grey, rgb = ingest.ingest_frames(d_src, 16, 21)
    assert (rgb[0] == 0).all() and (rgb[1] == 255).all()
    t = ingest.normalisation_table()
    assert (grey[0] == float(t[0])).all() and (grey[1] == float(t[255])).all()


def test_device_entry_refuses_bad_arguments_on_the_gpu_box():
    from acezero_amd import _native as N
    lib = N.lib()
    buf = torch.zeros(1 << 12, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert lib.acez_ingest_frames(p, 1, 8, 8, 8, 8, p, p, 4 * 80 - 1, p, None, p, None) == -1
    assert lib.acez_ingest_frames(p, 1, 8, 8, 8, 8, None, p, 1 << 12, p, None, p, None) == -1
    assert lib.acez_ingest_frames(p, 0, 8, 8, 8, 8, p, p, 1 << 12, p, None, p, None) == -1
    with pytest.raises(RuntimeError, match="device frames"):
        ingest.ingest_frames(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 8, 8)


# (h, w) of the source: the first two resize to one shape (16 x 24), the third is portrait (24 x 16)
_SIZES = [(32, 48), (64, 96), (48, 32)]


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = tmp_path_factory.mktemp("ingest_folder")
    order = [0, 1, 0, 2, 1, 1, 0, 2, 2, 0, 1, 0, 0]                      # the shared class interleaves its two source sizes
    for i, k in enumerate(order):
        h, w = _SIZES[k]
        _save(d / f"im_{i:02d}.png", R.frames(h, w, "noise", seed=100 + i)[0])
    return d, order


def _same_loaded(dev, host):
    files, classes, factors, rgb = dev
    hfiles, hclasses, hfactors, hrgb = host
    assert files == hfiles
    assert factors.dtype == hfactors.dtype and np.array_equal(factors, hfactors)
    assert len(classes) == len(hclasses)
    for (pos, t), (hpos, ht) in zip(classes, hclasses):
        assert pos.dtype == hpos.dtype and np.array_equal(pos, hpos)
        assert t.is_cuda and t.dtype == ht.dtype and t.shape == ht.shape and t.is_contiguous()
        assert torch.equal(t.cpu(), ht)
    assert len(rgb) == len(hrgb)
    for a, b in zip(rgb, hrgb):
        assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and np.array_equal(a, b)


@pytest.mark.parametrize("chunk_frames,workers", [(2, 3), (64, 1), (1, 16)])
def test_loader_equals_load_frames_on_mixed_sizes(folder, chunk_frames, workers):
    d, _ = folder
    host = cli.load_frames(str(d / "im_*.png"), 16, return_rgb=True, size_classes=True)
    dev = ingest.load_frames_device(str(d / "im_*.png"), 16, return_rgb=True, size_classes=True, workers=workers, chunk_frames=chunk_frames)
    assert [tuple(t.shape[2:]) for _, t in dev[1]] == [(16, 24), (24, 16)]
    _same_loaded(dev, host)
    # without rgb, and through the entry points' loader
    h3 = cli.load_session_frames(str(d / "im_*.png"), 16)
    d3 = ingest.load_session_frames_device(str(d / "im_*.png"), 16, workers=workers)
    assert len(d3) == len(h3) == 3 and d3[0] == h3[0] and np.array_equal(d3[2], h3[2])
    assert all(np.array_equal(a[0], b[0]) and torch.equal(a[1].cpu(), b[1]) for a, b in zip(d3[1], h3[1]))


def test_loader_of_one_size_crosses_chunks_and_equals_load_frames(folder):
    d, order = folder
    files = [str(d / f"im_{i:02d}.png") for i, k in enumerate(order) if k == 0]
    assert len(files) == 6
    hf, hframes, hfactor, hrgb = cli.load_frames(None, 16, files=files, return_rgb=True)
    for chunk in (4, 64):                                                # 6 frames in chunks of 4 + 2, and in one
        df, dframes, dfactor, drgb = ingest.load_frames_device(None, 16, files=files, return_rgb=True, chunk_frames=chunk)
        assert df == hf and dfactor == hfactor and dframes.is_cuda and torch.equal(dframes.cpu(), hframes)
        assert drgb.dtype == np.uint8 and np.array_equal(drgb, hrgb)
    a = ingest.load_session_frames_device(None, 16, files=files, return_rgb=True)
    b = cli.load_session_frames(None, 16, files=files, return_rgb=True)
    assert a[0] == b[0] and torch.equal(a[1].cpu(), b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])


def test_loader_refusals_are_the_host_loader_s(folder, tmp_path):
    d, _ = folder
    with pytest.raises(SystemExit) as host:
        cli.load_frames(str(d / "im_*.png"), 16)
    with pytest.raises(SystemExit) as dev:
        ingest.load_frames_device(str(d / "im_*.png"), 16)
    assert str(dev.value) == str(host.value) and "frames of ONE size were expected" in str(dev.value)
    with pytest.raises(SystemExit) as host:
        cli.load_frames(str(tmp_path / "none_*.png"), 16)
    with pytest.raises(SystemExit) as dev:
        ingest.load_frames_device(str(tmp_path / "none_*.png"), 16)
    assert str(dev.value) == str(host.value)
    _save(tmp_path / "big.png", np.zeros((8, 8, 3), np.uint8))           # 1100 x 1100 px resized: more scene coordinates than RANSAC takes
    with pytest.raises(SystemExit) as host:
        cli.load_frames(str(tmp_path / "big.png"), 1100)
    with pytest.raises(SystemExit) as dev:
        ingest.load_frames_device(str(tmp_path / "big.png"), 1100)
    assert str(dev.value) == str(host.value) and "16384" in str(dev.value)


def test_entry_points_write_the_same_pose_files_with_gpu_ingest(tmp_path):
    """The scenario of tests/test_dsac_rgbd_gpu.py::test_register_mapping_rgbd_end_to_end (train_ace.py on PNG frames + depth, then
    register_mapping_rgbd.py), once on the host path and once with --gpu_ingest True: identical pose files, byte for byte."""
    from PIL import Image
    from acezero_amd import synth
    n = 16
    seq = synth.render_room_sequence(seed=5, n_frames=n, arc_deg=15.0, device="cuda")
    for i in range(n):
        img = ((seq["images"][i, 0] * 0.25 + 0.4).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
        Image.fromarray(np.stack([img] * 3, -1)).save(tmp_path / f"rgb_{i:04d}.png")
        dep = (seq["depth"][i].cpu().numpy() * 1000).round().astype(np.uint16)
        Image.fromarray(np.kron(dep, np.ones((8, 8), np.uint16))).save(tmp_path / f"depth_{i:04d}.png")
        np.savetxt(tmp_path / f"pose_{i:04d}.txt", seq["poses"][i].cpu().numpy().astype(np.float64))
    torch.save({k: torch.from_numpy(v) for k, v in synth.init_encoder_weights_bandpass(seed=4099).items()}, tmp_path / "encoder.pt")
    f = str(seq["focal"])
    written = {}
    for tag, extra in (("host", []), ("device", ["--gpu_ingest", "True", "--num_data_workers", "4"])):
        out = tmp_path / tag / "scene.pt"
        assert cli.train_main([str(tmp_path / "rgb_*.png"), str(out), "--pose_files", str(tmp_path / "pose_*.txt"), "--depth_files",
                               str(tmp_path / "depth_*.png"), "--encoder_path", str(tmp_path / "encoder.pt"), "--use_external_focal_length", f,
                               "--iterations", "1500", "--learning_rate_cooldown_iterations", "300", "--aug_rotation", "2"] + extra) == 0
        assert cli.register_rgbd_main([str(tmp_path / "rgb_*.png"), str(out), "--depth_files", str(tmp_path / "depth_*.png"), "--encoder_path",
                                       str(tmp_path / "encoder.pt"), "--session", "rgbd", "--use_external_focal_length", f] + extra) == 0
        written[tag] = [open(tmp_path / tag / name, "rb").read() for name in ("poses_scene_preliminary.txt", "poses_rgbd.txt")]
        assert len(written[tag][1].splitlines()) == n
    assert written["host"] == written["device"]
