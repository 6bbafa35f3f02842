"""CPU: the host side of the device ingest path (include/acez.h section I, acezero_amd/ingest.py). The library's resize tables equal
the numpy restatement of Pillow's arithmetic entry for entry, the restatement equals the installed Pillow bit for bit, the
normalisation table is cli.load_frames' expression, the threaded decoder keeps file order, and nothing runs without a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from acezero_amd import _native as N
from acezero_amd import cli, ingest
from tests import ingest_restated as R


@pytest.mark.parametrize("h,w,res", R.CASES)
def test_library_tables_equal_the_restatement(h, w, res):
    nh, nw = R.resized_size(h, w, res)
    for n_in, n_out in ((w, nw), (h, nh)):
        ks, bounds, taps = ingest.axis_coeffs(n_in, n_out)
        rks, rbounds, rtaps = R.coeffs(n_in, n_out)
        assert ks == rks, (n_in, n_out)
        assert np.array_equal(bounds, rbounds), (n_in, n_out)
        assert np.array_equal(taps, rtaps), (n_in, n_out)
        # what the kernels rely on: every tap inside the source, none negative, an int32 accumulator is enough
        assert bounds[:, 0].min() >= 0 and (bounds[:, 0] + bounds[:, 1]).max() <= n_in and bounds[:, 1].max() <= ks
        assert taps.min() >= 0 and 255 * int(taps.sum(1).max()) + (1 << 21) < 2 ** 31
    assert ingest.table_bytes(h, w, nh, nw) == 4 * (nw * (2 + R.coeffs(w, nw)[0]) + nh * (2 + R.coeffs(h, nh)[0]))


def test_scale_30_has_61_taps():
    assert ingest.axis_coeffs(480, 16)[0] == 61


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("h,w,res", R.CASES)
def test_restatement_equals_pillow(h, w, res, content):
    nh, nw = R.resized_size(h, w, res)
    src = R.frames(h, w, content)[0]
    want_rgb, want_grey = R.pillow_resize(src, nh, nw)
    got = R.resize_bilinear(src, nh, nw)
    assert np.array_equal(got, want_rgb)
    assert np.array_equal(R.to_grey(got), want_grey)


def test_normalisation_table_is_the_host_expression():
    t = ingest.normalisation_table()
    assert t.dtype == np.float32 and t.shape == (256,)
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    want = (np.asarray(g, np.float32) / 255.0 - 0.4) / 0.25            # cli.load_frames, line for line
    assert np.array_equal(t[g].view(np.uint32), want.view(np.uint32))


def test_normalisation_table_gives_load_frames_values(tmp_path):
    """Every grey value through cli.load_frames itself: a 16 x 16 grey ramp saved at the resolution it is loaded at."""
    from PIL import Image
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    Image.fromarray(np.stack([g] * 3, -1)).save(tmp_path / "ramp.png")
    _, frames, _ = cli.load_frames(str(tmp_path / "ramp.png"), image_resolution=16)
    assert np.array_equal(frames[0, 0].numpy().view(np.uint32), ingest.normalisation_table()[g].view(np.uint32))


@pytest.mark.parametrize("workers", [1, 3, 16])
def test_decode_frames_keeps_file_order(tmp_path, workers):
    from PIL import Image
    files = []
    for i in range(20):
        files.append(str(tmp_path / f"f{i:02d}.png"))
        Image.fromarray(np.full((8 + i % 3, 12, 3), i, np.uint8)).save(files[-1])
    order = files[::-1][:7] + files[:13]
    out = ingest.decode_frames(order, workers)
    assert len(out) == 20
    for f, a in zip(order, out):
        i = int(os.path.basename(f)[1:3])
        assert a.dtype == np.uint8 and a.shape == (8 + i % 3, 12, 3) and (a == i).all()
    assert 1 <= ingest.pool_size(workers) <= min(workers, 16, len(os.sched_getaffinity(0)))
    assert ingest.pool_size(0) == 1 and ingest.pool_size(1000) <= 16


def test_decode_frames_names_the_undecodable_file(tmp_path):
    from PIL import Image
    good = str(tmp_path / "a.png")
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(good)
    bad = str(tmp_path / "broken.png")
    with open(bad, "wb") as f:
        f.write(b"not an image")
    with pytest.raises(SystemExit, match="broken.png"):
        ingest.decode_frames([good, bad, good], 3)


def test_invalid_arguments_are_refused_before_any_device_work():
    lib = N.lib()
    a = np.zeros(64, np.uint8).ctypes.data                               # never dereferenced: every call below is refused first
    ok = dict(src=a, n=1, H=8, W=8, nh=8, nw=8, tmp=a, tables=a, nbytes=1 << 20, norm=a, rgb=None, grey=a)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.acez_ingest_frames(v["src"], v["n"], v["H"], v["W"], v["nh"], v["nw"], v["tmp"], v["tables"], v["nbytes"], v["norm"],
                                      v["rgb"], v["grey"], None)
    for name in ("src", "tmp", "tables", "norm", "grey"):
        assert call(**{name: None}) == -1, name
    for name in ("n", "H", "W", "nh", "nw"):
        assert call(**{name: 0}) == -1 and call(**{name: -3}) == -1, name
    assert call(n=65536) == -1 and call(W=32769) == -1
    assert call(nbytes=4 * (8 * 5 + 8 * 5) - 1) == -1                    # one byte short of the two 8 -> 8 tables (ksize 3)
    assert b"table block too small" in lib.acez_last_error()
    # sizes that session.check_frame_size refuses: more than 16384 scene coordinates
    assert call(H=2000, W=2000, nh=1032, nw=1024) == -1 and b"16384" in lib.acez_last_error()
    from acezero_amd.session import check_frame_size
    with pytest.raises(RuntimeError):
        check_frame_size(1032, 1024)
    check_frame_size(1024, 1024)
    ks = C.c_int(0)
    assert lib.acez_ingest_coeffs(0, 4, C.byref(ks), None, None) == -1 and lib.acez_ingest_coeffs(4, 0, C.byref(ks), None, None) == -1
    assert lib.acez_ingest_coeffs(4, 4, None, None, None) == -1
    assert lib.acez_ingest_coeffs(8, 8, C.byref(ks), None, None) == 0 and ks.value == 3


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_no_device_no_ingest(tmp_path):
    from PIL import Image
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(tmp_path / "a.png")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.load_frames_device(str(tmp_path / "*.png"), 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.load_session_frames_device(str(tmp_path / "*.png"), 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ingest.ingest_frames(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), 16, 16)
    lib = N.lib()
    a = np.zeros(1 << 12, np.uint8).ctypes.data
    assert lib.acez_ingest_frames(a, 1, 8, 8, 8, 8, a, a, 1 << 12, a, None, a, None) == -3   # valid arguments, no device: nothing runs
    assert b"no HIP device" in lib.acez_last_error()


def test_entry_points_take_gpu_ingest_and_keep_their_pinned_surfaces(tmp_path):
    base = {"train": (cli.train_parser, ["a/*.png", "out.pt"]), "register": (cli.register_parser, ["a/*.png", "net.pt"]),
            "rgbd": (cli.register_rgbd_parser, ["a/*.png", "net.pt", "--depth_files", "d/*.png"]),
            "ace_zero": (cli.ace_zero_cli_parser, ["a/*.png", str(tmp_path)]), "export": (cli.export_point_cloud_parser, ["pc.txt"])}
    for name, (make, argv) in base.items():
        assert not hasattr(make().parse_args(argv), "gpu_ingest"), name
        p = cli.with_ingest_flag(make())
        assert p.parse_args(argv).gpu_ingest is False, name
        assert p.parse_args(argv + ["--gpu_ingest", "True"]).gpu_ingest is True, name
    off = cli.train_parser().parse_args(base["train"][1])
    assert cli._frame_loaders(off) == (cli.load_frames, cli.load_session_frames)           # the default path is the host one, untouched
    on = cli.with_ingest_flag(cli.train_parser()).parse_args(base["train"][1] + ["--gpu_ingest", "True", "--num_data_workers", "5"])
    lf, lsf = cli._frame_loaders(on)
    assert lf.func is ingest.load_frames_device and lsf.func is ingest.load_session_frames_device
    assert lf.keywords == {"workers": 5} and lsf.keywords == {"workers": 5}
