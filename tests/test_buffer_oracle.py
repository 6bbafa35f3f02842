"""Properties of the training-buffer sampling oracle (ace_trainer.py:404-431 restated in oracle/buffer_oracle.py)."""
import numpy as np

from oracle import buffer_oracle as bo


def test_draws_are_uniform_over_valid_pixels_with_replacement():
    rng = np.random.default_rng(0)
    mask = rng.uniform(size=(12, 16)) < 0.4
    mask[0, 0] = True
    pix = bo.sample_view(mask, 20000, seed=2089, view_id=3)
    valid = np.flatnonzero(mask.reshape(-1))
    assert set(np.unique(pix)) <= set(valid)                 # only valid pixels
    counts = np.array([(pix == v).sum() for v in valid])
    assert counts.min() > 0                                   # all of them reachable
    exp = 20000 / len(valid)
    chi2 = float(((counts - exp) ** 2 / exp).sum())
    assert chi2 < 2.0 * len(valid)                            # ~ chi-square with len(valid)-1 dof
    assert len(np.unique(pix)) < len(pix)                     # with replacement


def test_stream_is_keyed_by_view_and_sample_not_by_batching():
    mask = np.ones((6, 8), bool)
    a = bo.sample_view(mask, 64, 7, view_id=5)
    b = bo.sample_view(mask, 32, 7, view_id=5)
    assert np.array_equal(a[:32], b)
    assert not np.array_equal(a, bo.sample_view(mask, 64, 7, view_id=6))
    assert not np.array_equal(a, bo.sample_view(mask, 64, 8, view_id=5))


def test_target_pixels_are_cell_centres():
    px = bo.target_px(np.array([0, 1, 8, 17]), w=8)
    assert np.array_equal(px, np.array([[4, 4], [12, 4], [4, 12], [12, 20]], np.float32))   # ace_util.py:7-13


def test_one_valid_cell_takes_every_draw():
    for at in (0, 30 * 40 - 1):                                # the first and the last index
        mask = np.zeros((30, 40), np.uint8)
        mask.reshape(-1)[at] = 1
        assert (bo.sample_view(mask, 500, 2089, 3) == at).all()


def test_largest_map_stays_in_range_and_reaches_its_last_cell():
    hw = 128 * 192                                             # 24576 cells: what the kernel's LDS prefix holds
    pix = bo.sample_view(np.ones((128, 192), np.uint8), 200000, 2089, 3)
    assert pix.min() >= 0 and pix.max() == hw - 1 and pix.min() == 0
    # k = (r * n) >> 32 with r < 2^32 can never reach n
    assert (0xFFFFFFFF * hw) >> 32 == hw - 1


def test_keys_are_64_bit():
    mask = np.ones((30, 40), bool)
    seed, view = 2 ** 63 + 5, 2 ** 40 + 3
    a = bo.sample_view(mask, 64, seed, view)
    assert not np.array_equal(a, bo.sample_view(mask, 64, seed & 0xFFFFFFFF, view))
    assert not np.array_equal(a, bo.sample_view(mask, 64, seed, view & 0xFFFFFFFF))
    assert not np.array_equal(a, bo.sample_view(mask, 64, seed & 0xFFFFFFFF, view & 0xFFFFFFFF))
    assert a.min() >= 0 and a.max() < 1200
