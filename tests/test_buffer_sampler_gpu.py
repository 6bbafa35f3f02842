"""The buffer sampler (sample_one_view of buffer_api.hip, through acez_buffer_sample_views and acez_buffer_sample_views_table) against
oracle/buffer_oracle.py at the sizes where its code takes another path: a production map (19 cells per thread, 4 workgroups per view),
cell counts one over and one under the workgroup size, the largest map the LDS prefix holds (full and with only its tail valid), one
valid cell, mask bytes other than 1, rows wider and narrower than one trip of the channel loop, the cap of 64 workgroups per view, one
sample, 64-bit keys, a view without a valid cell, and the table entry point's maps in any order, mixed sizes and refusals.

Every assertion is an equality. Features are int16 rows whose value is a function of (view, cell, channel), so a row copied from the
wrong cell or view, or shifted by a channel, differs. Every output is poisoned before the call and has 64 poisoned guard rows behind."""
import ctypes as C

import numpy as np
import pytest
import torch

from acezero_amd import _native as N
from oracle import buffer_oracle as bo

pytestmark = pytest.mark.gpu

GUARD = 64
P_FEAT, P_PX, P_IDX = 0x7fff, -1.0, -1        # poison: no feature is 32767, no target pixel negative, no view index or pixel id negative
JUNK = 31000                                  # rows of a store that belong to no view


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def features(view, hw, ch):
    """int16 [hw, ch] in [-30000, 29999]: a function of (view, cell, channel) in which neighbouring cells, views and channels differ."""
    p = np.arange(hw, dtype=np.int64)[:, None]
    c = np.arange(ch, dtype=np.int64)[None, :]
    return ((view * 7919 + p * 31 + c * 17 + (p * c) % 13) % 60000 - 30000).astype(np.int16)


def _density(rng, n, hw, d):
    m = (rng.uniform(size=(n, hw)) < d).astype(np.uint8)
    m[:, hw // 2] = 1
    return m


def _single(n, hw, at):
    m = np.zeros((n, hw), np.uint8)
    m[:, at] = 1
    return m


def _tail(n, hw, k):
    m = np.zeros((n, hw), np.uint8)
    m[:, hw - k:] = 1
    return m


def _bytes(rng, n, hw):
    return _density(rng, n, hw, 0.5) * rng.choice(np.array([2, 128, 255], np.uint8), size=(n, hw))


def _empty_middle(rng, n, hw):
    m = _density(rng, n, hw, 0.5)
    m[1] = 0
    return m


# name -> (h, w, samples, channels, views, mask(rng, views, hw) or None, seed, first_view_id, view_index_base)
CASES = {
    "production": (60, 80, 1024, 512, 2, lambda r, n, hw: _density(r, n, hw, 0.7), 2089, 10, 7),            # per = 19, 4 workgroups
    "one_over": (1, 257, 300, 8, 2, lambda r, n, hw: _density(r, n, hw, 0.5), 2089, 10, 7),                  # per = 2, slices past the end, 150 + 150
    "one_under": (1, 255, 257, 8, 2, None, 2089, 10, 7),                                                     # per = 1, an idle thread, 129 + 128
    "largest": (128, 192, 300, 8, 2, lambda r, n, hw: np.ones((n, hw), np.uint8), 2089, 10, 7),              # pref up to 24576, per = 96
    "largest_sparse": (128, 192, 300, 8, 2, lambda r, n, hw: _tail(n, hw, 50), 2089, 10, 7),                 # the search ends in the tail
    "single_first": (30, 40, 64, 16, 2, lambda r, n, hw: _single(n, hw, 0), 2089, 10, 7),                    # nvalid = 1
    "single_last": (30, 40, 64, 16, 2, lambda r, n, hw: _single(n, hw, hw - 1), 2089, 10, 7),
    "byte_values": (30, 40, 256, 16, 2, _bytes, 2089, 10, 7),                                                # the != 0 rule
    "wide_1024": (6, 8, 70, 1024, 2, None, 2089, 10, 7),                                                     # a second trip of the channel loop
    "wide_520": (6, 8, 70, 520, 2, None, 2089, 10, 7),                                                       # and a partial one
    "split_cap": (6, 8, 16385, 8, 2, lambda r, n, hw: _density(r, n, hw, 0.5), 2089, 10, 7),                 # 64 workgroups of 257 samples
    "one_sample": (6, 8, 1, 8, 2, None, 2089, 10, 7),
    "keys": (30, 40, 128, 8, 3, lambda r, n, hw: _density(r, n, hw, 0.5), 2 ** 63 + 5, 2 ** 40 + 3, 1000003),
    "empty_view": (30, 40, 64, 8, 3, _empty_middle, 2089, 10, 7),                                            # view 1: the documented early return
}


def _case(name):
    h, w, S, ch, n, mk, seed, fid, base = CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    mask = mk(rng, n, h * w) if mk is not None else None
    feats = [features(v, h * w, ch) for v in range(n)]
    return h, w, S, ch, n, mask, feats, seed, fid, base


class Outputs:
    """The four output arrays of a launch of n views x S samples, poisoned, with GUARD poisoned rows behind each."""

    def __init__(self, n, S, ch):
        rows = n * S + GUARD
        self.n, self.S, self.ch = n, S, ch
        self.feat = torch.full((rows, ch), P_FEAT, dtype=torch.int16, device="cuda")
        self.px = torch.full((rows, 2), P_PX, dtype=torch.float32, device="cuda")
        self.view = torch.full((rows,), P_IDX, dtype=torch.int32, device="cuda")
        self.pix = torch.full((rows,), P_IDX, dtype=torch.int32, device="cuda")

    def ptrs(self):
        return [_p(self.feat), _p(self.px), _p(self.view), _p(self.pix)]

    def check(self, expect):
        """expect[v] = None (the view's rows keep their poison) or (mask [hw] or None, feats [hw,ch], w, seed, view id, view index)."""
        torch.cuda.synchronize()
        feat, px, view, pix = (t.cpu().numpy() for t in (self.feat, self.px, self.view, self.pix))
        n, S = self.n, self.S
        assert (feat[n * S:] == P_FEAT).all() and (px[n * S:] == P_PX).all() and (view[n * S:] == P_IDX).all() and (pix[n * S:] == P_IDX).all()
        for v, e in enumerate(expect):
            sl = slice(v * S, (v + 1) * S)
            if e is None:
                assert (feat[sl] == P_FEAT).all() and (px[sl] == P_PX).all() and (view[sl] == P_IDX).all() and (pix[sl] == P_IDX).all(), v
                continue
            mask, feats, w, seed, view_id, view_index = e
            ref = bo.sample_view(mask if mask is not None else np.ones(len(feats), np.uint8), S, seed, view_id)
            assert np.array_equal(pix[sl], ref), v
            assert np.array_equal(feat[sl], feats[ref]), v
            assert np.array_equal(px[sl], bo.target_px(ref, w)), v
            assert (view[sl] == view_index).all(), v
            assert not (feat[sl] == P_FEAT).any() and not (px[sl] == P_PX).any(), v


def _expect(h, w, n, mask, feats, seed, fid, base):
    out = []
    for v in range(n):
        m = mask[v] if mask is not None else None
        out.append(None if m is not None and not m.any() else (m, feats[v], w, seed, fid + v, base + v))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_one_size_sampler_equals_the_oracle(name):
    h, w, S, ch, n, mask, feats, seed, fid, base = _case(name)
    d_feat = torch.from_numpy(np.concatenate(feats)).cuda()
    d_mask = torch.from_numpy(mask).cuda().contiguous() if mask is not None else None
    out = Outputs(n, S, ch)
    N.check(N.lib().acez_buffer_sample_views(_p(d_feat), _p(d_mask), n, h, w, ch, S, C.c_uint64(seed), C.c_uint64(fid), base, *out.ptrs(), None))
    out.check(_expect(h, w, n, mask, feats, seed, fid, base))


def _store(maps, ch, order, gap=37, lead=0):
    """A store with the maps' rows placed in `order` and `gap` junk rows before, between and behind them (`lead` more in front), and a
    mask buffer laid out likewise with junk bytes of 1. maps = [(feats [hw,ch], mask [hw] or None)]. Returns (store, masks, rows, offsets)."""
    rows, offs = [0] * len(maps), [-1] * len(maps)
    parts, mparts, r, o = [np.full((gap + lead, ch), JUNK, np.int16)], [np.ones(gap, np.uint8)], gap + lead, gap
    for i in order:
        f, m = maps[i]
        rows[i] = r
        parts += [f, np.full((gap, ch), JUNK, np.int16)]
        r += len(f) + gap
        if m is not None:
            offs[i] = o
            mparts += [m, np.ones(gap, np.uint8)]
            o += len(m) + gap
    return np.concatenate(parts), np.concatenate(mparts), rows, offs


def _table_call(store, masks, table, max_hw, ch, S, seed, fid, base, out, n_rows=None, mask_bytes=None, skip_rows=0):
    """The table entry point on store[skip_rows:] (rows in the table count from there)."""
    d_store = torch.from_numpy(store).cuda()
    d_mask = torch.from_numpy(masks).cuda() if masks is not None else None
    d_table = torch.from_numpy(np.asarray(table, np.int64)).cuda()
    n_rows = len(store) - skip_rows if n_rows is None else n_rows
    mask_bytes = (len(masks) if masks is not None else 0) if mask_bytes is None else mask_bytes
    rc = N.lib().acez_buffer_sample_views_table(C.c_void_p(d_store.data_ptr() + skip_rows * ch * 2), n_rows, _p(d_mask), mask_bytes, _p(d_table),
                                                len(table), max_hw, ch, S, C.c_uint64(seed), C.c_uint64(fid), base, *out.ptrs(), None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("name", list(CASES))
def test_table_sampler_equals_the_oracle(name):
    """All views of the case in one launch, their maps out of order in a larger store with unrelated rows between them."""
    h, w, S, ch, n, mask, feats, seed, fid, base = _case(name)
    maps = [(feats[v], mask[v] if mask is not None else None) for v in range(n)]
    store, masks, rows, offs = _store(maps, ch, order=list(range(n))[::-1])
    out = Outputs(n, S, ch)
    rc = _table_call(store, masks if mask is not None else None, [(rows[v], h, w, offs[v]) for v in range(n)], h * w, ch, S, seed, fid, base, out)
    assert rc == 0
    out.check(_expect(h, w, n, mask, feats, seed, fid, base))


def _mixed_maps():
    """The production, one-over and single-last maps (and a second production one) at one channel count: (h, w, feats, mask)."""
    rng = np.random.default_rng(5)
    shapes = [(60, 80), (1, 257), (30, 40), (60, 80)]
    masks = [_density(rng, 1, 4800, 0.7)[0], _density(rng, 1, 257, 0.5)[0], _single(1, 1200, 1199)[0], None]
    return [(h, w, features(v, h * w, 512), masks[v]) for v, (h, w) in enumerate(shapes)]


def test_table_sampler_mixes_sizes_in_one_launch():
    views = _mixed_maps()
    S, ch, seed, fid, base = 1024, 512, 77, 500, 3
    store, masks, rows, offs = _store([(f, m) for _, _, f, m in views], ch, order=[2, 0, 3, 1])
    out = Outputs(len(views), S, ch)
    table = [(rows[v], h, w, offs[v]) for v, (h, w, _, _) in enumerate(views)]
    assert _table_call(store, masks, table, 4800, ch, S, seed, fid, base, out) == 0
    out.check([(m, f, w, seed, fid + v, base + v) for v, (h, w, f, m) in enumerate(views)])


@pytest.mark.parametrize("refusal", ["negative_row", "larger_than_max_hw", "past_the_store", "past_the_masks"])
def test_table_sampler_refuses_a_view_that_does_not_fit(refusal):
    """Return code 0, the refused view's rows keep their poison, every other view is exact. Nothing here would read outside an
    allocation even if the view were not refused: the store begins 64 rows into its allocation, and n_rows and mask_bytes are stated
    smaller than the buffers are."""
    rng = np.random.default_rng(9)
    S, ch, seed, fid, base = 96, 16, 2089, 40, 2
    shapes = [(30, 40), (30, 50), (30, 40), (20, 30)]
    maps = [(features(v, h * w, ch), _density(rng, 1, h * w, 0.5)[0]) for v, (h, w) in enumerate(shapes)]
    lead = 64
    store, masks, rows, offs = _store(maps, ch, order=[0, 2, 3, 1], lead=lead)   # view 1's map and mask are the last in their buffers
    rows = [r - lead for r in rows]
    table = [[rows[v], h, w, offs[v]] for v, (h, w) in enumerate(shapes)]
    max_hw, n_rows, mask_bytes, bad = 1500, None, None, 1
    if refusal == "negative_row":
        table[1][0] = -5
    elif refusal == "larger_than_max_hw":
        max_hw = 1200                                                    # view 1 has 1500 cells
    elif refusal == "past_the_store":
        n_rows = rows[1] + 1499                                          # one row short of view 1's map
    else:
        mask_bytes = offs[1] + 1499                                      # one byte short of view 1's mask
    out = Outputs(len(shapes), S, ch)
    assert _table_call(store, masks, table, max_hw, ch, S, seed, fid, base, out, n_rows=n_rows, mask_bytes=mask_bytes, skip_rows=lead) == 0
    out.check([None if v == bad else (maps[v][1], maps[v][0], w, seed, fid + v, base + v) for v, (h, w) in enumerate(shapes)])
