"""The summation order of acezero_amd/csrc/ordered_sum.h restated in numpy, once: the butterfly of a wavefront, the wavefronts of a
workgroup, the rows of many workgroups. tests/icp_restated.py, tests/track_restated.py, tests/simplify_restated.py and
tests/warp_restated.py build their sums on it. A helper module, not a test file."""
import numpy as np

WAVE = 64
LANES = np.arange(WAVE)


def _bits(a):
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def wave_sums(v):
    """[..., c] from [..., 64, c], in v's dtype: the xor butterfly 32, 16, .. 1 over the 64 lanes; lane 0's sums, which every lane
    holds bit for bit."""
    for s in (32, 16, 8, 4, 2, 1):
        v = v + v[..., LANES ^ s, :]
    assert all(np.array_equal(_bits(v[..., 0, :]), _bits(v[..., k, :])) for k in (1, 37, 63)), "a + b == b + a"
    return v[..., 0, :]


def block_sums(t, tile=256):
    """float64 [ceil(n / tile), c] from [n, c]: row i is lane i % 64 of wavefront (i / 64) % (tile / 64) of workgroup i / tile; per
    wavefront the butterfly, then the wavefronts in ascending order."""
    blocks = (len(t) + tile - 1) // tile
    v = np.zeros((blocks * tile, t.shape[1]))
    v[:len(t)] = t
    w = wave_sums(v.reshape(blocks, tile // WAVE, WAVE, t.shape[1]))
    out = w[:, 0]
    for k in range(1, tile // WAVE):
        out = out + w[:, k]
    return out


def totals(partials, tile=256):
    """float64 [c]: thread t adds rows t, t + tile, .. in ascending order from 0.0; then the threads' sums as a workgroup's."""
    v = np.zeros((tile, partials.shape[1]))
    for lo in range(0, len(partials), tile):
        part = partials[lo:lo + tile]
        v[:len(part)] = v[:len(part)] + part
    return block_sums(v, tile)[0]


def lane_strided_totals(partials, nblk, inv_scale=None, swap=None, extra=0):
    """head_opt.h tail_output in float32, bit for bit: lane j adds rows j, j + 64, .. of `partials` [>= nblk, k] in order from 0, then
    the xor butterfly 32 .. 1 (wave_sums, which keeps the dtype of its input), then x inv_grad_scale where one is given. swap = (a, b):
    those two rows exchanged; extra: rows past nblk included (the mutants of tests/test_loss_stage_cpu.py)."""
    p = np.asarray(partials, np.float32)[:nblk + extra].copy()
    if swap:
        p[[swap[0], swap[1]]] = p[[swap[1], swap[0]]]
    acc = np.zeros((WAVE, p.shape[1]), np.float32)
    for b in range(p.shape[0]):
        acc[b % WAVE] = acc[b % WAVE] + p[b]
    tot = wave_sums(acc)
    assert tot.dtype == np.float32
    return tot if inv_scale is None else tot * np.float32(inv_scale)
