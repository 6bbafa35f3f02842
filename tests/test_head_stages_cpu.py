"""CPU: the per-element checker of tests/head_stage_restated.py is proven before it judges a kernel (tests/test_head_stages_gpu.py).

A stand-in for the kernels is built from oracle-made operands (the oracle's rounded weights, the features, the oracle's d loss / d fc2
pre-activation) with numpy fp32 arithmetic in two accumulation orders that differ from each other and from the fp64 restatement: the
reduction dimension of every GEMM (K for the row GEMMs, the batch rows for the weight gradients) in 64-wide stages, or in 16-wide blocks
taken in reversed order. Its outputs are rounded to 16 bits. The stand-in must pass every check; seven deliberately wrong stand-ins must
each fail, with the failing elements counted in the message -- a mutation that passed would mean the bound is too loose for that defect."""
import functools
import re

import numpy as np
import pytest
import torch

from oracle import head_oracle
from tests import head_stage_restated as hs
from tests import helpers

CASES = [(dtype, regime, n) for dtype in ("bf16", "fp16") for regime in ("untrained", "trained") for n in (81, 129)]
ORDERS = ("stages64", "rev16")


def _gemm32(X, Wt, order):
    """X [m, K] @ Wt [K, N] in fp32, the reduction dimension in chunks that are summed in fp32 one after the other."""
    K = X.shape[1]
    step = 64 if order == "stages64" else 16
    chunks = [(k, min(K, k + step)) for k in range(0, K, step)]
    if order == "rev16":
        chunks.reverse()
    acc = np.zeros((X.shape[0], Wt.shape[1]), np.float32)
    for a, b in chunks:
        acc = acc + X[:, a:b] @ Wt[a:b]
    return acc


def _to16(fmt, x32, rounding):
    """fp32 array -> uint16 patterns: round to nearest even, or (mutation d) truncate toward zero."""
    bits = fmt.bits(torch.from_numpy(np.ascontiguousarray(x32, np.float32)))
    if rounding == "trunc":
        over = np.abs(fmt.values(bits).numpy()) > np.abs(x32.astype(np.float64))
        bits = np.where(over, bits - 1, bits).astype(np.uint16)      # sign-magnitude patterns: one step toward zero
    return bits


def _f32(fmt, bits):
    return fmt.values(bits).to(torch.float32).numpy()


@functools.lru_cache(maxsize=None)
def _operands(dtype, regime, n):
    """Oracle-made operands on whole 80-row tiles (the rows past n are what a larger batch would have left in the buffers)."""
    fmt = hs.Fmt(dtype)
    if regime == "trained":
        prob, flat0 = helpers.trained_problem()
    else:
        prob, flat0 = helpers.golden_problem()
    npad = (n + 79) // 80 * 80
    pool = np.random.default_rng(7).permutation(prob["features"].shape[0])[:4 * npad]
    cfg = helpers.full_cfg(helpers.HEAD_CONFIGS["head_tanh_1cyclepoly"], prob)
    cfg["global_batch"] = n
    orc = head_oracle.HeadOracle(flat0.clone(), prob["mean"], mode=dtype)
    s, tape = orc.forward(torch.from_numpy(prob["features"][pool]))
    ds = orc.loss_and_ds(s, helpers.torch_batch(prob, pool), cfg, 0)["ds"]
    # Every computation is row by row, so the batch is any npad rows of the pool. Under the tanh loss a row with a saturated error has no
    # gradient at all, and a mutation that drops or adds such a row changes nothing: the rows at the slab edges and the rows past n are
    # taken from those that do have one.
    live = (ds.abs().sum(1) > 0).numpy()
    rows = list(range(npad))
    spare = [r for r in range(npad, 4 * npad) if live[r]]
    for e in [63, 64, 127, 128, n - 1] + list(range(n, npad)):
        if e < npad and not live[rows[e]]:
            rows[e] = spare.pop()
    rows = torch.tensor(rows)
    feats, ds = torch.from_numpy(prob["features"][pool])[rows], ds[rows]
    f2 = tape["out"][orc.p.L - 1][rows]
    dz_last = fmt.bits(((ds @ orc.r(orc.p.W3)) * (f2 > 0) * orc.gs).float())     # stored scaled (fp16: by the oracle's first-step scale)
    L = orc.p.L
    w16 = np.stack([fmt.bits(orc.p.W[l].contiguous()) for l in range(L)])
    bias = np.stack([orc.p.b[l].numpy() for l in range(L)]).astype(np.float32)
    return fmt, fmt.bits(orc.r(feats)), w16, bias, dz_last, 1.0 / orc.gs


@functools.lru_cache(maxsize=None)
def _stand_in(dtype, regime, n, order, rounding="rne", residual_before_relu=False):
    """(Capture of n rows, padded dZ list) of the numpy fp32 stand-in."""
    fmt, r0, w16, bias, dz_last, inv = _operands(dtype, regime, n)
    nb = 1
    L, fwd, dgrad, ins = hs.structure(nb)
    W = [_f32(fmt, w16[l]) for l in range(L)]
    out, R, mask, dZ = {}, [r0] + [None] * (nb + 1), {}, [None] * L
    get = lambda s: _f32(fmt, R[s[1]] if s[0] == "R" else out[s[1]])
    for l, src, rb in fwd:
        acc = _gemm32(get(src), W[l].T.copy(), order) + bias[l]
        y = _to16(fmt, np.maximum(acc, 0), rounding)
        out[l] = y
        mask[l] = _f32(fmt, y) > 0
        if rb is not None:
            r = _f32(fmt, R[rb])
            R[rb + 1] = _to16(fmt, np.maximum(acc + r, 0) if residual_before_relu else _f32(fmt, y) + r, rounding)
    dZ[L - 1] = dz_last
    dR = None
    for l, lo_, adds, emits in dgrad:
        acc = _gemm32(_f32(fmt, dZ[l]), W[l], order)
        if adds:
            acc = acc + _f32(fmt, dR)
        y = _to16(fmt, acc, rounding)
        if emits:
            dR = y
        dZ[lo_] = np.where(mask[lo_], y, 0).astype(np.uint16)
    ns = hs.n_slabs(L)
    slabs = np.zeros((ns, L * hs.LAYER), np.float32)
    grad = np.zeros(L * hs.LAYER + 4 * 513 + 4, np.float32)
    partials = {}
    tiles = (n + 79) // 80
    for l in range(L):
        Z, X = _f32(fmt, dZ[l]), get(ins[l])
        for sl in range(ns):
            mb, me = hs.slab_rows(n, ns, sl)
            slabs[sl, l * hs.LAYER:l * hs.LAYER + 262144] = _gemm32(Z[mb:me].T.copy(), X[mb:me], order).reshape(-1)
        grad[l * hs.LAYER:l * hs.LAYER + 262144] = slabs[:, l * hs.LAYER:l * hs.LAYER + 262144].sum(0, dtype=np.float32) * np.float32(inv)
        rows = 80 if l < L - 1 else 32
        p = np.stack([Z[m0:min(n, m0 + rows)].sum(0, dtype=np.float32) for m0 in range(0, n, rows)])
        if l < L - 1:
            partials[l] = p
        grad[l * hs.LAYER + 262144:(l + 1) * hs.LAYER] = p.sum(0, dtype=np.float32) * np.float32(inv)
    kept = {l: a[:n] for l, a in out.items() if not hs.unkept(l, L)}
    cap = hs.Capture(fmt=fmt, nb=nb, n=n, nslabs=ns, inv_grad_scale=inv, w16=w16, bias=bias, out=kept, R=[a[:n] for a in R],
                     mask={l: m[:n] for l, m in mask.items() if l < L - 1}, dZ=[a[:n] for a in dZ], slabs=slabs, bias_partials=partials,
                     grad=grad)
    assert len(partials[0]) == tiles
    return cap, dZ


def _failed(results):
    return {(r.stage, r.layer) for r in results if r.bad}


def _must_fail(results, expected, exactly=True):
    """assert_clean raises, its message counts the failing elements and names every expected stage; `exactly`: and no other stage fails."""
    with pytest.raises(AssertionError) as e:
        hs.assert_clean(results, "mutation")
    msg = str(e.value)
    assert re.search(r"mutation: [1-9]\d* elements outside their bounds in [1-9]\d* stages", msg), msg
    for stage, layer in expected:
        assert re.search(r"%s\[%s\]: [1-9]\d* of \d+ elements outside" % (re.escape(stage), layer), msg), (stage, layer, msg)
    if exactly:
        assert _failed(results) == set(expected), (_failed(results), expected)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dtype,regime,n", CASES)
def test_stand_in_passes_every_check(dtype, regime, n, order):
    cap, _ = _stand_in(dtype, regime, n, order)
    results = hs.check_all(cap)
    L = 8
    # every element of every checked buffer is judged: out of 6 kept layers, R[1..2], 7 masks, 7 dZ, 2 slabs + grad (twice) per layer, partials, biases
    assert len(results) == 6 + 2 + 7 + 7 + 4 * L + 7 + L
    hs.assert_clean(results, (dtype, regime, n, order))
    hs.assert_left_out_capped(results, (dtype, regime, n, order))      # (the oracle's data stays inside the cap, layer by layer)
    assert all(r.left_out == 0 for r in results if not (r.stage == "mask" and hs.unkept(r.layer, L)))
    # the two orders are different kernels as far as the checker can tell: they differ in stored bits
    other, _ = _stand_in(dtype, regime, n, ORDERS[1 - ORDERS.index(order)])
    assert not np.array_equal(cap.slabs, other.slabs)
    assert any(not np.array_equal(a, b) for a, b in zip(cap.dZ, other.dZ))


def _order_of(dtype, regime, n):
    return ORDERS[CASES.index((dtype, regime, n)) % 2]


@pytest.mark.parametrize("dtype,regime,n", CASES)
def test_a_row_dropped_or_doubled_at_the_slab_edge_fails(dtype, regime, n):
    """a: the last row of slab 0 is dropped; b: the first row of slab 1 is also summed into slab 0."""
    base, _ = _stand_in(dtype, regime, n, _order_of(dtype, regime, n))
    L, _, _, ins = hs.structure(1)
    fmt = base.fmt
    mb1, _ = hs.slab_rows(n, 2, 1)
    for row, sign in ((mb1 - 1, -1.0), (mb1, 1.0)):
        cap = base.copy()
        for l in range(L):
            Z, X = _f32(fmt, cap.dZ[l]), fmt.values(base.R[ins[l][1]] if ins[l][0] == "R" else base.out[ins[l][1]]).to(torch.float32).numpy()
            w = slice(l * hs.LAYER, l * hs.LAYER + 262144)
            cap.slabs[0, w] += np.float32(sign) * np.outer(Z[row], X[row]).reshape(-1)
            cap.grad[w] = (cap.slabs[0, w] + cap.slabs[1, w]) * np.float32(cap.inv_grad_scale)
        results = hs.check_wgrad(cap)
        _must_fail(results, [(s, l) for s in ("slab0", "grad_w") for l in range(L)])


@pytest.mark.parametrize("dtype,regime,n", CASES)
def test_two_k_chunks_swapped_in_one_column_tile_fail(dtype, regime, n):
    """c: one 128-column tile of one forward layer / of one input-gradient layer multiplies two 8-wide K chunks of its input with each
    other's weights."""
    order = _order_of(dtype, regime, n)
    base, _ = _stand_in(dtype, regime, n, order)
    fmt = base.fmt
    perm = np.arange(512)
    perm[136:144], perm[168:176] = np.arange(168, 176), np.arange(136, 144)
    cols = slice(256, 384)
    # forward layer 1: out[1] = relu(out[0] @ W[1]^T + b[1])
    cap = base.copy()
    x = _f32(fmt, base.out[0])[:, perm]
    acc = _gemm32(x, _f32(fmt, base.w16[1]).T.copy(), order) + base.bias[1]
    cap.out[1][:, cols] = _to16(fmt, np.maximum(acc, 0), "rne")[:, cols]
    # (only the buffer is patched: its mask bits need no longer be its sign, and the layer that reads it no longer matches it either)
    _must_fail(hs.check_forward(cap), [("out", 1)], exactly=False)
    assert _failed(hs.check_forward(cap)) <= {("out", 1), ("mask", 1), ("R", 1), ("mask", 2)}
    # input-gradient layer: dZ[3] = mask[3] * round(dZ[4] @ W[4])
    cap = base.copy()
    z = _f32(fmt, base.dZ[4])[:, perm]
    y = _to16(fmt, _gemm32(z, _f32(fmt, base.w16[4]), order), "rne")
    cap.dZ[3][:, cols] = np.where(base.mask[3], y, 0).astype(np.uint16)[:, cols]
    _must_fail(hs.check_dgrad(cap), [("dZ", 3)], exactly=False)
    assert _failed(hs.check_dgrad(cap)) <= {("dZ", 3), ("dZ", 2)}       # (dZ[2] is computed from the patched buffer)


@pytest.mark.parametrize("dtype,regime,n", CASES)
def test_truncated_outputs_fail(dtype, regime, n):
    """d: every 16-bit output truncated toward zero instead of rounded to nearest even."""
    cap, _ = _stand_in(dtype, regime, n, _order_of(dtype, regime, n), rounding="trunc")
    L = 8
    _must_fail(hs.check_forward(cap), [("out", l) for l in range(L) if not hs.unkept(l, L)] + [("R", 1), ("R", 2)], exactly=False)
    # (the trained problem's fc2 passes seven channels on through unit weights: dZ[6] is a copy of 16-bit values, which truncation leaves alone)
    _must_fail(hs.check_dgrad(cap), [("dZ", l) for l in range(L - 1 if regime == "untrained" else L - 2)])


@pytest.mark.parametrize("dtype,regime,n", CASES)
def test_bias_sum_over_the_rows_past_the_end_of_a_ragged_tile_fails(dtype, regime, n):
    """e: the last tile's column sums run over 80 rows instead of n - m0 (the rows past n hold what a larger batch left there)."""
    base, padded = _stand_in(dtype, regime, n, _order_of(dtype, regime, n))
    cap = base.copy()
    last = (n - 1) // 80
    layers = range(7)
    for l in layers:
        assert np.any(padded[l][n:] != 0)
        cap.bias_partials[l][last] = _f32(base.fmt, padded[l])[80 * last:80 * last + 80].sum(0, dtype=np.float32)
    _must_fail(hs.check_bias(cap), [("bias_partials", l) for l in layers])


@pytest.mark.parametrize("dtype,regime,n", CASES)
def test_one_flipped_mask_bit_of_an_unkept_layer_fails(dtype, regime, n):
    """f: one bit of a layer whose activation is not kept, where |v| > 10 s."""
    base, _ = _stand_in(dtype, regime, n, _order_of(dtype, regime, n))
    for l, src in ((2, ("out", 1)), (5, ("out", 4))):
        v, s = hs.forward_value(base, l, src)
        for sign in (1.0, -1.0):
            sel = torch.nonzero(sign * v > 10 * s)
            assert len(sel)
            r, c = (int(x) for x in sel[len(sel) // 2])
            cap = base.copy()
            cap.mask[l][r, c] ^= True
            results = hs.check_forward(cap)
            _must_fail(results, [("mask", l)])
            assert [x.bad for x in results if (x.stage, x.layer) == ("mask", l)] == [1]


@pytest.mark.parametrize("dtype,regime,n", CASES)
def test_residual_added_before_the_relu_fails(dtype, regime, n):
    """g: R[b + 1] = round(relu(u + R[b])) instead of round(round(relu(u)) + R[b])."""
    cap, _ = _stand_in(dtype, regime, n, _order_of(dtype, regime, n), residual_before_relu=True)
    _must_fail(hs.check_forward(cap), [("R", 1)], exactly=False)
    assert ("R", 2) in _failed(hs.check_forward(cap))


def test_slab_rows_are_the_kernels():
    """rows_per_slab is rounded up to whole 64-row stages: 64 rows leave slab 1 empty, 65 give it one row."""
    assert [hs.slab_rows(n, 2, 1) for n in (1, 64, 65, 128, 129, 637)] == [(64, 64), (64, 64), (64, 65), (64, 128), (128, 129), (320, 637)]
    assert hs.slab_rows(357, 1, 0) == (0, 357) and hs.n_slabs(8) == 2 and hs.n_slabs(11) == 1


def test_mask_layout_decodes_what_the_epilogue_packs():
    """decode_mask_bits against a plain restatement of the packing loop of rowgemm80_body (fragment f = 2 j + i ends at bits 9 - f / 25 - f)."""
    rng = np.random.default_rng(1)
    n = 97
    bits = rng.uniform(size=(160, 512)) < 0.5
    words = np.zeros((2, 4, 4, 64, 2), np.uint32)
    for mt in range(2):
        for nt in range(4):
            for w in range(4):
                for lane in range(64):
                    fr, fq = lane & 15, lane >> 4
                    x = y = 0
                    for j in range(5):
                        for i in range(2):
                            r, c = mt * 80 + j * 16 + fr, nt * 128 + w * 32 + i * 16 + 4 * fq
                            x = (x << 1) | int(bits[r, c]) | (int(bits[r, c + 1]) << 16)
                            y = (y << 1) | int(bits[r, c + 2]) | (int(bits[r, c + 3]) << 16)
                    words[mt, nt, w, lane] = (x, y)
    assert np.array_equal(hs.decode_mask_bits(words.reshape(2, 2048), n), bits[:n])
