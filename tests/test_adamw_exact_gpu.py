"""GPU: the optimiser launches of the head's training step against tests/adamw_restated.py, bit for bit.

Every step here is the split flow a data-parallel host drives: tr.backward(idx) on 16 rows (it arms the schedule and produces the
statistics), a write into the caller-owned tr.grad, then tr.update(). Given the gradient, the optimiser stage is elementwise float32
arithmetic without contraction, with correctly rounded divide and square root: the restatement (itself pinned to torch.optim.AdamW in
tests/test_adamw_restated_cpu.py) must be met exactly -- params, adam_m, adam_v, the pose parameters and their moments, and the
16-bit recasts W, W^T, W3. The other flows (the fused step, wgrad_opt_kernel, update_next, update_layers, the group step, the fused pose
launches) are pinned to this one bit for bit by their own tests, so the exact pin carries over to them.

Sensitivity, tried once on scratch builds of the library with one line changed each (MI355X; every other test of this file passed):
  eps moved inside the square root        -> one_step (1.95 M elements of p), free_running (step 1), fp16_overflow_flag (its ordinary steps)
  bc2_sqrt taken from the previous step   -> free_running (step 2), fp16_overflow_flag (the step after the skipped one)
  decay applied after the step            -> one_step (138 k elements of p, one ulp each), free_running, fp16_overflow_flag
  m store dropped, small-parameter path   -> one_step, ties, free_running, fp16_overflow_flag (m of the 6148 biases and fc3 elements)
  W^T store with row and column swapped   -> 16_bit_copies (the gradient on the optimiser's copies), the backward comparison of the pose tests
  W3 copy not rewritten                   -> 16_bit_copies, the backward comparison of the pose tests
  pose gate it >= wait                    -> pose_parameters (all four cases, at it = 2)
  pose network's transposed copies not refreshed by the optimiser launch -> pose_parameters[mlp] (the backward comparison)"""
import functools

import numpy as np
import pytest
import torch

from tests import adamw_restated as R
from tests import helpers
from tests.test_head_gpu import _trainer

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "fp16"]
N_ROWS = 16
LAYOUT = R.flat_layout(1, 4)
B1, B2 = R.CFG["beta1"], R.CFG["beta2"]


@functools.lru_cache(maxsize=None)
def _problem():
    prob, flat0 = helpers.golden_problem()
    idx = torch.from_numpy(helpers.golden_batches(prob, 1)[0][:N_ROWS].astype(np.int64))
    return prob, flat0, idx


def _mk(dtype, base="head_tanh_1cyclepoly", **over):
    prob, flat0, idx = _problem()
    cfg = helpers.full_cfg(helpers.HEAD_CONFIGS[base], prob)
    cfg.update(over)
    tr = _trainer(prob, flat0, cfg, dtype=dtype)
    assert tr.n_params == R.num_params(1, 4)
    return tr, idx.cuda()


def _np(t):
    return t.detach().cpu().numpy().copy()


def _put(t, a):
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(t.dtype))


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_u32(a), _u32(b))


def _pows(steps):
    b1p = b2p = 1.0
    for _ in range(steps):      # the running products of sched_post_wave, not pow
        b1p *= B1
        b2p *= B2
    return b1p, b2p


def _head_state(tr):
    return _np(tr.params), _np(tr.adam_m), _np(tr.adam_v)


def _assert_bitwise(what, gpu, ref, mask=None, layout=LAYOUT, ref64=None):
    ne = _u32(gpu) != _u32(ref)
    if mask is not None:
        ne &= mask
    if ne.any():
        i = int(np.flatnonzero(ne)[0])
        ulps = int(_u32(gpu)[i].astype(np.int64) - _u32(ref)[i].astype(np.int64))
        more = "" if ref64 is None else f", float64 {ref64[i]!r}"
        where = R.locate(layout, i) if layout is not None else f"element {i}"
        raise AssertionError(f"{what}: {int(ne.sum())} elements differ; first at {where}: kernel {gpu[i]!r}, restated {ref[i]!r} "
                             f"({ulps:+d} in the float32 bit pattern{more})")


def _assert_bound(what, gpu, ref64, bound, layout=LAYOUT):
    ok = R.within(gpu, ref64, bound)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        where = R.locate(layout, i) if layout is not None else f"element {i}"
        raise AssertionError(f"{what}: {int((~ok).sum())} elements beyond the rounding bound; first at {where}: kernel {gpu[i]!r}, float64 "
                             f"{ref64[i]!r}, bound {bound[i]:.3e}")


def _check_step(what, before, g, after, s, layout=LAYOUT):
    """The kernels' (p, m, v) `after` against the restatement of one step from `before` with gradient g and scalars s: bitwise wherever
    v is not subnormal before or after, within the derived bound against float64 everywhere. Returns the number of subnormal-class
    elements that differ bitwise."""
    p32, m32, v32 = R.step32(before[0], g, before[1], before[2], s)
    p64, m64, v64 = R.step64(before[0], g, before[1], before[2], s)
    bp, bm, bv = R.bounds(before[0], g, before[1], before[2], s)
    sub = R.is_subnormal(before[2]) | R.is_subnormal(v32)
    for name, x, r32, r64, b in (("m", after[1], m32, m64, bm), ("v", after[2], v32, v64, bv), ("p", after[0], p32, p64, bp)):
        _assert_bitwise(f"{what}: {name}", x, r32, ~sub, layout, r64)
        _assert_bound(f"{what}: {name}", x, r64, b, layout)
    diff = (_u32(after[0]) != _u32(p32)) | (_u32(after[1]) != _u32(m32)) | (_u32(after[2]) != _u32(v32))
    return int((diff & sub).sum()), int(sub.sum()), (p32, m32, v32)


def _overflow_flag(tr):
    return float(tr.grad[tr.n_params + 3]) >= 1024.0     # fp16: this step's own gradient chain stored an infinity (the head's update is skipped)


def _export16(tr):
    dst = tr.new_weights16_buffer()
    tr.export_weights16(0, tr.L, dst)
    return dst.cpu().numpy().view(np.uint16).reshape(tr.L, 512, 512)


def _rne(dtype):
    return R.rne_fp16 if dtype == "fp16" else R.rne_bf16


def _assert_copies_are_rne_of(tr, dtype, masters):
    w16 = _export16(tr)
    for l in range(tr.L):
        name, o, shape = LAYOUT[2 * l]
        want = _rne(dtype)(masters[o:o + 262144]).reshape(512, 512)
        ne = w16[l] != want
        if ne.any():
            r, c = (int(x[0]) for x in np.nonzero(ne))
            raise AssertionError(f"16-bit W of layer {l} {name}: {int(ne.sum())} elements are not the rounding of their master; first at row {r}, "
                                 f"column {c}: copy {w16[l][r, c]:#06x}, master {masters[o + r * 512 + c]!r} rounds to {want[r, c]:#06x}")
    return w16


def _backward_record(tr, idx):
    tr.backward(idx)
    torch.cuda.synchronize()
    return _np(tr.grad), tr.last_scene_coords(N_ROWS)


# ------------------------------------------------------------------------------------------------ a + b: one step, every element
@functools.lru_cache(maxsize=None)
def _one_step(dtype):
    tr, idx = _mk(dtype)
    n = tr.n_params
    npad = tr._state.numel() // 3
    pos = R.planted_positions(LAYOUT)
    p, g, m, v = R.random_state(n, seed=11, p_scale=1e-3)
    p += _problem()[1].numpy()             # around the initial weights: test_16_bit_copies_after_the_step runs a forward on the updated masters
    cls = R.plant(p, g, m, v, pos)
    tr.backward(idx)
    _put(tr.params, p); _put(tr.adam_m, m); _put(tr.adam_v, v)
    for i in range(3):
        tr._state[i * npad + n:(i + 1) * npad] = 7.25 + i        # the padding up to the 1024-float boundary
    tr.sync_weights()
    _put(tr.grad[:n], g)
    st = tr.state()
    assert not _overflow_flag(tr) and st["opt_steps"] == 0 and st["iteration"] == 0
    tr.update()
    st2 = tr.state()
    assert st2["opt_steps"] == 1 and st2["iteration"] == 1 and not st2["nan"]
    return dict(tr=tr, idx=idx, before=(p, m, v), g=g, after=_head_state(tr), lr=st["lr"], pos=pos, cls=cls, pad=_np(tr._state), npad=npad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_step_from_a_chosen_state_every_element(dtype):
    """params, adam_m, adam_v, the gradient from a seeded generator, with the edge classes of adamw_restated.CLASSES planted at the first and
    last element of every weight and bias, on both sides of every 64 x 64 tile edge of one layer, and at 2048 seeded positions: bitwise
    equal to step32 on every element whose v is not subnormal, within the rounding bound of float64 on all of them; nothing outside
    [0, n_params) of the three vectors is written. Measured (MI355X, both formats): 292 elements in the subnormal class, none of them
    differs bitwise -- the kernels do not flush float32 subnormals."""
    r = _one_step(dtype)
    s = R.scalars(r["lr"], 1.0, 1.0)
    n_diff, n_sub, _ = _check_step("one step", r["before"], r["g"], r["after"], s)
    print(f"[{dtype}] subnormal-class elements: {n_sub}, of which {n_diff} differ bitwise from the restatement "
          "(non-zero: the kernel flushes subnormals)")
    at = lambda c: r["pos"][r["cls"] == c]
    P, M, V = r["after"]
    assert np.isinf(V[at(4)]).all() and n_sub >= len(at(3)) > 0
    assert _same_bits(P[at(4)], r["before"][0][at(4)] * s.decay) and _same_bits(P[at(7)], r["before"][0][at(7)] * s.decay)
    n, npad = len(P), r["npad"]
    for i in range(3):
        assert (r["pad"][i * npad + n:(i + 1) * npad] == 7.25 + i).all(), "the optimiser wrote into the padding behind vector %d" % i


@pytest.mark.parametrize("dtype", DTYPES)
def test_16_bit_copies_after_the_step(dtype):
    """W: the exported copies are the round-to-nearest-even of the kernel's own new masters, every layer, every element. W^T and W3
    have no export and are pinned by behaviour: a backward on the copies the optimiser left equals, bit for bit, a backward after
    sync_weights() has recast all three from the masters (a stale or misplaced W^T element shows in the propagated gradient, a stale W3
    element in the coordinates). That this comparison can fail is shown in place: one master moved by one 16-bit ulp WITHOUT a recast
    leaves a stale copy, and the same two backwards then differ."""
    r = _one_step(dtype)
    tr, idx = r["tr"], r["idx"]
    P = r["after"][0]
    assert _same_bits(_np(tr.params), P)
    _assert_copies_are_rne_of(tr, dtype, P)
    g1, x1 = _backward_record(tr, idx)
    tr.sync_weights()
    g2, x2 = _backward_record(tr, idx)
    assert np.isfinite(g1).all() and np.abs(g1[:tr.n_params]).sum() > 0 and g1[tr.n_params + 3] == 0
    _assert_bitwise("gradient on the optimiser's copies vs after a recast", g1[:tr.n_params], g2[:tr.n_params])
    assert _same_bits(g1, g2) and _same_bits(x1, x2)
    # the check can fail: a stale fc3 copy. The column with the largest fc2 activation in row 0, so that the product is not zero.
    act = torch.from_numpy(tr.debug_read("out", tr.L - 1, N_ROWS).view(np.int16)).view(tr.feature_dtype).float().numpy()
    c = int(np.abs(act[0]).argmax())
    assert act[0, c] != 0
    i = LAYOUT[-2][1] + c
    w = P[i:i + 1]
    up = _rne(dtype)(w) + np.uint16(1)                                   # the next 16-bit value away from zero
    w_up = up.view(np.float16).astype(np.float32) if dtype == "fp16" else (up.astype(np.uint32) << 16).view(np.float32)
    assert np.isfinite(w_up).all() and w_up[0] != w[0]
    tr.params[i] = float(w_up[0])
    g3, x3 = _backward_record(tr, idx)
    assert _same_bits(x3, x2), "a backward reads the 16-bit copies, not the masters"
    tr.sync_weights()
    g4, x4 = _backward_record(tr, idx)
    assert not _same_bits(x3, x4), "a stale W3 element went unnoticed"


def _tie_values(count, seed):
    """float32 values of weight-like magnitude that sit exactly between two bf16 / fp16 neighbours (above an even and above an odd
    kept mantissa), one float32 unit to either side, with all-ones mantissas that round up into the next binade, in the fp16
    subnormal range, both signs."""
    rng = np.random.default_rng(seed)
    k = np.arange(count)
    e = rng.integers(118, 125, count).astype(np.uint32)            # 2^-9 .. 2^-3
    hi7 = rng.integers(0, 128, count).astype(np.uint32)
    m10 = rng.integers(0, 1024, count).astype(np.uint32)
    kinds = [(hi7 & ~np.uint32(1)) << 16 | 0x8000, (hi7 | 1) << 16 | 0x8000, hi7 << 16 | 0x7fff, hi7 << 16 | 0x8001,
             (m10 & ~np.uint32(1)) << 13 | 0x1000, (m10 | 1) << 13 | 0x1000, m10 << 13 | 0x0fff, m10 << 13 | 0x1001,
             np.full(count, 0x7fffff, np.uint32), np.full(count, 0x7f8000, np.uint32), np.full(count, 0x7ff000, np.uint32)]
    mant = np.choose(k % len(kinds), kinds).astype(np.uint32)
    x = ((e << 23) | mant).view(np.float32)
    sub = ((2 * rng.integers(0, 1024, count) + 1) * 2.0 ** -25).astype(np.float32)      # exact ties between fp16 subnormals
    x = np.where(k % (len(kinds) + 1) == len(kinds), sub, x)
    return np.where((k // 2) % 2 == 0, x, -x).astype(np.float32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_are_recast_to_even_at_learning_rate_zero(dtype):
    """schedule='constant', lr_min=0: the kernel computes p * 1 - 0 * (m / denom) = p exactly and still recasts. Masters that are exact
    16-bit ties stay bitwise unchanged and their copies are the round-to-nearest-EVEN of them (the moments still advance: step32)."""
    tr, idx = _mk(dtype, schedule="constant", lr_min=0.0)
    n = tr.n_params
    pos = R.planted_positions(LAYOUT, extra=20000, seed=3)
    p, g, m, v = R.random_state(n, seed=12)
    v = np.maximum(v, np.float32(1e-20))
    p[pos] = _tie_values(len(pos), seed=4)
    tr.backward(idx)
    _put(tr.params, p); _put(tr.adam_m, m); _put(tr.adam_v, v)
    _put(tr.grad[:n], g)
    st = tr.state()
    assert st["lr"] == 0.0 and not _overflow_flag(tr)
    tr.update()
    assert tr.state()["opt_steps"] == 1
    P, M, V = _head_state(tr)
    _assert_bitwise("masters at lr = 0", P, p)
    p32, m32, v32 = R.step32(p, g, m, v, R.scalars(0.0, 1.0, 1.0))
    _assert_bitwise("m at lr = 0", M, m32)
    _assert_bitwise("v at lr = 0", V, v32)
    w16 = _assert_copies_are_rne_of(tr, dtype, p)
    # (the planted ties did land in weights, and were resolved in both directions)
    o = LAYOUT[2][1]
    sel = pos[(pos >= o) & (pos < o + 262144)] - o
    back = w16[1].reshape(-1)[sel]
    back = back.view(np.float16).astype(np.float32) if dtype == "fp16" else (back.astype(np.uint32) << 16).view(np.float32)
    assert (np.abs(back) > np.abs(p[o + sel])).any() and (np.abs(back) < np.abs(p[o + sel])).any()


# ------------------------------------------------------------------------------------------------ c: a free-running sequence
@pytest.mark.parametrize("dtype", DTYPES)
def test_free_running_sequence_matches_bitwise(dtype):
    """120 steps of a 1cyclepoly schedule whose learning rate changes at every step (60 of warm-up, 60 of cool-down), host-made
    gradients in the normal range. The restatement carries its own p, m, v and its own running products of beta from step 0 and never
    reads them back; only lr and the step count come from state(). All three vectors bitwise at steps 1, 2, 3, 10, 50, 120: the bias
    corrections (1 - beta2^t grows from 1e-3 to 0.11) and the step count."""
    steps = 120
    tr, idx = _mk(dtype, schedule="1cyclepoly", iterations=steps, warmup_iterations=60, cooldown_iterations=60, cooldown_trigger_percent=2.0,
                  lr_min=1e-4, lr_max=6e-4, warmup_lr=1e-4)
    n = tr.n_params
    rng = np.random.default_rng(21)
    mag = (10.0 ** rng.uniform(-6, 2, n)).astype(np.float32)
    z = rng.standard_normal(n + 997 * steps, dtype=np.float32)
    z[z == 0] = 1.0
    p, m, v = _head_state(tr)
    assert not v.any() and not m.any()
    b1p = b2p = 1.0
    applied, lrs = 0, []
    for k in range(steps):
        tr.backward(idx)
        g = z[997 * k:997 * k + n] * mag
        _put(tr.grad[:n], g)
        st = tr.state()
        assert st["iteration"] == k and st["opt_steps"] == applied, (k, st)
        lrs.append(st["lr"])
        skipped = _overflow_flag(tr)
        tr.update()
        if not skipped:
            p, m, v = R.step32(p, g, m, v, R.scalars(st["lr"], b1p, b2p))
            b1p *= B1; b2p *= B2
            applied += 1
        if k + 1 in (1, 2, 3, 10, 50, 120):
            assert not R.is_subnormal(v).any() and not R.is_subnormal(m).any()
            P, M, V = _head_state(tr)
            _assert_bitwise(f"step {k + 1}: m", M, m)
            _assert_bitwise(f"step {k + 1}: v", V, v)
            _assert_bitwise(f"step {k + 1}: p", P, p)
    st = tr.state()
    assert st["iteration"] == steps and st["opt_steps"] == applied and applied >= steps - 4
    assert all(a != b for a, b in zip(lrs, lrs[1:])), "the learning rate was meant to change at every step"
    _assert_copies_are_rne_of(tr, dtype, p)


# ------------------------------------------------------------------------------------------------ d: pose parameters
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["mlp", "naive"])
def test_pose_parameters_gate_and_step_bitwise(kind, dtype):
    """adamw_split_pose_kernel / adamw_small_one with pose_refinement_wait = 2: while it <= wait the pose vectors are untouched and
    the head's step count advances; from it = 3 they equal step32 with the pose optimiser's own scalars (its step count starts at 1,
    lr = pose_refinement_lr = 1e-3). Afterwards the transposed copies of the network's four 128 x 128 layers that the kernel keeps are
    pinned by behaviour (a backward on them equals a backward after sync_weights() has rebuilt them) and the refined poses equal those of
    a fresh trainer loaded with the same pose parameters (current_poses() rebuilds the transposed copies before it uses them, so it is
    the backward comparison that notices a copy the optimiser's launch left stale)."""
    over = dict(pose_refinement=kind, pose_refinement_wait=2)
    tr, idx = _mk(dtype, base="head_tanh_posemlp", **over)
    n, npose = tr.n_params, tr.n_pose
    rng = np.random.default_rng(31)
    pos = np.unique(np.concatenate([[0, npose - 1], rng.permutation(npose)[:min(npose, 2048)]]))
    pos = pos[rng.permutation(len(pos))]
    cls = np.arange(len(pos)) % len(R.CLASSES)
    pp, pm, pv = _np(tr.pose_params), _np(tr.pose_m), _np(tr.pose_v)
    initial = (pp.copy(), pm.copy(), pv.copy())
    b1p = b2p = 1.0
    head_steps = 0
    n_sub_diff = 0
    for it in range(6):
        tr.backward(idx)
        g = (rng.standard_normal(npose) * 10.0 ** rng.uniform(-6, 0, npose)).astype(np.float32)
        keep = g[pos[cls == 1]].copy()
        R.plant(None, g, None, None, pos)
        g[pos[cls == 5]] = -pm[pos[cls == 5]]
        if it % 2 == 1:
            g[pos[cls == 1]] = keep               # (g = 0 with m != 0 needs a step with g != 0 before it: steps 3 and 5 move m, step 4 has g = 0)
        _put(tr.grad[n + 4:], g)
        st = tr.state()
        assert st["iteration"] == it and st["opt_steps"] == head_steps
        head_steps += 0 if _overflow_flag(tr) else 1
        tr.update()
        st2 = tr.state()
        assert st2["iteration"] == it + 1 and st2["opt_steps"] == head_steps       # the head's step count advances during the wait
        got = (_np(tr.pose_params), _np(tr.pose_m), _np(tr.pose_v))
        if it <= 2:
            for name, x, x0 in zip(("pose_params", "pose_m", "pose_v"), got, initial):
                _assert_bitwise(f"it {it} <= wait: {name}", x, x0, layout=None)
        else:
            s = R.scalars(1e-3, b1p, b2p)
            d, _, (pp, pm, pv) = _check_step(f"pose step at it {it}", (pp, pm, pv), g, got, s, layout=None)
            n_sub_diff += d
            b1p *= B1; b2p *= B2
    assert head_steps >= 5
    assert np.isinf(pv[pos[cls == 4]]).all() and (pm[pos[cls == 1]] != 0).all()
    print(f"[{kind}, {dtype}] subnormal-class pose elements that differ bitwise: {n_sub_diff}")
    ga, xa = _backward_record(tr, idx)            # on the transposed copies the optimiser's launch kept
    tr.sync_weights()
    gb, xb = _backward_record(tr, idx)            # ... and on rebuilt ones
    assert np.isfinite(ga[n + 4:]).all() and np.abs(ga[n + 4:]).sum() > 0
    assert _same_bits(ga, gb) and _same_bits(xa, xb)
    fresh, _ = _mk(dtype, base="head_tanh_posemlp", **over)
    fresh.pose_params.copy_(tr.pose_params)
    fresh.sync_weights()
    assert _same_bits(tr.current_poses(), fresh.current_poses())


# ------------------------------------------------------------------------------------------------ e: calibration scalar
@pytest.mark.parametrize("dtype", DTYPES)
def test_calibration_scalar_follows_calib_step(dtype):
    """refine_calibration: the scalar's own AdamW in the schedule wave, 20 steps with chosen gradients in statistics slot 2 (zeros, sign
    changes, 1e6): state()['focal_scale'] against 1 + calib_step(...) within 2^-23, one float32 ulp at 1."""
    tr, idx = _mk(dtype, base="head_tanh_calib", iterations=40)
    n = tr.n_params
    gs = [0.0, 0.0, 1.0, -1.0, 3e-4, 2.5, -2.5, 0.0, 1e6, -1e6, 0.0, 7.0, -1e-3, 1e-3, 40.0, 40.0, 40.0, -0.5, 0.0, 1e-6]
    p = m = v = 0.0
    worst = 0.0
    for k, g in enumerate(gs):
        tr.backward(idx)
        tr.grad[n + 2] = g
        g32 = float(tr.grad[n + 2])
        tr.update()
        st = tr.state()
        assert st["iteration"] == k + 1
        p, m, v = R.calib_step(p, m, v, g32, k + 1, lr=1e-3)
        worst = max(worst, abs(st["focal_scale"] - (1.0 + p)))
        assert abs(st["focal_scale"] - (1.0 + p)) <= 2.0 ** -23, (k, st["focal_scale"], 1.0 + p)
    assert abs(p) > 1e-3
    print(f"[{dtype}] focal_scale vs 1 + calib_step over {len(gs)} steps: worst difference {worst:.3e}")


# ------------------------------------------------------------------------------------------------ f: a skipped step changes nothing
def _snapshot(tr):
    return _head_state(tr) + (_export16(tr).copy(),)


def _assert_unchanged(what, tr, snap):
    now = _snapshot(tr)
    for name, a, b in zip(("params", "adam_m", "adam_v"), now, snap):
        _assert_bitwise(f"{what}: {name}", a, b)
    assert np.array_equal(now[3], snap[3]), f"{what}: the 16-bit copies changed"


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_loss_skips_the_step_and_ends_the_schedule(dtype):
    tr, idx = _mk(dtype)
    n = tr.n_params
    p, g, m, v = R.random_state(n, seed=41)
    tr.backward(idx)
    _put(tr.params, p); _put(tr.adam_m, m); _put(tr.adam_v, v)
    tr.sync_weights()
    snap = _snapshot(tr)
    _put(tr.grad[:n], g)
    tr.grad[n] = float("nan")
    tr.update()
    st = tr.state()
    assert st["nan"]
    _assert_unchanged("NaN loss", tr, snap)
    tr.backward(idx)
    _put(tr.grad[:n], g)
    tr.update()
    assert tr.state()["nan"]
    _assert_unchanged("the step after a NaN loss", tr, snap)


def test_fp16_overflow_flag_skips_the_head_step_only():
    """Statistics slot 3 = 1024 (the all-reduced overflow flag of some rank): the head vectors and copies are untouched, AdamW's step
    count stays while the iteration advances, and the next ordinary step uses the UN-advanced bias corrections."""
    tr, idx = _mk("fp16")
    n = tr.n_params
    p, g, m, v = R.random_state(n, seed=42)
    b1p = b2p = 1.0
    tr.backward(idx)
    _put(tr.params, p); _put(tr.adam_m, m); _put(tr.adam_v, v)
    tr.sync_weights()
    for k, flag in enumerate((False, True, False)):
        if k:
            tr.backward(idx)
        assert not _overflow_flag(tr)
        _put(tr.grad[:n], g)
        if flag:
            tr.grad[n + 3] = 1024.0
            snap = _snapshot(tr)
        st = tr.state()
        tr.update()
        st2 = tr.state()
        assert st2["iteration"] == k + 1
        if flag:
            assert st2["opt_steps"] == st["opt_steps"] == 1
            _assert_unchanged("overflow flag", tr, snap)
        else:
            assert st2["opt_steps"] == st["opt_steps"] + 1
            p, m, v = R.step32(p, g, m, v, R.scalars(st["lr"], b1p, b2p))
            b1p *= B1; b2p *= B2
            P, M, V = _head_state(tr)
            for name, a, b in (("m", M, m), ("v", V, v), ("p", P, p)):
                _assert_bitwise(f"ordinary step {k}: {name}", a, b)
        g = -0.5 * g
    assert (b1p, b2p) == _pows(2)
