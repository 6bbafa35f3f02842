"""CPU: tests/adamw_restated.py IS AdamW. The GPU tests (tests/test_adamw_exact_gpu.py) compare the optimiser kernels with that
module bit for bit; here the module itself is compared with torch.optim.AdamW, its float32 form with its float64 form under a derived
rounding bound, and its 16-bit roundings with torch's conversions."""
import numpy as np
import torch

from tests import adamw_restated as R


def _torch_adamw(x, lr):
    p = torch.nn.Parameter(x)
    return p, torch.optim.AdamW([p], lr=lr, betas=(R.CFG["beta1"], R.CFG["beta2"]), eps=R.CFG["eps"], weight_decay=R.CFG["weight_decay"],
                                foreach=False)


def test_scalars_are_the_float32_casts_of_the_doubles():
    s64 = R.scalars(3e-4, 0.9 ** 7, 0.999 ** 7, dtype=np.float64)
    s32 = R.scalars(3e-4, 0.9 ** 7, 0.999 ** 7)
    for a, b in zip(s32, s64):
        assert type(a) is np.float32 and a == np.float32(b)
    assert s64.decay == 1.0 - 3e-4 * 1e-2 and s64.eps == 1e-8
    assert s64.step_size == 3e-4 / (1.0 - 0.9 ** 7 * 0.9)
    assert s64.bc2_sqrt == (1.0 - 0.999 ** 7 * 0.999) ** 0.5


def test_step64_with_running_products_is_torch_adamw():
    """200 steps on 4096 float64 elements, the learning rate changing every step, gradient magnitudes spread over 1e-12 .. 1e6:
    step64 with the scalars() of a running product beta^t (uncast: dtype=float64) against torch.optim.AdamW (beta ** t) at every step.
    Pins the order of decay and step, both bias corrections, eps outside the root and the running-product form.
    Tolerance 1e-12 relative: of |v| for v; of |m| + |g| for m (the lerp cancels); of |p| + step_size for p (a parameter that
    crosses zero is measured against the step that moved it). Measured: 3.1e-13 at worst -- the running product and beta ** t differ by
    an ulp of beta^t, which 1 - beta2^t (1e-3 .. 0.18 here) magnifies in bc2."""
    n, steps = 4096, 200
    rng = np.random.default_rng(0)
    mag = 10.0 ** rng.uniform(-12, 6, n)
    p0 = rng.standard_normal(n)
    tp, opt = _torch_adamw(torch.from_numpy(p0.copy()), 1e-3)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    b1p = b2p = 1.0
    worst = 0.0
    for k in range(steps):
        lr = 1e-4 + 4e-3 * abs(np.sin(0.37 * k)) * (1.0 + 0.01 * k)
        g = rng.standard_normal(n) * mag
        s = R.scalars(lr, b1p, b2p, dtype=np.float64)
        p, m, v = R.step64(p, g, m, v, s)
        b1p *= R.CFG["beta1"]; b2p *= R.CFG["beta2"]
        opt.param_groups[0]["lr"] = lr
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[tp]
        tm, tv, tq = st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), tp.detach().numpy()
        em = np.abs(m - tm) / (np.abs(tm) + np.abs(g))
        ev = np.abs(v - tv) / np.abs(tv)
        ep = np.abs(p - tq) / (np.abs(tq) + float(s.step_size))
        worst = max(worst, em.max(), ev.max(), ep.max())
        assert em.max() <= 1e-12 and ev.max() <= 1e-12 and ep.max() <= 1e-12, (k, em.max(), ev.max(), ep.max())
    print("step64 vs torch.optim.AdamW, worst relative difference over %d steps: %.2e" % (steps, worst))


def _edge_case():
    n = 1 << 16
    layout = R.flat_layout(0, 4)
    p, g, m, v = R.random_state(n, seed=5)
    pos = np.random.default_rng(6).permutation(n)[:4096]
    cls = R.plant(p, g, m, v, pos)
    return p, g, m, v, pos, cls, layout


def test_step32_meets_the_derived_bound_against_step64():
    """The planted edge classes of the GPU test (g = 0 with and without moments, underflow and overflow of g * g, a subnormal v,
    g = -m, p = 0, an absorbed step) among random elements, at three points of the schedule: step32 against step64 under
    adamw_restated.bounds -- N roundings * 2^-24 * the sum of the absolute terms rounded, derived there for m, v and p, with the
    absolute floor 2^-126. The GPU test applies the same bound to the kernels' output."""
    p, g, m, v, pos, cls, _ = _edge_case()
    assert set(cls) == set(range(len(R.CLASSES)))
    for lr, t in ((1e-4, 0), (5e-3, 3), (6e-4, 400)):
        s = R.scalars(lr, 0.9 ** t, 0.999 ** t)
        p32, m32, v32 = R.step32(p, g, m, v, s)
        p64, m64, v64 = R.step64(p, g, m, v, s)
        bp, bm, bv = R.bounds(p, g, m, v, s)
        for name, x, ref, b in (("m", m32, m64, bm), ("v", v32, v64, bv), ("p", p32, p64, bp)):
            ok = R.within(x, ref, b)
            assert ok.all(), (name, t, [(R.CLASSES[c], x[i], ref[i], b[i]) for i, c in zip(pos, cls) if not ok[i]][:4], np.flatnonzero(~ok)[:8])
        # the classes do what their names say
        at = lambda c: pos[cls == c]
        assert np.isinf(v32[at(4)]).all() and (p32[at(4)] == p[at(4)] * s.decay).all()          # overflow: the update is exactly 0
        assert R.is_subnormal(v32[at(3)]).all()
        assert (v32[at(2)] == v[at(2)] * s.beta2).all()                                          # g * g underflowed to 0
        assert (p32[at(0)] == p[at(0)] * s.decay).all() and (v32[at(0)] == 0).all()              # 0 / eps
        assert (p32[at(7)] == p[at(7)] * s.decay).all()                                          # absorbed
        assert (p32[at(6)] != 0).all() and (m32[at(5)] == m[at(5)] + (g[at(5)] - m[at(5)]) * s.one_minus_beta1).all()
        # and the bound is a rounding bound, not slack: it stays below 2^-20 of the terms' size on every finite element
        fin = np.isfinite(v64)
        assert (bm[fin] <= 2.0 ** -20 * (np.abs(m64[fin]) + np.abs(g[fin].astype(np.float64)) + np.abs(m[fin].astype(np.float64))) + 2 * R.FLOOR).all()


def _bits16(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def _rounding_inputs():
    rng = np.random.default_rng(1)
    xs = [rng.standard_normal(4096).astype(np.float32) * np.float32(10.0) ** rng.integers(-8, 5, 4096).astype(np.float32)]
    f32 = lambda bits: np.asarray(bits, np.uint32).view(np.float32)
    # exact bf16 ties (low 16 bits = 0x8000) above an even and above an odd kept mantissa, both signs
    hi = rng.integers(0x0080, 0x7f7f, 512).astype(np.uint32)
    xs += [f32((hi << 16) | 0x8000), f32((hi << 16) | 0x8000 | 0x80000000), f32(((hi | 1) << 16) | 0x8000), f32(((hi & ~np.uint32(1)) << 16) | 0x8000)]
    # ... one float32 unit to either side of a tie
    xs += [f32((hi << 16) | 0x7fff), f32((hi << 16) | 0x8001)]
    # round up into the next binade: mantissa all ones
    e = rng.integers(1, 254, 256).astype(np.uint32)
    xs += [f32((e << 23) | 0x7fffff), f32((e << 23) | 0x7f8000), f32((e << 23) | 0x7fffff | 0x80000000)]
    # exact fp16 ties (13 dropped bits = 0x1000) in the fp16 normal range, even and odd kept mantissa, both signs; binade carries
    e16 = rng.integers(113, 142, 512).astype(np.uint32)       # float32 exponents of 2^-14 .. 2^14
    mant = rng.integers(0, 1 << 10, 512).astype(np.uint32)
    xs += [f32((e16 << 23) | (mant << 13) | 0x1000), f32((e16 << 23) | (mant << 13) | 0x1000 | 0x80000000),
           f32((e16 << 23) | (mant << 13) | 0x0fff), f32((e16 << 23) | (mant << 13) | 0x1001), f32((e16 << 23) | 0x7ff000), f32((e16 << 23) | 0x7fffff)]
    # +-0, fp16 subnormals (below 2^-14 = 6.1e-5, down to and below half of the smallest one, 2^-25) with their ties
    k = np.arange(0, 2049, dtype=np.float64)
    xs += [np.array([0.0, -0.0], np.float32), (k * 2.0 ** -25).astype(np.float32), (-k * 2.0 ** -25).astype(np.float32),
           np.array([2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23), 2.0 ** -25 * (1 - 2.0 ** -24), 2.0 ** -26, 3 * 2.0 ** -25, 1e-10, -1e-10], np.float32)]
    # magnitudes above 65504: the last finite fp16, the tie to infinity (65520) and its neighbours, and far beyond
    xs += [np.array([65504.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e5, 1e30, -65504.0, -65519.996, -65520.0, -1e5, 3.3e38, -3.3e38], np.float32)]
    return np.concatenate([np.asarray(x, np.float32).ravel() for x in xs])


def test_16_bit_roundings_are_torchs():
    x = _rounding_inputs()
    t = torch.from_numpy(x.copy())
    np.testing.assert_array_equal(R.rne_bf16(x), _bits16(t.to(torch.bfloat16)))
    np.testing.assert_array_equal(R.rne_fp16(x), _bits16(t.to(torch.float16)))
    # the inputs do contain what they claim: ties resolved in both directions, infinities, subnormals
    b = R.rne_bf16(x).astype(np.uint32) << 16
    tie = (x.view(np.uint32) & 0xffff) == 0x8000
    up = np.abs(b.view(np.float32)[tie]) > np.abs(x[tie])
    assert up.any() and (~up).any()
    h = R.rne_fp16(x).view(np.float16)
    assert np.isinf(h).any() and ((h != 0) & (np.abs(h) < np.float16(6.1e-5))).any()


def test_calibration_step_is_torch_adamw_on_a_float32_scalar():
    """calib_step (double arithmetic, float32 state, bias corrections by pow) against torch.optim.AdamW on a float32 scalar at
    lr = 1e-3, 50 free-running steps. The trainer reports focal_scale = 1 + g, and that is what is bounded, here and on the GPU: one
    float32 unit in the last place at 1, 2^-23. (In units of the small parameter itself the two differ by a few ulp from the first step
    on: torch rounds each of its ~10 operations to float32, the restatement rounds once per step. Printed below.)"""
    rng = np.random.default_rng(2)
    gs = list(rng.standard_normal(50) * 10.0 ** rng.uniform(-3, 3, 50))
    gs[3], gs[4], gs[40], gs[41] = 0.0, 0.0, 1e6, -1e6   # (late: v keeps the memory of 1e12 for a thousand steps)
    tp, opt = _torch_adamw(torch.zeros((), dtype=torch.float32), 1e-3)
    p = m = v = 0.0
    worst = worst_ulp = travelled = 0.0
    for k, g in enumerate(gs):
        g = float(np.float32(g))
        before = p
        p, m, v = R.calib_step(p, m, v, g, k + 1)
        travelled += abs(p - before)
        assert p == float(np.float32(p)) and m == float(np.float32(m)) and v == float(np.float32(v))
        tp.grad = torch.tensor(g, dtype=torch.float32)
        opt.step()
        ref = float(tp.detach())
        worst = max(worst, abs(p - ref))
        worst_ulp = max(worst_ulp, abs(p - ref) / float(np.spacing(np.float32(abs(ref)))))
        assert abs((1.0 + p) - (1.0 + ref)) <= 2.0 ** -23, (k, p, ref)
    assert travelled > 1e-2    # the scalar did move: many steps of ~lr each
    print("calib_step vs torch float32 AdamW over 50 steps: worst |difference| %.2e = %.1f ulp of the parameter" % (worst, worst_ulp))


def test_flat_layout_restates_the_trainers_views():
    lay = R.flat_layout(1, 4)
    assert [x[0] for x in lay][:4] == ["res3_conv1.weight", "res3_conv1.bias", "res3_conv2.weight", "res3_conv2.bias"]
    assert lay[-2] == ("fc3.weight", 8 * 262656, (4, 512)) and lay[-1] == ("fc3.bias", 8 * 262656 + 2048, (4,))
    assert R.num_params(1, 4) == 8 * 262656 + 2052
    assert R.locate(lay, 3 * 262656 + 17 * 512 + 40).startswith("layer 3 0c0.weight, row 17, column 40")
    pos = R.planted_positions(lay)
    assert len(np.unique(pos)) == len(pos) and pos.max() < R.num_params(1, 4)
    for name, o, shape in lay:
        assert o in pos and o + int(np.prod(shape)) - 1 in pos
    o = lay[2][1]
    for r, c in ((63, 64), (64, 63), (448, 447), (0, 511), (511, 0), (127, 128)):
        assert o + r * 512 + c in pos
