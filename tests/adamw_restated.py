"""The optimiser stage of the head's training step, restated in plain numpy (no import from the package or the oracle).

What is restated, and where it lives in the kernels:
  scalars()      sched_prepare_hot (head_sched.h): the seven AdamScalars of a step, computed in double and cast to float32
  step32()       adamw_one / adamw_small_one (head_opt.h, pose_kernels.hip): five un-contracted float32 lines
  step64()       the same formula in float64 from the same float32 inputs: the yardstick of the rounding bound
  bounds()       the per-element distance a correct float32 evaluation may keep from step64 (derived below)
  rne_bf16/fp16  the recast of the fp32 masters into the 16-bit compute copies (round to nearest, ties to even)
  calib_step()   the calibration scalar's own AdamW inside sched_post_wave (double arithmetic, float32 state)
  flat_layout()  HeadTrainer._views: where each layer's weight and bias sit in the flat parameter vector

torch.optim.AdamW semantics (single tensor): decay first, then the moments, then the step with both bias corrections; eps is added
OUTSIDE the square root, after the division by sqrt(1 - beta2^t)."""
import collections
import math

import numpy as np

CFG = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)   # torch.optim.AdamW defaults (head.py: cfg.beta1 ... cfg.weight_decay)

AdamScalars = collections.namedtuple("AdamScalars", "decay one_minus_beta1 beta2 one_minus_beta2 bc2_sqrt eps step_size")

U = 2.0 ** -24          # unit roundoff of float32 (round to nearest)
FLOOR = 2.0 ** -126     # smallest normal float32: the absolute floor of every bound (a result below it may be rounded on the
#                         subnormal grid, spacing 2^-149, or flushed to zero)
F32_OVF = (2.0 - 2.0 ** -24) * 2.0 ** 127   # magnitudes from here on round to +-inf in float32 (largest float32 + half a unit of its last place)


def scalars(lr, beta1_pow, beta2_pow, cfg=CFG, dtype=np.float32):
    """The AdamScalars of the step that FOLLOWS `beta1_pow` = beta1^t, `beta2_pow` = beta2^t completed steps (running products, 1.0
    before the first step; the caller multiplies them by beta after a step that was applied). Python doubles, cast to `dtype` at the
    end (float32: what the kernels read; float64: the uncast values, for the comparison with torch in double)."""
    lr = float(lr)
    b1p = float(beta1_pow) * cfg["beta1"]
    b2p = float(beta2_pow) * cfg["beta2"]
    bc1 = 1.0 - b1p
    bc2 = 1.0 - b2p
    return AdamScalars(*(dtype(x) for x in (1.0 - lr * cfg["weight_decay"], 1.0 - cfg["beta1"], cfg["beta2"], 1.0 - cfg["beta2"],
                                            math.sqrt(bc2), cfg["eps"], lr / bc1)))


def step32(p, g, m, v, s):
    """One AdamW step on float32 arrays: the five lines of adamw_one in their order, one numpy operation per rounding.
    Returns (p, m, v); the inputs are not modified. Overflow to inf and underflow are the float32 ones (no warnings raised)."""
    p, g, m, v = (np.asarray(x, np.float32) for x in (p, g, m, v))
    s = AdamScalars(*(np.float32(x) for x in s))
    with np.errstate(all="ignore"):
        pd = p * s.decay                         # p = p * s.decay
        t = g - m                                # m = m + (g - m) * s.one_minus_beta1
        t = t * s.one_minus_beta1
        m = m + t
        a = v * s.beta2                          # v = v * s.beta2 + s.one_minus_beta2 * g * g      ((omb2 * g) * g)
        b = s.one_minus_beta2 * g
        b = b * g
        v = a + b
        d = np.sqrt(v)                           # denom = sqrtf(v) / s.bc2_sqrt + s.eps
        d = d / s.bc2_sqrt
        d = d + s.eps
        q = m / d                                # return p - s.step_size * (m / denom)
        q = s.step_size * q
        p = pd - q
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def _ovf(x):
    """A float64 term in the magnitude class float32 rounding would leave it in: past the float32 range it is +-inf."""
    return np.where(np.abs(x) >= F32_OVF, np.copysign(np.inf, x), x)


def _terms64(p, g, m, v, s):
    p, g, m, v = (np.asarray(x).astype(np.float64) for x in (p, g, m, v))   # (float32 inputs convert exactly)
    s = AdamScalars(*(np.float64(x) for x in s))
    with np.errstate(all="ignore"):
        T = {"g": g}
        T["a_p"] = _ovf(p * s.decay)
        T["gm"] = _ovf(g - m)
        T["t"] = _ovf(T["gm"] * s.one_minus_beta1)
        T["m"] = _ovf(m + T["t"])
        T["a_v"] = _ovf(v * s.beta2)
        T["c"] = _ovf(_ovf(s.one_minus_beta2 * g) * g)
        T["v"] = _ovf(T["a_v"] + T["c"])
        T["d"] = _ovf(_ovf(np.sqrt(T["v"]) / s.bc2_sqrt) + s.eps)
        T["q"] = _ovf(T["m"] / T["d"])
        T["r"] = _ovf(s.step_size * T["q"])
        T["p"] = _ovf(T["a_p"] - T["r"])
    return T, s


def step64(p, g, m, v, s):
    """The same formula in float64, from the inputs (float32 arrays convert exactly) and the scalars as given. One rule of float32 is kept, because it
    is part of the operation and not a rounding: a term whose magnitude exceeds the largest float32 is +-inf (g * g for |g| = 1e25:
    v = inf, the denominator is inf and the update is exactly 0 -- torch's float32 AdamW does the same)."""
    T, _ = _terms64(p, g, m, v, s)
    return T["p"], T["m"], T["v"]


def bounds(p, g, m, v, s):
    """(bound_p, bound_m, bound_v): how far a correct float32 evaluation of the five lines may be from step64, per element.

    Notation: u = 2^-24; fl(x) = x (1 + d), |d| <= u for a normal result; every bound carries the absolute floor 2^-126 for results
    below the normal range. The rule is: (number of float32 roundings on the path) * u * (sum of the absolute values of the terms
    rounded, each in units of the result). The factor N over-counts the first-order sum (each term's rounding enters once), which
    leaves room for the second-order terms a first-order analysis drops.

    m' = fl(m + fl(fl(g - m) * omb1)): N = 3, terms g - m (its error is then scaled by omb1 < 1), t = (g - m) omb1, m'.
        bound_m = 3 u (|g - m| + |t| + |m'|)
    v' = fl(fl(v beta2) + fl(fl(omb2 g) g)): N = 4, terms a = v beta2, omb2 g (its error scaled by g: u |c|), c = omb2 g g, v'.
        bound_v = 4 u (|a| + 2 |c| + |v'|)
    p' = fl(a - r), a = fl(p decay), r = fl(step fl(m' / d)), d = fl(fl(fl(sqrt v') / bc2s) + eps): N = 7 roundings of its own. Those of
        sqrt, the division by bc2s and the sum each move d by at most u d (sqrt(v') / bc2s <= d), hence r by u |r|; the quotient and the
        product move r by u |r| each:
        own = 7 u (|a| + |r| + |p'|)
      On top, p' inherits the errors of m' and v' through q = m' / d:
        E_s = min(bound_v / (2 sqrt v'), sqrt(bound_v))        (|sqrt(x + e) - sqrt(x)| <= both)
        inherited = step (bound_m / d + |q| E_s / (bc2s d))
        bound_p = own + inherited
    Where v' = inf (overflow of g * g) both evaluations give d = inf, q = 0 and p' = a: nothing is inherited."""
    T, s = _terms64(p, g, m, v, s)
    A = np.abs
    with np.errstate(all="ignore"):
        bm = 3 * U * (A(T["gm"]) + A(T["t"]) + A(T["m"])) + FLOOR
        bv = 4 * U * (A(T["a_v"]) + 2 * A(T["c"]) + A(T["v"])) + FLOOR
        own = 7 * U * (A(T["a_p"]) + A(T["r"]) + A(T["p"]))
        sv = np.sqrt(T["v"])
        e_s = np.minimum(np.where(sv > 0, bv / (2 * np.where(sv > 0, sv, 1.0)), np.inf), np.sqrt(bv))
        inh = s.step_size * (bm / T["d"] + A(T["q"]) * e_s / (s.bc2_sqrt * T["d"]))
        inh = np.where(np.isinf(T["v"]), 0.0, inh)
        bp = own + inh + FLOOR
    return bp, bm, bv


def within(x, ref, bound):
    """Elementwise: x meets `bound` against ref; an infinite reference is met by the same infinity only."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.isinf(ref), x == ref, np.abs(x - ref) <= bound)


def rne_bf16(x):
    """float32 -> bf16 bit patterns (uint16): integer round-to-nearest-even on the float32 bits (no NaN inputs)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7fff + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


def rne_fp16(x):
    """float32 -> fp16 bit patterns (uint16): IEEE round-to-nearest-even with subnormals; beyond 65520 it is +-inf."""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(x, np.float32).astype(np.float16).view(np.uint16)


def calib_step(p, m, v, g, step, cfg=CFG, lr=1e-3):
    """One AdamW step of the calibration scalar (sched_post_wave): double arithmetic, the bias corrections by pow, and p, m, v
    rounded through float32 after the step (a float32 parameter in the reference). `step` counts from 1. Returns (p, m, v)."""
    p, m, v, g = float(p), float(m), float(v), float(g)
    p = p * (1.0 - lr * cfg["weight_decay"])
    m = m + (g - m) * (1.0 - cfg["beta1"])
    v = v * cfg["beta2"] + (1.0 - cfg["beta2"]) * g * g
    bc1 = 1.0 - math.pow(cfg["beta1"], float(step))
    bc2 = 1.0 - math.pow(cfg["beta2"], float(step))
    denom = math.sqrt(v) / math.sqrt(bc2) + cfg["eps"]
    p = p - (lr / bc1) * (m / denom)
    with np.errstate(over="ignore"):
        return float(np.float32(p)), float(np.float32(m)), float(np.float32(v))


def is_subnormal(x):
    x = np.abs(np.asarray(x, np.float32))
    return (x > 0) & (x < np.float32(FLOOR))


# ---- the edge classes of the optimiser arithmetic, planted at chosen positions of a state (shared by the CPU and GPU tests) ----
CLASSES = ("g=0, m=0, v=0: the denominator is eps alone", "g=0, m!=0", "|g|=1e-30: g*g underflows", "|g|=1e-20: v lands subnormal",
           "|g|=1e25: g*g overflows, v=inf, the update is 0", "g=-m", "p=0", "|p| so large that the step is absorbed")


def random_state(n, seed, p_scale=0.05):
    """(p, g, m, v) float32 of n elements from a seeded generator: magnitudes spread over several decades, everything in the normal
    range, v > 0."""
    rng = np.random.default_rng(seed)
    dec = lambda lo, hi: 10.0 ** rng.uniform(lo, hi, n)
    p = (rng.standard_normal(n) * p_scale).astype(np.float32)
    g = (rng.standard_normal(n) * dec(-8, 0)).astype(np.float32)
    m = (rng.standard_normal(n) * dec(-8, -2)).astype(np.float32)
    # v >= m^2, as after real steps: |m| / sqrt(v) <= 1 keeps every update of the order of the learning rate, so that the updated
    # parameters are still weights a forward pass can run on
    v = ((np.abs(m.astype(np.float64)) * (1.0 + 3.0 * np.abs(rng.standard_normal(n)))) ** 2).astype(np.float32)
    assert v.min() >= FLOOR
    return p, g, m, v


def plant(p, g, m, v, positions, p_large=0.5):
    """Write the classes into the arrays (in place; any of p, m, v may be None: that part of a class is then left as it is), class
    k % 8 with sign (-1)^(k // 8) at positions[k]. Returns the class of every position."""
    positions = np.asarray(positions, np.int64)
    k = np.arange(len(positions))
    cls, sgn = k % len(CLASSES), np.where((k // len(CLASSES)) % 2 == 0, 1.0, -1.0).astype(np.float32)

    def put(arr, c, val):
        if arr is not None:
            sel = cls == c
            arr[positions[sel]] = (val[sel] if isinstance(val, np.ndarray) else val)
    put(g, 0, 0.0); put(m, 0, 0.0); put(v, 0, 0.0)
    put(g, 1, 0.0)
    if m is not None:
        put(m, 1, sgn * np.float32(3e-3)); put(v, 1, np.float32(1e-4))
    put(g, 2, sgn * np.float32(1e-30))
    put(g, 3, sgn * np.float32(1e-20)); put(m, 3, 0.0); put(v, 3, 0.0)
    put(g, 4, sgn * np.float32(1e25))
    if m is not None:
        sel = cls == 5
        g[positions[sel]] = -m[positions[sel]]
    put(p, 6, 0.0)
    # large against its step, that is: m / sqrt(v) = 1e-6 makes the step ~1e-6 * step_size, far below half a unit in the last place of
    # |p| = 0.5 (the weights stay usable in an fp16 forward, which the tests run on the updated masters)
    put(p, 7, sgn * np.float32(p_large)); put(g, 7, np.float32(1e-6)); put(m, 7, np.float32(1e-6)); put(v, 7, np.float32(1.0))
    return cls


def planted_positions(layout, tile_layer=1, extra=2048, seed=0):
    """Flat indices: the first and last element of every tensor of the layout, the elements on both sides of every 64 x 64 tile edge
    of one wide layer's weight (rows and columns 63|64, 127|128, ... crossed with each other and with the matrix's border), and
    `extra` seeded positions anywhere. Unique, in a fixed order."""
    pos = []
    for name, o, shape in layout:
        pos += [o, o + int(np.prod(shape)) - 1]
    _, o, _ = layout[2 * tile_layer]
    edges = [0] + [e for k in range(1, 8) for e in (64 * k - 1, 64 * k)] + [511]
    pos += [o + r * 512 + c for r in edges for c in edges]
    n = layout[-1][1] + int(np.prod(layout[-1][2]))
    pos += list(np.random.default_rng(seed).integers(0, n, extra))
    _, first = np.unique(np.asarray(pos, np.int64), return_index=True)
    return np.asarray(pos, np.int64)[np.sort(first)]


def layer_names(num_head_blocks):
    names = ["res3_conv1", "res3_conv2", "res3_conv3"]
    for b in range(num_head_blocks):
        names += [f"{b}c0", f"{b}c1", f"{b}c2"]
    return names + ["fc1", "fc2"]


def flat_layout(num_head_blocks, n_out):
    """[(name, offset, shape)] of every tensor in the flat parameter vector, in order: per wide layer a 512 x 512 weight and a
    512 bias, then fc3.weight [n_out, 512] and fc3.bias [n_out]. The last entry's offset + size is the parameter count."""
    out, o = [], 0
    for name in layer_names(num_head_blocks):
        out.append((name + ".weight", o, (512, 512)))
        o += 262144
        out.append((name + ".bias", o, (512,)))
        o += 512
    out.append(("fc3.weight", o, (n_out, 512)))
    o += n_out * 512
    out.append(("fc3.bias", o, (n_out,)))
    return out


def num_params(num_head_blocks, n_out):
    name, o, shape = flat_layout(num_head_blocks, n_out)[-1]
    return o + int(np.prod(shape))


def locate(layout, i):
    """'layer 3 weight, row 17, column 40' for a flat index."""
    for k, (name, o, shape) in enumerate(layout):
        n = int(np.prod(shape))
        if o <= i < o + n:
            r = i - o
            where = f"row {r // shape[1]}, column {r % shape[1]}" if len(shape) == 2 else f"element {r}"
            return f"layer {k // 2} {name}, {where} (flat {i})"
    return f"outside the parameters (flat {i})"
