"""The loss stage of the head's training step (head_kernels.hip loss_body, phases A, B, C) restated in float64 interval arithmetic from
the stage's own operands, and judged per row and per element.

Operands, all as stored: out[L - 1] (debug_read 'out'), the 16-bit compute copy of W3 (debug_read 'W3') and the fp32 b3, the buffer
tables the test passed to set_buffer, the scene mean and the configuration scalars, and loss_weight / calib_g / grad_scale of the judged
iteration (a backward() at iteration 0: head_optim.hip's initial state, or head_sched.h's formula for the weight).

One text, three arithmetics. `geometry` / `loss_rows` / `phase_c` are written ONCE over an arithmetic object:
  * IvArith  -- every value is an interval [lo, hi] of float64 over the rows, every operation widens outwards: an fp32 + - x / fma by
                2^-24 of the result's magnitude (plus 2^-50 of it for the float64 arithmetic of the restatement, plus 2^-149 for a result
                that underflows), a device math call by its bound in ulps of the result (tests/golden/parity_tolerances.json,
                "loss_stage_math_ulps"). A product-sum the compiler may contract is evaluated with every rounding: the set of values that
                allows contains what any contraction gives. An interval that is exactly 0 stays exactly 0. An operation that cannot be
                contracted and whose operands are all exact fp32 values (the tables, the stored X, the explicit fmaf chains of the
                projection, the correctly rounded division) has ONE result, which is taken (IvArith._pointwise): the pixel error e
                of a row, and so every comparison on it, is decided exactly -- e == inlier_px included.
  * F32Arith -- numpy float32, the stand-in of the kernel on the CPU (tests/test_loss_stage_cpu.py), with product-sums contracted into
                FMAs or not, and with the mutants the checker must catch.
  * the third is torch float64 (`forward_torch`): only the forward pass, written separately; autograd's d(loss)/ds must equal the interval
    midpoints, and oracle/head_oracle.py (pinned against the reference) must agree on loss, inliers and ds. So the text below is held by
    autograd and by the oracle, not by the kernel's text.

Comparisons (`bx > 20`, `hraw > min_inv_scale`, `pp[2] < depth_min`, the three validity tests, `tavail`, `tdist > 0.1`, `tdist > 0`,
`e > wgt`, `e < inlier_px`, sgn(du), sgn(dv), the proxy target's sgn(d)) are decided where the intervals do not meet. A row with an
undecided comparison that matters is evaluated on every feasible side (a depth-first walk over its undecided sites) and carries the hull;
such rows are counted, nothing is left out.

X is an output AND an operand: the kernel stores the very fp32 value it goes on computing with. It is judged against its interval, and
the restatement continues from the stored value (so a target_crds equal to the kernel's X gives tdist == 0 exactly).

Phase A: s_j = sum x w3_j + b3_j, fp32 FMAs and the DPP wave sum, 513 terms: within 513 * 2^-24 * sum |terms| of the float64 value in any
order (no matrix instruction: no doubling). Phase C: d = sum_j fma(ds_j, w3_jc) as an interval; the stored dZ element passes iff it lies
between the 16-bit roundings of the interval's ends (monotone map, as in tests/head_stage_restated.py); the ReLU mask is exactly
`stored out[L - 1] > 0`. fp16 values are in scaled units; the scale is a power of two.

Bit for bit: bias_partials[L - 1] from the stored dZ rows (sequential fp32 sum in row order over a block's rows below n), and the fc3 /
statistics entries of tr.grad from the partials that were read (lane j adds blocks j, j + 64, .. in order, xor butterfly 32 .. 1,
x inv_grad_scale for the fc3 entries: head_opt.h tail_output).

A pose configuration (pose_refinement 'naive': the matrices are the parameters, orthonormalised on the device) adds row_dT, judged
as intervals from the refined matrices the loss read (debug_read 'pose_cur'), and row_image, exact."""
import json
import os

import numpy as np
import torch

from tests import ordered_sums
from tests.head_stage_restated import Fmt

U = 2.0 ** -24
EPS64 = 2.0 ** -50
TINY = 2.0 ** -149
BLOCK = 16                # rows of a loss block (loss_kernel<E, 4>: four waves of four rows)
LOSS_IDS = {"tanh": 0, "dyntanh": 1, "l1": 2, "l1+sqrt": 3, "l1+log": 4}


def math_ulps():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parity_tolerances.json")) as f:
        d = json.load(f)["loss_stage_math_ulps"]
    return {k: float(v) for k, v in d.items() if not k.startswith("_")}


# ------------------------------------------------------------------------------------------------ intervals
class Iv:
    __slots__ = ("lo", "hi")

    def __init__(self, lo, hi=None):
        self.lo = np.asarray(lo, np.float64)
        self.hi = self.lo if hi is None else np.asarray(hi, np.float64)

    @property
    def mid(self):
        return 0.5 * (self.lo + self.hi)

    @property
    def rad(self):
        return 0.5 * (self.hi - self.lo)

    def __getitem__(self, k):
        return Iv(self.lo[k], self.hi[k])

    def contains(self, x):
        return (self.lo <= x) & (x <= self.hi)


def _widen(lo, hi, rel=U):
    m = np.maximum(np.abs(lo), np.abs(hi))
    w = np.where((lo == 0) & (hi == 0), 0.0, m * (rel + EPS64) + TINY)
    return Iv(lo - w, hi + w)


def _ulp(m):
    """ulp of an fp32 number of magnitude m (>= the smallest normal's)."""
    _, e = np.frexp(np.maximum(m, 2.0 ** -126))
    return np.ldexp(1.0, e - 24)


def _mul_raw(a, b):
    p = np.stack([a.lo * b.lo, a.lo * b.hi, a.hi * b.lo, a.hi * b.hi])
    return p.min(0), p.max(0)


class IvArith:
    """Interval arithmetic over rows; `forced`: site -> the outcome to take where that comparison is undecided; after a pass
    `undecided[site]` marks the rows where the site was undecided AND mattered, `options[site]` the feasible outcomes there."""
    interval = True
    mut = frozenset()

    def __init__(self, ulps, forced=None, points=True, zero_width=False):
        # zero_width: no widening at all -- the float64 value of the same text (what autograd of the second forward is compared with)
        self.ulps, self.forced, self.points, self.zero = ulps, dict(forced or {}), points and not zero_width, zero_width
        self.undecided, self.options = {}, {}

    def _w(self, lo, hi):
        return Iv(lo, hi) if self.zero else _widen(lo, hi)

    def c(self, x):
        return Iv(np.asarray(x, np.float64))

    # One fp32 operation on operands that are all POINTS (exact fp32 values: table entries, the stored X and what follows from them by
    # such operations) has one possible result, the correctly rounded one: + - x fma by IEEE, the division as measured (0.5 ulp,
    # tools/math_ulp.hip). It is taken from the float64 result, unless that result is itself rounded (`exact` false) AND lies within
    # 2^-50 of a rounding tie of fp32, or the result is subnormal: then, as for every other operand, the widened interval stands.
    def _pointwise(self, v64, ops, wide, exact):
        if not self.points:              # (the autograd and oracle comparisons: midpoints that follow the float64 value)
            return wide
        pt = np.ones(np.shape(v64), bool)
        for o in ops:
            pt &= o.lo == o.hi
        with np.errstate(all="ignore"):
            r = np.asarray(v64, np.float64).astype(np.float32).astype(np.float64)
            m = np.abs(r)
            safe = np.isfinite(r) & ((r == 0) & (v64 == 0) | (m >= 2.0 ** -126)) & (exact | (np.abs(np.abs(v64 - r) - 0.5 * _ulp(m)) > m * EPS64))
        pt &= safe
        if not pt.any():
            return wide
        return Iv(np.where(pt, r, wide.lo), np.where(pt, r, wide.hi))

    @staticmethod
    def _sum_exact(x, y, s):             # TwoSum: the float64 sum s = x + y carries no rounding error
        with np.errstate(all="ignore"):
            yy = s - x
            return ((x - (s - yy)) + (y - yy)) == 0

    def add(self, a, b):
        s = a.lo + b.lo
        return self._pointwise(s, (a, b), self._w(s, a.hi + b.hi), self._sum_exact(a.lo, b.lo, s))

    def sub(self, a, b):
        s = a.lo - b.lo
        return self._pointwise(s, (a, b), self._w(a.lo - b.hi, a.hi - b.lo), self._sum_exact(a.lo, -b.lo, s))

    def mul(self, a, b, fusable=False):  # fusable: the product feeds an addition the compiler may contract it into
        w = self._w(*_mul_raw(a, b))
        return w if fusable else self._pointwise(a.lo * b.lo, (a, b), w, True)   # (24 x 24 bits: exact in float64)

    def div(self, a, b):
        assert bool(np.all((b.lo > 0) | (b.hi < 0))), "a divisor's interval meets zero"
        q = np.stack([a.lo / b.lo, a.lo / b.hi, a.hi / b.lo, a.hi / b.hi])
        with np.errstate(all="ignore"):  # (a tie of fp32 has 25 bits: its product with b is exact in float64)
            exact = q[0] * b.lo == a.lo
        return self._pointwise(q[0], (a, b), self._w(q.min(0), q.max(0)), exact)

    def fma(self, a, b, c):
        lo, hi = _mul_raw(a, b)
        p = a.lo * b.lo
        return self._pointwise(p + c.lo, (a, b, c), self._w(lo + c.lo, hi + c.hi), self._sum_exact(p, c.lo, p + c.lo))

    def _add_w(self, a, b):
        return self._w(a.lo + b.lo, a.hi + b.hi)

    def mul_add(self, a, b, c):          # a * b + c as the compiler likes: every rounding
        return self._add_w(self.mul(a, b, True), c)

    def dot(self, pairs, tail=None):     # a0 b0 + a1 b1 + .. (+ tail), left to right
        acc = self.mul(*pairs[0], True)
        for a, b in pairs[1:]:
            acc = self._add_w(acc, self.mul(a, b, True))
        return acc if tail is None else self._add_w(acc, tail)

    def neg(self, a):
        return Iv(-a.hi, -a.lo)

    def fabs(self, a):
        lo = np.where((a.lo <= 0) & (a.hi >= 0), 0.0, np.minimum(np.abs(a.lo), np.abs(a.hi)))
        return Iv(lo, np.maximum(np.abs(a.lo), np.abs(a.hi)))

    def scale(self, a, k):               # by a power of two (k > 0): exact
        return Iv(a.lo * k, a.hi * k)

    def times_sign(self, a, sg):         # by an exact -1 / 0 / +1
        lo, hi = _mul_raw(a, sg)
        return Iv(lo, hi)

    def _fn(self, name, f, a):
        with np.errstate(all="ignore"):
            lo, hi = f(a.lo), f(a.hi)
        m = np.maximum(np.abs(lo), np.abs(hi))
        w = np.where((lo == 0) & (hi == 0), 0.0, self.ulps[name] * _ulp(m) + m * EPS64)
        return Iv(lo, hi) if self.zero else Iv(lo - w, hi + w)

    def exp(self, a):
        return self._fn("expf", np.exp, a)

    def log1p(self, a):
        return self._fn("log1pf", np.log1p, Iv(np.maximum(a.lo, 0.0), a.hi))

    def tanh(self, a):
        return self._fn("tanhf", np.tanh, a)

    def log(self, a):
        return self._fn("logf", np.log, a)

    def sqrt(self, a):
        r = self._fn("sqrtf", np.sqrt, Iv(np.maximum(a.lo, 0.0), np.maximum(a.hi, 0.0)))
        return Iv(np.maximum(r.lo, 0.0), r.hi)

    def positive(self, a):               # a square root known to be > 0: no smaller than that of the smallest fp32 number
        return Iv(np.maximum(a.lo, 2.0 ** -75), np.maximum(a.hi, 2.0 ** -75))

    def where(self, c, a, b):
        return Iv(np.where(c, a.lo, b.lo), np.where(c, a.hi, b.hi))

    def _site(self, site, yes, no, live, options):
        und = ~(yes | no) & live
        self.undecided[site] = self.undecided.get(site, False) | und
        self.options[site] = options
        return und

    def gt(self, a, b, site, live):
        yes, no = a.lo > b.hi, a.hi <= b.lo
        und = self._site(site, yes, no, live, (False, True))
        return np.where(und, bool(self.forced.get(site, False)), yes)

    def lt(self, a, b, site, live):
        return self.gt(b, a, site, live)

    def sgn(self, a, site, live):
        pos, neg, zero = a.lo > 0, a.hi < 0, (a.lo == 0) & (a.hi == 0)
        und = self._site(site, pos | neg, zero, live, (-1.0, 0.0, 1.0))
        v = np.where(pos, 1.0, np.where(neg, -1.0, 0.0))
        return Iv(np.where(und, float(self.forced.get(site, 0.0)), v))


class F32Arith:
    """The kernel's arithmetic in numpy float32. contract: product-sums become FMAs (one rounding, through float64: a float32 product is
    exact there). mut: the mutants of tests/test_loss_stage_cpu.py."""
    interval = False

    def __init__(self, contract, mut=()):
        self.contract, self.mut = bool(contract), frozenset(mut)

    def c(self, x):
        return np.asarray(x, np.float32)

    def add(self, a, b):
        return a + b

    def sub(self, a, b):
        return a - b

    def mul(self, a, b, fusable=False):
        return a * b

    def div(self, a, b):
        with np.errstate(all="ignore"):
            return a / b

    def fma(self, a, b, c):
        with np.errstate(all="ignore"):
            return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)

    def mul_add(self, a, b, c):
        return self.fma(a, b, c) if self.contract else a * b + c

    def dot(self, pairs, tail=None):
        acc = pairs[0][0] * pairs[0][1]
        for a, b in pairs[1:]:
            acc = self.fma(a, b, acc) if self.contract else acc + a * b
        return acc if tail is None else acc + tail

    def neg(self, a):
        return -a

    def fabs(self, a):
        return np.abs(a)

    def scale(self, a, k):
        return a * np.float32(k)

    def times_sign(self, a, sg):
        return a * sg

    def exp(self, a):
        with np.errstate(all="ignore"):
            return np.exp(a)

    def log1p(self, a):
        return np.log1p(a)

    def tanh(self, a):
        return np.tanh(a)

    def log(self, a):
        with np.errstate(all="ignore"):
            return np.log(a)

    def sqrt(self, a):
        with np.errstate(all="ignore"):
            return np.sqrt(a)

    def positive(self, a):
        return a

    def where(self, c, a, b):
        return np.where(c, a, b)

    def gt(self, a, b, site, live):
        return a > b

    def lt(self, a, b, site, live):
        if site == "e<inlier" and "inlier_le" in self.mut:
            return a <= b
        return a < b

    def sgn(self, a, site, live):
        return np.sign(a).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the stage, written once
def f32(x):
    return float(np.float32(x))


def make_cfg(*, homog, loss_type, mean, refine_calibration=False, focal_init=0.0, calib_g=0.0, global_batch, wgt, grad_scale=1.0, f16=False, pose=False,
             hard_clamp=1000.0, depth_min=0.1, depth_max=1000.0, depth_target=10.0, inlier_px=10.0, min_scale=0.01, max_scale=4.0):
    """The scalars loss_body reads, as the fp32 values it reads (HeadTrainer.buffers' float32 arithmetic for the homogeneous constants)."""
    mx, mn = torch.tensor([max_scale]), torch.tensor([min_scale])
    return dict(pose=bool(pose), homog=bool(homog), loss=LOSS_IDS[loss_type], mean=[f32(m) for m in np.asarray(mean).reshape(3)],
                max_inv_scale=f32(float(1.0 / mx)), min_inv_scale=f32(float(1.0 / mn)), h_beta=f32(float(np.log(2) / (1.0 - 1.0 / mx))),
                calib=bool(refine_calibration), focal_init=f32(focal_init), calib_g=f32(calib_g), inv_batch=f32(np.float32(1.0) / np.float32(global_batch)),
                wgt=f32(wgt), gscale=float(grad_scale), f16=bool(f16), hard_clamp=f32(hard_clamp), depth_min=f32(depth_min),
                depth_max=f32(depth_max), depth_target=f32(depth_target), inlier_px=f32(inlier_px))


def geometry(A, X, t, c):
    """P = A . T, the intrinsics of the iteration, the camera coordinates and the homogeneous pixel of X (three values over rows).
    Explicit fmaf chains in the kernel: from point operands every value here is a point."""
    rows = t["tu"].shape[0]
    K_ = lambda x: A.c(np.full(rows, x))
    col = lambda a, i: A.c(a[:, i])
    zero, one = K_(0.0), K_(1.0)
    Am = [col(t["A"], i) for i in range(12)]
    Tm = [col(t["T"], i) for i in range(16)]
    K = [col(t["K"], i) for i in range(9)]
    kscale = None
    if c["calib"]:
        kscale = A.div(K[0], K_(c["focal_init"]))
        f = A.mul(A.mul(A.add(one, K_(c["calib_g"])), K_(c["focal_init"])), kscale)
        K[0], K[1], K[3], K[4] = f, zero, zero, f
    P = []
    for i in range(3):
        for j in range(4):
            acc = zero
            for k in range(4):
                acc = A.fma(Am[i * 4 + k], Tm[k * 4 + j], acc)
            P.append(acc)
    Xc = [A.fma(P[i * 4], X[0], A.fma(P[i * 4 + 1], X[1], A.fma(P[i * 4 + 2], X[2], P[i * 4 + 3]))) for i in range(3)]
    pp = [A.fma(K[i * 3], Xc[0], A.fma(K[i * 3 + 1], Xc[1], A.mul(K[i * 3 + 2], Xc[2]))) for i in range(3)]
    return P, K, kscale, Xc, pp


def pixel_points(X_stored, t, c):
    """(u, v, Xc2, pp2) the kernel computes from its stored X and the tables, as float64 arrays of exact fp32 values, and which rows are
    exact (all of them but for a float64 rounding tie): what the cases plant their targets around."""
    A = IvArith({})
    rows = t["tu"].shape[0]
    _, _, _, Xc, pp = geometry(A, [A.c(np.asarray(X_stored, np.float64)[:, k]) for k in range(3)], t, c)
    dmin = A.c(np.full(rows, c["depth_min"]))
    pz = A.where(pp[2].hi < dmin.lo, dmin, pp[2])
    u, v = A.div(pp[0], pz), A.div(pp[1], pz)
    exact = (u.lo == u.hi) & (v.lo == v.hi) & (Xc[2].lo == Xc[2].hi) & (pp[2].lo == pp[2].hi)
    return u.mid, v.mid, Xc[2].mid, pp[2].mid, exact


def loss_rows(A, s, t, c, X_stored=None):
    """Phase B for the rows of s (four values over rows; s[3] unused without the homogeneous output) and the per-row tables t:
    tu, tv [rows]; A [rows,12]; T [rows,16]; K, Ki [rows,9]; tc [rows,3] or None.
    Returns X (computed), ds (four, in the kernel's scaled units), loss, inl, fgrad and the branch record."""
    rows = t["tu"].shape[0]
    K_ = lambda x: A.c(np.full(rows, x))
    col = lambda a, i: A.c(a[:, i])
    all_rows = np.ones(rows, bool)
    zero, one = K_(0.0), K_(1.0)
    mut = A.mut
    rec = {}
    if c["homog"]:
        bx = A.mul(K_(c["h_beta"]), s[3])
        big = A.gt(bx, K_(20.0), "bx>20", all_rows)
        z = A.exp(A.where(big, zero, bx))                       # (the branch not taken: on a harmless argument)
        sp = A.where(big, s[3], A.div(A.log1p(z), K_(c["h_beta"])))
        hraw = A.add(sp, K_(c["max_inv_scale"]))
        hcl = A.gt(hraw, K_(c["min_inv_scale"]), "hclamped", all_rows)
        hval = A.where(hcl, K_(c["min_inv_scale"]), hraw)
        X = [A.add(A.div(s[k], hval), K_(c["mean"][k])) for k in range(3)]
        rec["bx>20"], rec["hclamped"] = big, hcl
    else:
        X = [A.add(s[k], K_(c["mean"][k])) for k in range(3)]
    Xc_ = X
    if X_stored is not None:                                    # the kernel goes on with the value it stored
        X = [A.c(X_stored[:, k]) for k in range(3)]
    tu, tv = A.c(t["tu"]), A.c(t["tv"])
    P, K, kscale, Xc, pp = geometry(A, X, t, c)
    dmin = K_(c["depth_min"])
    near = A.lt(Xc[2], dmin, "Xc2<depth_min", all_rows)
    hard_live = ~near
    zcl = A.lt(pp[2], dmin, "zclamped", hard_live)
    pz = A.where(zcl, dmin, pp[2])
    u, v = A.div(pp[0], pz), A.div(pp[1], pz)
    du, dv = A.sub(u, tu), A.sub(v, tv)
    e = A.add(A.fabs(du), A.fabs(dv))
    hard = A.gt(e, K_(c["hard_clamp"]), "e>hard_clamp", hard_live)
    far = A.gt(Xc[2], K_(c["depth_max"]), "Xc2>depth_max", hard_live & ~hard)
    invalid = near | hard | far
    rec.update({"Xc2<depth_min": near, "e>hard_clamp": hard & ~near, "Xc2>depth_max": far & ~near & ~hard})
    depth = t.get("tc") is not None
    if depth:
        tc = [col(t["tc"], k) for k in range(3)]
        tavail = A.gt(A.add(A.add(A.fabs(tc[0]), A.fabs(tc[1])), A.fabs(tc[2])), K_(f32(0.00001)), "tavail", all_rows)
        tcd = [A.sub(tc[k], X[k]) for k in range(3)]
        tdist = A.sqrt(A.dot([(tcd[0], tcd[0]), (tcd[1], tcd[1]), (tcd[2], tcd[2])]))
        tfar = A.gt(tdist, K_(f32(0.1)), "tdist>0.1", tavail & ~invalid)
        rec.update({"tavail": tavail, "tdist>0.1": tavail & tfar, "geometry_valid": ~invalid})
        invalid = invalid | (tavail & tfar)
    valid = ~invalid
    rec["zclamped"], rec["zclamped_raw"] = zcl & valid, zcl
    rec["valid"] = valid
    # ---- the valid branch
    wgt = K_(c["wgt"])
    lt = c["loss"]
    if lt in (0, 1):
        th = A.tanh(A.div(e, wgt))
        loss_v = A.mul(wgt, th)
        ge = A.mul_add(A.neg(th), th, one)
    else:
        big_e = A.gt(e, wgt, "e>wgt", valid)
        rec["e>wgt"] = big_e & valid
        es = A.where(big_e, e, one)
        if lt == 2:
            loss_v, ge = A.where(big_e, zero, e), A.where(big_e, zero, one)
        elif lt == 3:
            sq = A.sqrt(A.mul(wgt, es))
            loss_v, ge = A.where(big_e, sq, e), A.where(big_e, A.div(A.scale(wgt, 0.5), sq), one)
        else:
            w1 = A.mul_add(wgt, es, one)
            loss_v, ge = A.where(big_e, A.log(w1), e), A.where(big_e, A.div(wgt, w1), one)
    inl_b = A.lt(e, K_(c["inlier_px"]), "e<inlier", valid)
    rec["e<inlier"] = inl_b & valid
    gu, gv = A.times_sign(ge, A.sgn(du, "sgn(du)", valid)), A.times_sign(ge, A.sgn(dv, "sgn(dv)", valid))
    dp0, dp1 = A.div(gu, pz), A.div(gv, pz)
    dp2 = A.div(A.neg(A.dot([(gu, pp[0]), (gv, pp[1])])), A.mul(pz, pz))
    if "dp2_not_zeroed" not in mut:
        dp2 = A.where(zcl, zero, dp2)
    fgrad = zero
    if c["calib"]:
        fgrad = A.mul(A.mul(A.dot([(dp0, Xc[0]), (dp1, Xc[1])]), K_(c["focal_init"])), kscale)
        fgrad = A.where(valid, fgrad, zero)
    dXc_v = [A.dot([(K[j], dp0), (K[3 + j], dp1), (K[6 + j], dp2)]) for j in range(3)]
    dXs = [zero, zero, zero]
    # ---- the invalid branches
    if depth:
        dXc_i = [zero, zero, zero]
        pos = A.gt(tdist, zero, "tdist>0", invalid & tavail)
        rec["tdist>0"] = pos & invalid & tavail
        rec["tdist==0"] = ~pos & invalid & tavail
        inv = A.where(pos, A.div(one, A.where(pos, A.positive(tdist), one)), zero)
        loss_i = A.where(tavail, tdist, zero)
        dXs = [A.where(invalid & tavail, A.mul(A.neg(tcd[k]), inv, True), zero) for k in range(3)]
    else:
        Ki = [col(t["Ki"], i) for i in range(9)]
        a, b = (tv, tu) if "tu_tv_swapped" in mut else (tu, tv)
        loss_i, dXc_i = zero, []
        for i in range(3):
            d = A.mul_add(K_(c["depth_target"]), A.fma(Ki[i * 3], a, A.fma(Ki[i * 3 + 1], b, Ki[i * 3 + 2])), A.neg(Xc[i]))
            loss_i = A.fabs(d) if i == 0 else A.add(loss_i, A.fabs(d))
            dXc_i.append(A.neg(A.sgn(d, "sgn(d%d)" % i, invalid)))
    loss = A.where(valid, loss_v, loss_i)
    inl = A.where(valid & inl_b, one, zero)
    dXc = [A.where(valid, dXc_v[j], dXc_i[j]) for j in range(3)]
    invB = K_(1.0 if "no_inv_batch" in mut else c["inv_batch"])
    out = {}
    if c.get("pose"):   # d(loss)/dT[k][j] = sum_i A[i][k] dXc[i] Xh[j], k < 3: ak = (three-term product-sum) * invB, then ak * Xh[j] (Xh[3] = 1: ak itself)
        Am = [col(t["A"], i) for i in range(12)]
        out["rd"] = []
        for k in range(3):
            ia = (4 * k, 4 * k + 1, 4 * k + 2) if "rd_A_transposed" in mut else (k, 4 + k, 8 + k)
            ak = A.mul(A.dot([(Am[ia[0]], dXc[0]), (Am[ia[1]], dXc[1]), (Am[ia[2]], dXc[2])]), invB)
            out["rd"] += [A.mul(ak, X[0]), A.mul(ak, X[1]), A.mul(ak, X[2]), ak]
    dX = [A.mul(A.dot([(P[k], dXc[0]), (P[4 + k], dXc[1]), (P[8 + k], dXc[2])], dXs[k]), invB) for k in range(3)]
    fgrad = A.mul(fgrad, invB)
    if c["homog"]:
        ds = [A.div(dX[k], hval) for k in range(3)]
        dh = A.div(A.neg(A.dot([(dX[0], s[0]), (dX[1], s[1]), (dX[2], s[2])])), A.mul(hval, hval))
        if "dh_not_zeroed" not in mut:
            dh = A.where(hcl, zero, dh)
        zz = A.exp(bx) if "sigmoid_when_big" in mut else z
        sig = A.div(A.mul(dh, zz), A.add(zz, one))
        ds.append(sig if "sigmoid_when_big" in mut else A.where(big, dh, sig))
    else:
        ds = dX + [zero]
    if "fc3_row3_kept" in mut and not c["homog"]:
        ds[3] = dX[0]
    if c["f16"]:
        g = c["gscale"] * (c["gscale"] if "grad_scale_twice" in mut else 1.0)
        ds = [A.scale(d, g) for d in ds]
    out.update({"X": Xc_, "ds": ds, "loss": loss, "inl": inl, "fgrad": fgrad, "rec": rec})
    return out


def phase_a_interval(fmt, out16, W3_16, b3, no):
    x, w = fmt.values(out16).numpy(), fmt.values(W3_16).numpy()
    b = np.asarray(b3, np.float64)
    v = x @ w.T + b
    s = 513 * U * (np.abs(x) @ np.abs(w).T + np.abs(b)) + np.abs(v) * EPS64
    zero = np.zeros(x.shape[0])
    return [Iv(v[:, j] - s[:, j], v[:, j] + s[:, j]) if j < no else Iv(zero) for j in range(4)]


def phase_a_f32(A, fmt, out16, W3_16, b3, no):
    x = fmt.values(out16).numpy().astype(np.float32).reshape(-1, 64, 8)
    w = fmt.values(W3_16).numpy().astype(np.float32).reshape(no, 64, 8)
    out = []
    for j in range(4):
        if j >= no:
            out.append(np.zeros(x.shape[0], np.float32))
            continue
        acc = np.zeros(x.shape[:2], np.float32)
        for e in range(8):
            acc = A.fma(x[:, :, e], np.broadcast_to(w[j, :, e], acc.shape), acc)
        out.append(ordered_sums.wave_sums(acc[:, :, None])[:, 0] + np.float32(b3[j]))
    return out


def phase_c(A, ds, x, w3, no):
    """d [rows,512] before the mask and the rounding: the FMA chain over the fc3 rows, from 0."""
    shape = x.shape
    d = A.c(np.zeros(shape))
    for j in range(no):
        if A.interval:
            dsb = Iv(np.broadcast_to(ds[j].lo[:, None], shape), np.broadcast_to(ds[j].hi[:, None], shape))
        else:
            dsb = np.broadcast_to(ds[j][:, None], shape)
        d = A.fma(dsb, A.c(np.broadcast_to(w3[j][None, :], shape)), d)
    return d


def block_sum(A, vals, n):
    """Sequential sums in row order over the rows below n of every 16-row block: [blocks, ...]; the first row starts the sum (0 + x = x)."""
    nblk = (n + BLOCK - 1) // BLOCK
    take = (lambda i: Iv(vals.lo[i], vals.hi[i])) if A.interval else (lambda i: vals[i])
    acc = take(np.arange(nblk) * BLOCK)
    for r in range(1, BLOCK):
        idx = np.arange(nblk) * BLOCK + r
        acc = A.where(idx < n, A.add(acc, take(np.minimum(idx, n - 1))), acc)
    return acc


def block_fma_sum(A, ds, x, n):
    """[blocks,512]: gw = fma(ds[r], x[r], gw) over the rows below n of every 16-row block in row order, from 0."""
    nblk = (n + BLOCK - 1) // BLOCK
    acc = A.c(np.zeros((nblk, 512)))
    for r in range(BLOCK):
        idx = np.arange(nblk) * BLOCK + r
        i = np.minimum(idx, n - 1)
        if A.interval:
            dsb = Iv(np.broadcast_to(ds.lo[i][:, None], (nblk, 512)), np.broadcast_to(ds.hi[i][:, None], (nblk, 512)))
        else:
            dsb = np.broadcast_to(ds[i][:, None], (nblk, 512))
        acc = A.where((idx < n)[:, None], A.fma(dsb, A.c(x[i]), acc), acc)
    return acc


# ------------------------------------------------------------------------------------------------ the float32 stand-in of the kernel
def bias_partials_from(fmt, dZ16, n, unrounded=None):
    """bias_partials[L - 1] bit for bit: the stored dZ rows below n, summed in fp32 in row order from 0 per 16-row block."""
    z = fmt.values(dZ16).numpy().astype(np.float32) if unrounded is None else unrounded
    nblk = (n + BLOCK - 1) // BLOCK
    out = np.zeros((nblk, 512), np.float32)
    with np.errstate(invalid="ignore"):
        for b in range(nblk):
            for r in range(b * BLOCK, min(n, b * BLOCK + BLOCK)):
                out[b] = out[b] + z[r]
    return out


def truncate16(fmt, x32):
    bits = np.ascontiguousarray(x32, np.float32).view(np.uint32)
    if fmt.name == "bf16":
        return (bits & np.uint32(0xFFFF0000)).view(np.float32)
    with np.errstate(over="ignore"):
        h = x32.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x32)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float32)


def stand_in_X(fmt, act16, W3_16, b3, c, no):
    """The stand-in's scene coordinates alone (they depend on the activations and fc3 only): what the CPU tests plant around."""
    A = F32Arith(False)
    rows = act16.shape[0]
    eye = lambda k, m: np.tile(np.eye(k, m).reshape(1, -1), (rows, 1))
    t = dict(A=eye(3, 4), T=eye(4, 4), K=eye(3, 3), Ki=eye(3, 3), tu=np.zeros(rows), tv=np.zeros(rows), tc=None)
    with np.errstate(all="ignore"):
        o = loss_rows(A, phase_a_f32(A, fmt, act16, W3_16, b3, no), t, dict(c, calib=False))
    return np.stack([np.asarray(v, np.float32) for v in o["X"]], 1)


def stand_in(fmt, act16, W3_16, b3, tabs, c, n, no, contract, mut=(), stale=None):
    """loss_body in numpy float32 for the first n rows of act16 [>= n (+ 1 for the row-past-n mutant), 512]. tabs: the per-row tables of
    at least as many rows. stale: (bias_partials, fc3_partials, stat_partials) of an earlier, larger batch -- what the slots past this
    batch's blocks hold. Returns the observables of a capture (see `judge`)."""
    mut = frozenset(mut)
    A = F32Arith(contract, mut)
    m = n + 1 if "row_past_n" in mut else n
    sub = {k: (None if v is None else np.asarray(v)[:m]) for k, v in tabs.items()}
    s = phase_a_f32(A, fmt, act16[:m], W3_16, b3, no)
    with np.errstate(all="ignore"):
        o = loss_rows(A, s, sub, c)
    x = fmt.values(act16[:m]).numpy().astype(np.float32)
    w3 = fmt.values(W3_16).numpy().astype(np.float32)
    ds = [np.asarray(d, np.float32) for d in o["ds"]]
    w3c, noc = w3, no
    if "fc3_row3_kept" in mut and no == 3:     # the kernel's fourth row aliases row 0 (`j < no ? j : 0`) and is zeroed after the load
        w3c, noc = np.concatenate([w3, w3[:1]]), 4
    with np.errstate(all="ignore"):
        d = phase_c(A, ds, x, w3c, noc)
    d = np.where((d > 0) if "mask_from_d" in mut else (x > 0), d, np.float32(0))
    r = truncate16(fmt, d) if "truncate16" in mut else fmt.round(torch.from_numpy(np.ascontiguousarray(d))).numpy()
    dZ16 = fmt.bits(torch.from_numpy(np.ascontiguousarray(r)))
    nblk = (n + BLOCK - 1) // BLOCK
    bias = bias_partials_from(fmt, dZ16, m, unrounded=d if "bias_unrounded" in mut else None)[:nblk]
    stride = (no * 513 + 3) & ~3
    fc3 = np.zeros((nblk, stride), np.float32)
    with np.errstate(all="ignore"):
        for j in range(no):
            fc3[:, j * 512:(j + 1) * 512] = block_fma_sum(A, ds[j], x, m)[:nblk]
            fc3[:, no * 512 + j] = block_sum(A, ds[j], m)[:nblk]
        stat = np.zeros((nblk, 4), np.float32)
        for k, name in enumerate(("loss", "inl", "fgrad")):
            stat[:, k] = block_sum(A, np.asarray(o[name], np.float32), m)[:nblk]
    if stale is not None:                      # the slots past this batch's blocks keep the earlier batch's values
        bias = np.concatenate([bias, stale[0][nblk:]])
        fc3 = np.concatenate([fc3, stale[1][nblk:]])
        stat = np.concatenate([stat, stale[2][nblk:]])
    inv = 1.0 / c["gscale"] if c["f16"] else 1.0
    extra = 1 if "block_past_end" in mut else 0
    swap = (0, 1) if "blocks_swapped" in mut else None
    return dict(X=np.stack([np.asarray(v, np.float32) for v in o["X"]], 1)[:n], dZ=dZ16[:n], bias_partials=bias, fc3_partials=fc3,
                stat_partials=stat, grad_fc3=ordered_sums.lane_strided_totals(fc3[:, :no * 513], nblk, inv, swap, extra),
                grad_stats=ordered_sums.lane_strided_totals(stat[:, :3], nblk, None, swap, extra), rec=o["rec"],
                **({"row_dT": np.stack([np.asarray(v, np.float32) for v in o["rd"]], 1)[:n]} if "rd" in o else {}))


# ------------------------------------------------------------------------------------------------ the judgement
def _hull(a, b):
    return Iv(np.minimum(a.lo, b.lo), np.maximum(a.hi, b.hi))


def rows_interval(s, tabs, c, X_stored, ulps, max_leaves=4096, points=True, zero_width=False):
    """loss_rows in intervals for all rows; the rows with an undecided comparison are walked over every feasible side and carry the hull.
    Returns (outputs, undecided [rows] bool)."""
    A = IvArith(ulps, points=points, zero_width=zero_width)
    o = loss_rows(A, s, tabs, c, X_stored)
    keys = [k for k in ("X", "ds", "rd") if k in o]
    for k in keys:
        o[k] = [_own(v) for v in o[k]]
    for k in ("loss", "inl", "fgrad"):
        o[k] = _own(o[k])
    und = np.zeros(tabs["tu"].shape[0], bool)
    for m in A.undecided.values():
        und |= m
    for r in np.nonzero(und)[0]:
        sl = slice(r, r + 1)
        s1 = [v[sl] for v in s]
        t1 = {k: (None if v is None else v[sl]) for k, v in tabs.items()}
        stack, leaves = [{}], []
        while stack:
            forced = stack.pop()
            B = IvArith(ulps, forced, points, zero_width)
            o1 = loss_rows(B, s1, t1, c, None if X_stored is None else X_stored[sl])
            new = [k for k, m in B.undecided.items() if bool(m[0]) and k not in forced]
            if new:
                stack += [dict(forced, **{new[0]: v}) for v in B.options[new[0]]]
            else:
                leaves.append(o1)
            assert len(leaves) + len(stack) <= max_leaves, "row %d: too many undecided comparisons" % r
        for k in keys:
            for j in range(len(o[k])):
                h = leaves[0][k][j]
                for lf in leaves[1:]:
                    h = _hull(h, lf[k][j])
                o[k][j].lo[r], o[k][j].hi[r] = h.lo[0], h.hi[0]
        for k in ("loss", "inl", "fgrad"):
            h = leaves[0][k]
            for lf in leaves[1:]:
                h = _hull(h, lf[k])
            o[k].lo[r], o[k].hi[r] = h.lo[0], h.hi[0]
    return o, und


class Verdict:
    def __init__(self):
        self.items = {}          # name -> [total, bad, worst ratio, first]

    def add(self, name, bad, ratio=None, describe=None):
        bad = np.asarray(bad)
        it = self.items.setdefault(name, [0, 0, 0.0, None])
        it[0] += bad.size
        it[1] += int(bad.sum())
        if ratio is not None and np.size(ratio):
            it[2] = max(it[2], float(np.max(np.where(np.isfinite(ratio), ratio, 0.0))))
        if bad.any() and it[3] is None:
            i = np.unravel_index(int(np.argmax(bad)), bad.shape)
            it[3] = describe(i) if describe else str(i)

    def failed(self):
        return {k: v for k, v in self.items.items() if v[1]}

    def lines(self, what):
        return ["LOSS-STAGE %s %s: %d elements, %d outside, worst |got - mid| / halfwidth = %.4f%s" % (what, k, v[0], v[1], v[2], "; first: %s" % v[3] if v[1] else "")
                for k, v in self.items.items()]


def _ratio(got, iv):
    rad = iv.rad
    with np.errstate(all="ignore"):
        return np.where(rad > 0, np.abs(got - iv.mid) / np.where(rad > 0, rad, 1.0), np.where(got == iv.mid, 0.0, np.inf))


def _own(iv):
    return Iv(np.array(iv.lo, np.float64), np.array(iv.hi, np.float64))


def judge(fmt, cap, tabs, c, n, no, ulps=None):
    """cap: out16 [n,512], W3 uint16 [no,512], b3, X [n,3], dZ uint16 [n,512], bias_partials / fc3_partials / stat_partials (>= nblk rows),
    grad_fc3 [no * 513], grad_stats [3]. Returns (Verdict, undecided [n] bool, the interval outputs of phase B)."""
    ulps = ulps or math_ulps()
    V = Verdict()
    nblk = (n + BLOCK - 1) // BLOCK
    sub = {k: (None if v is None else np.asarray(v, np.float64)[:n]) for k, v in tabs.items()}
    s = phase_a_interval(fmt, cap["out16"][:n], cap["W3"], cap["b3"], no)
    X = np.asarray(cap["X"], np.float32)[:n]
    assert np.isfinite(X).all(), "a stored scene coordinate is not finite"
    o, und = rows_interval(s, sub, c, X.astype(np.float64), ulps)
    Xi = Iv(np.stack([v.lo for v in o["X"]], 1), np.stack([v.hi for v in o["X"]], 1))
    V.add("X", ~Xi.contains(X), _ratio(X, Xi), lambda i: "row %d, coordinate %d: got %r, [%r, %r]" % (i[0], i[1], float(X[i]), float(Xi.lo[i]), float(Xi.hi[i])))
    if "rd" in o:    # the pose gradient rows (a pose configuration) and the image each row belongs to
        rd = Iv(np.stack([v.lo for v in o["rd"]], 1), np.stack([v.hi for v in o["rd"]], 1))
        g = np.asarray(cap["row_dT"], np.float32)[:n].astype(np.float64)
        V.add("row_dT", ~rd.contains(g), _ratio(g, rd), lambda i: "row %d, entry %d: got %r, [%r, %r]" % (i[0], i[1], g[i], rd.lo[i], rd.hi[i]))
        if cap.get("row_image") is not None:
            V.add("row_image", np.asarray(cap["row_image"])[:n] != np.asarray(cap["row_image_want"])[:n], None, lambda i: "row %d" % i[0])
    # ---- phase C: dZ
    A = IvArith(ulps)
    x = fmt.values(cap["out16"][:n]).numpy()
    w3 = fmt.values(cap["W3"]).numpy()
    d = phase_c(A, o["ds"], x, w3, no)
    r16 = lambda a: fmt.round(torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32)).numpy().astype(np.float64)
    with np.errstate(over="ignore"):
        lo16, hi16 = r16(d.lo), r16(d.hi)
    got = fmt.values(cap["dZ"][:n]).numpy()
    mask = x > 0
    bad = np.where(mask, ~((lo16 <= got) & (got <= hi16)), np.asarray(cap["dZ"][:n]) != 0)
    V.add("dZ", bad, np.where(mask, _ratio(got, Iv(np.minimum(lo16, d.lo), np.maximum(hi16, d.hi))), 0.0),
          lambda i: "row %d, channel %d: got %r, [%r, %r], mask %d" % (i[0], i[1], float(got[i]), float(lo16[i]), float(hi16[i]), int(mask[i])))
    # ---- bias partials, bit for bit from the stored rows
    want = bias_partials_from(fmt, cap["dZ"], n)
    gotb = np.asarray(cap["bias_partials"], np.float32)[:nblk]
    V.add("bias_partials_bits", (want.view(np.uint32) != gotb.view(np.uint32)) & ~(np.isnan(want) & np.isnan(gotb)), None,   # (fp16: inf - inf)
          lambda i: "block %d, channel %d: got %r, the ordered sum of the stored rows is %r" % (i[0], i[1], float(gotb[i]), float(want[i])))
    # ---- fc3 partials
    fc3 = np.asarray(cap["fc3_partials"], np.float32)
    for j in range(no):
        iv, g = block_fma_sum(A, o["ds"][j], x, n), fc3[:nblk, j * 512:(j + 1) * 512].astype(np.float64)
        V.add("fc3_weight_partials", ~iv.contains(g), _ratio(g, iv), lambda i, j=j, g=g, iv=iv: "fc3 row %d, block %d, channel %d: got %r, [%r, %r]" % (j, i[0], i[1], g[i], iv.lo[i], iv.hi[i]))
        iv, g = block_sum(A, o["ds"][j], n), fc3[:nblk, no * 512 + j].astype(np.float64)
        V.add("fc3_bias_partials", ~iv.contains(g), _ratio(g, iv), lambda i, j=j, g=g, iv=iv: "fc3 bias %d, block %d: got %r, [%r, %r]" % (j, i[0], g[i], iv.lo[i], iv.hi[i]))
        if n % BLOCK == 1:     # the last block is one row: its partial IS that row's ds
            last = o["ds"][j][n - 1]
            assert float(iv.lo[-1]) == float(last.lo) and float(iv.hi[-1]) == float(last.hi)
            V.add("one_row_block", np.array([not (last.lo <= g[-1] <= last.hi)]), None, lambda i, j=j, g=g: "ds[%d] of row %d: got %r" % (j, n - 1, g[-1]))
    # ---- statistics partials (the inlier count: exact sums of exact flags)
    stat = np.asarray(cap["stat_partials"], np.float32)
    for k, name in enumerate(("loss", "inl", "fgrad")):
        if name == "inl":
            lo = np.array([o["inl"].lo[b * BLOCK:min(n, b * BLOCK + BLOCK)].sum() for b in range(nblk)])
            hi = np.array([o["inl"].hi[b * BLOCK:min(n, b * BLOCK + BLOCK)].sum() for b in range(nblk)])
            iv = Iv(lo, hi)
        else:
            iv = block_sum(A, o[name], n)
        g = stat[:nblk, k].astype(np.float64)
        V.add("stat_partials_" + name, ~iv.contains(g), _ratio(g, iv), lambda i, g=g, iv=iv, name=name: "%s, block %d: got %r, [%r, %r]" % (name, i[0], g[i], iv.lo[i], iv.hi[i]))
        if n % BLOCK == 1:
            last = o[name][n - 1]
            V.add("one_row_block", np.array([not (last.lo <= g[-1] <= last.hi)]), None, lambda i, g=g, name=name: "%s of row %d: got %r" % (name, n - 1, g[-1]))
    # ---- tr.grad, bit for bit from the partials that were read
    inv = 1.0 / c["gscale"] if c["f16"] else 1.0
    want = ordered_sums.lane_strided_totals(fc3[:, :no * 513], nblk, inv)
    gotg = np.asarray(cap["grad_fc3"], np.float32)
    V.add("grad_fc3_bits", want.view(np.uint32) != gotg.view(np.uint32), None, lambda i: "fc3 entry %d: got %r, the ordered sum of the partials is %r" % (i[0], float(gotg[i]), float(want[i])))
    wants = ordered_sums.lane_strided_totals(stat[:, :3], nblk)
    gots = np.asarray(cap["grad_stats"], np.float32)[:3]
    V.add("grad_stats_bits", wants.view(np.uint32) != gots.view(np.uint32), None, lambda i: "statistic %d: got %r, the ordered sum of the partials is %r" % (i[0], float(gots[i]), float(wants[i])))
    if cap.get("state_loss") is not None:     # head_sched.h sched_post_wave: loss = g0 * inv_global_batch in fp32
        ig = np.float32(1.0) / np.float32(cap["global_batch"])
        V.add("state_bits", np.array([np.float32(cap["state_loss"]) != gots[0] * ig, np.float32(cap["state_inliers"]) != gots[1] * ig]), None,
              lambda i: "state()['%s']: got %r" % (("loss", "batch_inliers")[i[0]], (cap["state_loss"], cap["state_inliers"])[i[0]]))
    return V, und, o


# ------------------------------------------------------------------------------------------------ the forward pass once more, for autograd
def forward_torch(s, tabs, c, rec, X_point):
    """Sum over the rows of loss * inv_batch, from s [rows,4] (float64, requires grad), on the branches `rec` records. torch float64.
    X_point [rows,3]: where the restatement continued from the stored X, the difference stored - computed is carried as a constant."""
    T = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    if c["homog"]:
        bx = c["h_beta"] * s[:, 3]
        big, hcl = torch.as_tensor(rec["bx>20"]), torch.as_tensor(rec["hclamped"])
        sp = torch.where(big, s[:, 3], torch.log1p(torch.exp(torch.where(big, torch.zeros_like(bx), bx))) / c["h_beta"])
        h = torch.where(hcl, torch.full_like(sp, c["min_inv_scale"]), sp + c["max_inv_scale"])
        X = s[:, :3] / h[:, None] + T(c["mean"])
    else:
        X = s[:, :3] + T(c["mean"])
    X = X + (T(X_point) - X.detach())
    rows = X.shape[0]
    Am, Tm, K = T(tabs["A"]).view(rows, 3, 4), T(tabs["T"]).view(rows, 4, 4), T(tabs["K"]).view(rows, 3, 3).clone()
    if c["calib"]:
        f = (1.0 + c["calib_g"]) * c["focal_init"] * (K[:, 0, 0] / c["focal_init"])
        K[:, 0, 0], K[:, 1, 1], K[:, 0, 1], K[:, 1, 0] = f, f, 0.0, 0.0
    P = torch.bmm(Am, Tm)
    Xc = torch.bmm(P, torch.cat([X, torch.ones(rows, 1, dtype=torch.float64)], 1)[:, :, None])[:, :, 0]
    pp = torch.bmm(K, Xc[:, :, None])[:, :, 0]
    pz = torch.where(torch.as_tensor(rec["zclamped_raw"]), torch.full_like(pp[:, 2], c["depth_min"]), pp[:, 2])
    e = (pp[:, 0] / pz - T(tabs["tu"])).abs() + (pp[:, 1] / pz - T(tabs["tv"])).abs()
    w = c["wgt"]
    big_e = torch.as_tensor(rec.get("e>wgt", np.zeros(rows, bool)))
    es = torch.where(big_e, e, torch.ones_like(e))
    if c["loss"] in (0, 1):
        lv = w * torch.tanh(e / w)
    elif c["loss"] == 2:
        lv = torch.where(big_e, torch.zeros_like(e), e)
    elif c["loss"] == 3:
        lv = torch.where(big_e, torch.sqrt(w * es), e)
    else:
        lv = torch.where(big_e, torch.log(1 + w * es), e)
    if tabs.get("tc") is not None:
        tcd = T(tabs["tc"]) - X
        pos = torch.as_tensor(rec["tdist>0"])
        tdist = torch.sqrt(torch.where(pos[:, None], tcd, torch.ones_like(tcd)).pow(2).sum(1))
        li = torch.where(pos, tdist, torch.zeros_like(tdist))
    else:
        px = torch.stack([T(tabs["tu"]), T(tabs["tv"]), torch.ones(rows, dtype=torch.float64)], 1)
        tgt = c["depth_target"] * torch.bmm(T(tabs["Ki"]).view(rows, 3, 3), px[:, :, None])[:, :, 0]
        li = (tgt - Xc).abs().sum(1)
    return (torch.where(torch.as_tensor(rec["valid"]), lv, li) * c["inv_batch"]).sum()
