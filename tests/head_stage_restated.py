"""fp64 restatement of ONE 512 x 512 stage of the head's training step at a time, judged per element by an interval criterion.

Every stage is restated from the operands the kernel itself read: the trainer's 16-bit weight copies, the fp32 biases, and the buffers
HeadTrainer.debug_read returns ('out', 'R', 'mask', 'dZ', 'slab', 'bias_partials') plus tr.grad after backward(). Nothing comes from
the oracle's forward pass, so a rounding flip in one stage cannot leak into the judgement of the next. Which buffer feeds which layer is
oracle/head_oracle.py's forward() / backward() (the same tables as head_api.hip forward_layers, dgrad_layers, fill_wgrad_args).

The criterion. For one output element let v be the fp64 value of the sum the kernel forms (K products, plus the bias, plus the residual
gradient where there is one) and A the sum of the absolute values of the same terms. An fp32 accumulation of T terms in ANY order is off
by at most

    s = T * 2^-23 * A.

The textbook constant is 2^-24 per addition (gamma_T ~ T u); it is doubled to allow for alignment inside the matrix instruction that is
not round-to-nearest. The factor 2 is a SUPPOSITION about the matrix unit, not a documented property. (The fp64 restatement's own error,
about T * 2^-53 * A, is eight orders of magnitude below s and is not accounted for.)

In A, a non-zero SUBNORMAL 16-bit operand of a matrix instruction counts with the magnitude of the format's smallest normal number
(Fmt.tiny: 2^-14 in fp16; no bf16 value here comes near 2^-126). Derivation: the matrix instruction (E::mfma16 / E::mfma32,
gemm_common.h) aligns the products of one dot-product step to the largest sum of their operands' EXPONENT FIELDS and drops, toward zero,
what lies 24 bits below it. A subnormal carries the exponent field of the smallest normal, so its product is aligned -- and truncated --
as if the operand had that magnitude, however small it really is: the error of the step is relative to the nominal magnitudes, and so
must A be. Seen on an MI355X in the fp16 weight-gradient slabs, in elements all of whose terms have a subnormal gradient operand: two
terms, -106 * 2^-24 x 638 * 2^-24 (both subnormal) and 13 * 2^-24 x 1036 * 2^-17, nominal exponents -28 and -21, came out 2^-46 above
their exact sum -- the first product cut to a multiple of 2^(-21 - 24). Without the rule the plain bound was missed by up to 6.7 s in 1
to 73 of 262144 elements of a slab (fp16, n = 64, 80, 128, 400); with it the worst of those is 0.08 s, and for an element without
subnormal operands nothing changes (the median growth of s in those slabs is 0.2 - 0.5 %). The truncation toward zero also confirms that
the factor 2 above is needed.

  * 16-bit outputs ('out', 'R', 'dZ'): the kernel's fp32 value u lies in [v - s, v + s] and is an fp32 number, so it lies in
    [RN32(v - s), RN32(v + s)]; every map f from u to the stored pattern (ReLU, round to 16 bits, add the residual stream in fp32, round
    again) is monotone, so an element passes iff  f(RN32(v - s)) <= got <= f(RN32(v + s))  in the format's value order. No "within k ulp",
    no relative error: ties and values near zero are handled by construction. round16 is torch's bf16 / fp16 round-to-nearest-even, as in
    oracle/head_oracle.py.
  * fp32 outputs ('slab', 'bias_partials', tr.grad): |got - v| <= s, with one more 2^-24 |partial sum| per further fp32 addition on the
    way to tr.grad (the derivations stand next to the bounds below).
  * mask bits of the layers whose activation is not kept (l % 3 == 2, l < L - 2): the bit the kernel stores is `stored 16-bit value > 0`
    (head_kernels.hip rowgemm80_body, "A 16-bit output is > 0 iff it is non-zero"), a monotone map of u like the others: the bit must lie
    between round16(relu(v - s)) > 0 and round16(relu(v + s)) > 0. Where those two differ -- [v - s, v + s] straddles zero, or, in fp16,
    the point below which a positive value rounds to zero -- either bit is accepted. These are the ONLY left-out cases; their share is
    reported per layer and capped at MASK_LEFT_OUT_CAP by the tests.
  * the unmasked residual gradient dR has no debug_read kind: where the mask bit is 1 it IS the stored dZ, elsewhere it is carried as
    the interval [round16(v_lo - s), round16(v_hi + s)] of the stage that produced it, and the consuming stage's v becomes an interval.

Out of scope here: fc3, the loss with all its branches and the production of dZ[L - 1] with the fc3 / bias / statistics partials, which
tests/loss_stage_restated.py judges per row and per element (tests/test_loss_stage_gpu.py); the optimiser, pinned bit for bit by
tests/test_adamw_exact_gpu.py; the pose network behind the loss kernel's pose gradient rows, which stays on the vector-norm bounds of
tests/test_head_gpu.py. dZ[L - 1] is an OPERAND here (of dZ[L - 2], of the last layer's weight and bias gradients), never an output.
"""
import numpy as np
import torch

LAYER = 512 * 512 + 512          # floats of one wide layer (weight + bias) in the flat parameter / gradient / slab vectors
UNIT = 2.0 ** -23                # per term (see above)
ADD = 2.0 ** -24                 # one further fp32 addition, relative to the magnitude of its result
MASK_LEFT_OUT_CAP = 1e-3         # share of a layer's mask bits that may be undecided


def decode_mask_bits(words, n):
    """[row tiles, 2048] uint32 words of a layer (RowGemmArgs::mask_out) -> bool [n, 512]: lane-private layout of rowgemm80's accumulators."""
    mt_n = words.shape[0]
    w4 = words.reshape(mt_n, 4, 4, 64, 2)                     # [row tile][column tile][wave][lane][x | y]
    out = np.zeros((mt_n * 80, 512), bool)
    lane = np.arange(64)
    fr, fq = lane & 15, lane >> 4
    for j in range(5):
        for i in range(2):
            f = 2 * j + i
            for nt in range(4):
                for w in range(4):
                    rows = (np.arange(mt_n)[:, None] * 80 + j * 16 + fr[None, :])              # [mt, lane]
                    col0 = nt * 128 + w * 32 + i * 16 + 4 * fq                                 # [lane]
                    for word, cbase in ((0, 0), (1, 2)):
                        v = w4[:, nt, w, :, word]
                        out[rows, (col0 + cbase)[None, :]] = (v >> (9 - f)) & 1
                        out[rows, (col0 + cbase + 1)[None, :]] = (v >> (25 - f)) & 1
    return out[:n]


class Fmt:
    """A 16-bit operand format: bit patterns <-> values, round-to-nearest-even from fp32."""

    def __init__(self, name):
        assert name in ("bf16", "fp16")
        self.name = name
        self.dt = torch.bfloat16 if name == "bf16" else torch.float16
        self.tiny = 2.0 ** -126 if name == "bf16" else 2.0 ** -14      # the smallest normal number

    def nominal(self, x):
        """|x| as the matrix instruction aligns it: a non-zero subnormal has the exponent field of the smallest normal (module docstring)."""
        a = x.abs()
        return torch.where((a > 0) & (a < self.tiny), torch.full_like(a, self.tiny), a)

    def values(self, bits):
        """uint16 patterns -> float64 tensor (exact)."""
        return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(self.dt).to(torch.float64)

    def round(self, x32):
        assert x32.dtype == torch.float32
        return x32.to(self.dt).to(torch.float32)

    def bits(self, x32):
        """fp32 values that are representable -> uint16 patterns."""
        return x32.to(self.dt).view(torch.int16).numpy().view(np.uint16).copy()


def structure(nb):
    """The layer tables. forward: (layer, input, residual stream index or None) with input ('R', b) / ('out', l); dgrad: (layer whose
    weights multiply, layer whose dZ is produced, adds dR, emits dR); ins[l]: the weight-gradient operand of layer l."""
    L = 3 * nb + 5
    f1 = 3 * (nb + 1)
    fwd, ins = [], [None] * L
    for b in range(nb + 1):
        fwd += [(3 * b, ("R", b), None), (3 * b + 1, ("out", 3 * b), None), (3 * b + 2, ("out", 3 * b + 1), b)]
    fwd += [(f1, ("R", nb + 1), None), (f1 + 1, ("out", f1), None)]
    for l, src, _ in fwd:
        ins[l] = src
    dgrad = [(f1 + 1, f1, False, False), (f1, 3 * nb + 2, False, True)]
    for b in range(nb, -1, -1):
        dgrad += [(3 * b + 2, 3 * b + 1, False, False), (3 * b + 1, 3 * b, False, False)]
        if b > 0:
            dgrad.append((3 * b, 3 * (b - 1) + 2, True, True))
    return L, fwd, dgrad, ins


def unkept(l, L):
    """A block's last activation is not stored by a training forward: only its mask bits and its sum with the residual stream are."""
    return l % 3 == 2 and l < L - 2


def slab_rows(n, nslabs, slab):
    """Rows [mb, me) of a split-K slab (head_wgrad.h wgrad_kloop: rows_per_slab is rounded up to whole 64-row stages)."""
    rps = (n + nslabs * 64 - 1) // (nslabs * 64) * 64
    mb = slab * rps
    return mb, max(mb, min(n, mb + rps))


def n_slabs(L):
    """head_api.hip acez_trainer_create: as many row slabs as fill 256 workgroups with 16 tiles per layer."""
    return max(1, 256 // (16 * L))


class Capture:
    """What one backward() call left behind, as the kernels stored it.
    fmt, nb, n, nslabs, inv_grad_scale; w16 uint16 [L,512,512] ([out][in]); bias float32 [L,512]; out {l: uint16 [n,512]} (kept layers);
    R [nb + 2] uint16 [n,512]; mask {l: bool [n,512]} for l < L - 1; dZ [L] uint16 [n,512]; slabs float32 [nslabs, L * LAYER];
    bias_partials {l: float32 [row tiles,512]} for l < L - 1; grad float32 [>= L * LAYER]."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._w = {}

    def W(self, l):
        if l not in self._w:
            self._w[l] = self.fmt.values(self.w16[l])
        return self._w[l]

    def src(self, s):
        kind, i = s
        return self.fmt.values(self.R[i] if kind == "R" else self.out[i])

    def copy(self):
        c = Capture(**{k: v for k, v in self.__dict__.items() if k != "_w"})
        for k in ("out", "mask", "bias_partials"):
            setattr(c, k, {i: a.copy() for i, a in getattr(self, k).items()})
        for k in ("R", "dZ"):
            setattr(c, k, [a.copy() for a in getattr(self, k)])
        c.slabs, c.grad = self.slabs.copy(), self.grad.copy()
        return c


def capture_trainer(tr, n, w16, params, grad_scale):
    """Read everything the checks need from a HeadTrainer whose last call was backward() on n rows. w16: int32 [L,131072] (the export
    of the 16-bit copies, helpers.trainer_snapshot), params: the fp32 masters, grad_scale: state()['grad_scale'] read BEFORE the backward
    call (the schedule wave that changes it runs with the update)."""
    L, nb = tr.L, tr.nb
    tiles = (n + 79) // 80
    ns = n_slabs(L)
    p = np.asarray(params, np.float32)
    return Capture(
        fmt=Fmt(tr.dtype), nb=nb, n=n, nslabs=ns, inv_grad_scale=1.0 / float(grad_scale),
        w16=np.ascontiguousarray(w16).view(np.uint16).reshape(L, 512, 512),
        bias=np.stack([p[l * LAYER + 262144:(l + 1) * LAYER] for l in range(L)]),
        out={l: tr.debug_read("out", l, n) for l in range(L) if not unkept(l, L)},
        R=[tr.debug_read("R", b, n) for b in range(nb + 2)],
        mask={l: decode_mask_bits(tr.debug_read("mask", l, n), n) for l in range(L - 1)},
        dZ=[tr.debug_read("dZ", l, n) for l in range(L)],
        slabs=np.stack([tr.debug_read("slab", s, n) for s in range(ns)]),
        bias_partials={l: tr.debug_read("bias_partials", l, tiles) for l in range(L - 1)},
        grad=tr.grad.detach().cpu().numpy().copy())


class Result:
    """One stage of one layer: how many elements were judged, how many fell outside, how many were left out (mask bits only), and for the
    record `worst` (fp32 stages: the largest |got - v| / s) or `flips` (16-bit stages: elements whose pattern is not round16(f(v)), i.e.
    where the accumulation error moved the value across a rounding boundary -- allowed inside the interval)."""

    def __init__(self, stage, layer, total, bad, first, left_out=0, worst=None, flips=None):
        self.stage, self.layer, self.total, self.bad, self.first = stage, layer, int(total), int(bad), first
        self.left_out, self.worst, self.flips = int(left_out), worst, flips

    def __str__(self):
        s = f"{self.stage}[{self.layer}]: {self.bad} of {self.total} elements outside their bounds"
        if self.left_out:
            s += f", {self.left_out} left out"
        if self.worst is not None:
            s += f", worst |got - v| / s = {self.worst:.4f}"
        if self.flips is not None:
            s += f", {self.flips} rounding flips"
        return s + (f"; first: {self.first}" if self.bad else "")


def _first(bad, describe):
    if not bool(bad.any()):
        return None
    i, j = np.unravel_index(int(torch.argmax(bad.reshape(-1).to(torch.uint8))), tuple(bad.shape))
    return describe(int(i), int(j))


def _rowcol(stage, l, got, lo, hi):
    return lambda r, c: (f"{stage} layer {l} (row {r}, column {c}), row tile {r // 80}, column tile {c // 128}: got {float(got[r, c])!r}, "
                         f"lo {float(lo[r, c])!r}, hi {float(hi[r, c])!r}")


def _product(fmt, X, W_t):
    """v = X @ W_t in fp64, and A = the same sum over the nominal magnitudes of the operands."""
    return X @ W_t, fmt.nominal(X) @ fmt.nominal(W_t)


def forward_value(cap, l, src):
    """(v, s) of forward layer l: out[src] @ W[l]^T + b[l]; T = 512 products + the bias."""
    b = torch.from_numpy(cap.bias[l]).to(torch.float64)
    v, A = _product(cap.fmt, cap.src(src), cap.W(l).t())
    return v + b, 513 * UNIT * (A + b.abs())


def check_forward(cap):
    """'out' of every kept layer, every residual stream 'R', and the mask bits: of a kept layer exactly `stored activation > 0`, of an
    unkept layer by the interval of its recomputed pre-activation."""
    fmt = cap.fmt
    L, fwd, _, _ = structure(cap.nb)
    res = []
    for l, src, rb in fwd:
        v, s = forward_value(cap, l, src)
        lo32, hi32, pt32 = (v - s).to(torch.float32), (v + s).to(torch.float32), v.to(torch.float32)
        act = lambda x: fmt.round(torch.relu(x))      # rowgemm80_body: v += bias; fmaxf(v, 0); pk4
        if rb is None:
            got = fmt.values(cap.out[l]).to(torch.float32)
            lo, hi, pt = act(lo32), act(hi32), act(pt32)
            name, idx = "out", l
        else:
            # AUX_RESIDUAL: the ROUNDED activation and the residual stream are added in fp32 and rounded again (rowgemm80_body: un4(y), un4(rb), pk4)
            r32 = fmt.values(cap.R[rb]).to(torch.float32)
            f = lambda x: fmt.round(act(x) + r32)
            got = fmt.values(cap.R[rb + 1]).to(torch.float32)
            lo, hi, pt = f(lo32), f(hi32), f(pt32)
            name, idx = "R", rb + 1
        bad = ~((lo <= got) & (got <= hi))
        res.append(Result(name, idx, got.numel(), bad.sum(), _first(bad, _rowcol(name, idx, got, lo, hi)), flips=int((got != pt).sum())))
        if l < L - 1:
            bits = torch.from_numpy(cap.mask[l])
            if rb is None:
                want = got > 0
                badm = bits != want
                first = _first(badm, lambda r, c: f"mask layer {l} (row {r}, column {c}), row tile {r // 80}, column tile {c // 128}: bit "
                                                   f"{int(bits[r, c])}, stored activation {float(got[r, c])!r}")
                res.append(Result("mask", l, bits.numel(), badm.sum(), first))
            else:
                blo, bhi = act(lo32) > 0, act(hi32) > 0
                badm = (bits != blo) & (bits != bhi)
                first = _first(badm, lambda r, c: f"mask layer {l} (row {r}, column {c}), row tile {r // 80}, column tile {c // 128}: bit "
                                                   f"{int(bits[r, c])}, v {float(v[r, c])!r}, s {float(s[r, c])!r}")
                res.append(Result("mask", l, bits.numel(), badm.sum(), first, left_out=int((blo != bhi).sum())))
    return res


def check_dgrad(cap):
    """dZ[l] for l < L - 1: mask * round16(dZ[l'] @ W[l'] (+ dR)), in the kernel's scaled units (the operands are stored scaled)."""
    fmt = cap.fmt
    L, _, dgrad, _ = structure(cap.nb)
    res = []
    dR = None
    for l, lo_, adds, emits in dgrad:
        u, A = _product(fmt, fmt.values(cap.dZ[l]), cap.W(l))
        v_lo = v_hi = u
        T = 512
        if adds:   # HAS_ADD: the residual gradient joins the fp32 sum before the rounding (rowgemm80_body: v += ad; pk4)
            v_lo, v_hi, A, T = u + dR[0], u + dR[1], A + torch.maximum(dR[0].abs(), dR[1].abs()), 513
        s = T * UNIT * A
        lo = fmt.round((v_lo - s).to(torch.float32))
        hi = fmt.round((v_hi + s).to(torch.float32))
        pt = fmt.round((0.5 * (v_lo + v_hi)).to(torch.float32))
        got = fmt.values(cap.dZ[lo_]).to(torch.float32)
        m = torch.from_numpy(cap.mask[lo_])
        zero = torch.from_numpy(cap.dZ[lo_] == 0)            # a masked element is the pattern 0x0000 (y &= 0)
        bad = torch.where(m, ~((lo <= got) & (got <= hi)), ~zero)
        desc = _rowcol("dZ", lo_, got, torch.where(m, lo, torch.zeros_like(lo)), torch.where(m, hi, torch.zeros_like(hi)))
        flips = int((m & (got != pt)).sum()) if not adds or bool((dR[0] == dR[1]).all()) else None
        res.append(Result("dZ", lo_, got.numel(), bad.sum(), _first(bad, desc), flips=flips))
        if emits:   # AUX_UNMASKED: dR is the rounded value itself where the bit is set, and only known by its interval elsewhere
            dR = (torch.where(m, got, lo).to(torch.float64), torch.where(m, got, hi).to(torch.float64))
    return res


def _outin(stage, l, slab, got, v, s):
    return lambda o, i: (f"{stage} layer {l} (out {o}, in {i}), tile ({o // 128}, {i // 128}), slab {slab}: got {float(got[o, i])!r}, "
                         f"lo {float(v[o, i] - s[o, i])!r}, hi {float(v[o, i] + s[o, i])!r}")


def _judge32(got, v, s):
    bad = ~((got - v).abs() <= s)
    ratio = torch.where(s > 0, (got - v).abs() / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(s))
    return bad, float(ratio.max()) if ratio.numel() else 0.0


def check_wgrad(cap):
    """Every slab of dW[l] against the rows wgrad_kloop assigns to it (T = rows of the slab), and tr.grad's weights against the sum of
    the slabs times the exact power of two inv_grad_scale."""
    fmt = cap.fmt
    L, _, _, ins = structure(cap.nb)
    res = []
    inv = cap.inv_grad_scale
    for l in range(L):
        Z, X = fmt.values(cap.dZ[l]), cap.src(ins[l])
        v_sum = torch.zeros(512, 512, dtype=torch.float64)
        s_sum = torch.zeros(512, 512, dtype=torch.float64)
        for sl in range(cap.nslabs):
            mb, me = slab_rows(cap.n, cap.nslabs, sl)
            v, A = _product(fmt, Z[mb:me].t(), X[mb:me])
            s = (me - mb) * UNIT * A
            got = torch.from_numpy(cap.slabs[sl, l * LAYER:l * LAYER + 262144].reshape(512, 512)).to(torch.float64)
            bad, worst = _judge32(got, v, s)
            res.append(Result("slab%d" % sl, l, got.numel(), bad.sum(), _first(bad, _outin("slab", l, sl, got, v, s)), worst=worst))
            v_sum, s_sum = v_sum + v, s_sum + s
        # grad_reduce_body: acc = slab 0; acc += slab s (one fp32 addition each, |result| <= |v| + s); acc *= inv (exact)
        s_g = (s_sum + (cap.nslabs - 1) * ADD * (v_sum.abs() + s_sum)) * inv
        got = torch.from_numpy(cap.grad[l * LAYER:l * LAYER + 262144].reshape(512, 512)).to(torch.float64)
        bad, worst = _judge32(got, v_sum * inv, s_g)
        res.append(Result("grad_w", l, got.numel(), bad.sum(), _first(bad, _outin("grad_w", l, "all", got, v_sum * inv, s_g)), worst=worst))
        # ... and those very additions, restated in fp32 from the stored slabs, give tr.grad bit for bit
        acc = cap.slabs[0, l * LAYER:l * LAYER + 262144].copy()
        for sl in range(1, cap.nslabs):
            acc = acc + cap.slabs[sl, l * LAYER:l * LAYER + 262144]
        same = torch.from_numpy((acc * np.float32(inv)).view(np.uint32) != cap.grad[l * LAYER:l * LAYER + 262144].view(np.uint32)).reshape(512, 512)
        res.append(Result("grad_w_bits", l, same.numel(), same.sum(), _first(same, lambda o, i: f"grad_w layer {l} (out {o}, in {i}) is not the fp32 sum of its slabs")))
    return res


def check_bias(cap):
    """bias_partials of the layers whose dZ an input-gradient launch produces (l < L - 1): column sums of the STORED dZ rows of every 80-row
    tile, min(80, n - m0) of them; tr.grad's biases of every layer: the column sums over all n rows."""
    fmt = cap.fmt
    L = 3 * cap.nb + 5
    n, inv = cap.n, cap.inv_grad_scale
    tiles = (n + 79) // 80
    res = []
    for l in range(L):
        Z = fmt.values(cap.dZ[l])
        if l < L - 1:
            v = torch.stack([Z[80 * t:min(n, 80 * t + 80)].sum(0) for t in range(tiles)])
            A = torch.stack([Z[80 * t:min(n, 80 * t + 80)].abs().sum(0) for t in range(tiles)])
            T = torch.tensor([min(n, 80 * t + 80) - 80 * t for t in range(tiles)], dtype=torch.float64)[:, None]
            s = T * UNIT * A
            got = torch.from_numpy(cap.bias_partials[l][:tiles]).to(torch.float64)
            bad, worst = _judge32(got, v, s)
            first = _first(bad, lambda t, c: f"bias_partials layer {l} (row tile {t}, column {c}), column tile {c // 128}: got {float(got[t, c])!r}, "
                                             f"lo {float(v[t, c] - s[t, c])!r}, hi {float(v[t, c] + s[t, c])!r}")
            res.append(Result("bias_partials", l, got.numel(), bad.sum(), first, worst=worst))
        # A partial row sums at most 80 rows (an 80-row tile; 32 rows in the loss kernel, which produces layer L - 1's): 80 * 2^-23 * A over
        # all of them. The reduction (SmallCols: five in-register rounds, a three-level tree, three butterfly levels; more rounds past 320
        # partial rows) puts every partial through at most D further fp32 additions, each off by 2^-24 of a partial sum <= A (1 + 80 * 2^-23).
        v, A = Z.sum(0), Z.abs().sum(0)
        cnt = max(tiles, (n + 31) // 32)
        D = 11 + max(0, (cnt + 63) // 64 - 5)
        s = (80 * UNIT * A + D * ADD * A * (1 + 80 * UNIT)) * inv
        got = torch.from_numpy(cap.grad[l * LAYER + 262144:(l + 1) * LAYER]).to(torch.float64)
        bad, worst = _judge32(got[None], (v * inv)[None], s[None])
        first = _first(bad, lambda _, c: f"grad_b layer {l} (column {c}): got {float(got[c])!r}, lo {float(v[c] * inv - s[c])!r}, hi {float(v[c] * inv + s[c])!r}")
        res.append(Result("grad_b", l, got.numel(), bad.sum(), first, worst=worst))
    return res


def check_all(cap):
    L = 3 * cap.nb + 5
    assert np.isfinite(cap.bias).all() and np.isfinite(cap.grad[:L * LAYER]).all(), "a bias or a wide-layer gradient is not finite"
    for a in list(cap.R) + list(cap.dZ) + list(cap.out.values()):
        assert bool(torch.isfinite(cap.fmt.values(a)).all()), "a stored 16-bit operand is not finite: nothing can be restated from it"
    return check_forward(cap) + check_dgrad(cap) + check_wgrad(cap) + check_bias(cap)


def assert_clean(results, what=""):
    """Every element inside its bounds."""
    failed = [r for r in results if r.bad]
    assert not failed, "%s: %d elements outside their bounds in %d stages\n%s" % (what, sum(r.bad for r in failed), len(failed), "\n".join(str(r) for r in failed))


def assert_left_out_capped(results, what=""):
    """The undecided mask bits of every layer, over all the results given (one capture, or the captures of one configuration), within the cap."""
    pooled = {}
    for r in results:
        if r.stage == "mask":
            t = pooled.setdefault(r.layer, [0, 0])
            t[0] += r.left_out
            t[1] += r.total
    for layer, (left, total) in pooled.items():
        assert left <= MASK_LEFT_OUT_CAP * total, "%s: mask[%d]: %d of %d mask bits undecided" % (what, layer, left, total)


def summary(results):
    """Per stage, for the record: the worst |got - v| / s of the fp32 stages, the rounding flips and the left-out bits of the others."""
    out = {}
    for r in results:
        stage = r.stage[:4] if r.stage.startswith("slab") else r.stage
        d = out.setdefault(stage, {"elements": 0, "worst": None, "flips": None, "left_out": 0})
        d["elements"] += r.total
        d["left_out"] += r.left_out
        if r.worst is not None:
            d["worst"] = max(d["worst"] or 0.0, r.worst)
        if r.flips is not None:
            d["flips"] = (d["flips"] or 0) + r.flips
    return out
