"""CPU: the checker of the loss stage (tests/loss_stage_restated.py) proven before it judges a kernel, on exactly the inputs the GPU test
uses (tests/loss_stage_cases.py; only the activations differ: the oracle's forward pass instead of the kernels').

  * the numpy float32 stand-in of loss_body passes every configuration at every row count, with its product-sums contracted into FMAs
    and not contracted, with no element outside its interval and every bitwise sum reproduced;
  * the rows with an undecided comparison stay within the cap and every reachable branch holds its planted, decided rows;
  * the forward pass written a second time in torch float64 gives, by autograd, the ds of the interval midpoints;
  * loss, inliers and ds agree with oracle/head_oracle.py in fp32 mode, which is pinned against the reference;
  * every mutant of the stand-in fails."""
import functools

import numpy as np
import pytest
import torch

from oracle import head_oracle
from tests import loss_stage_cases as C
from tests import loss_stage_restated as ls

GRAD_SCALE_FP16 = 64.0


@functools.lru_cache(maxsize=None)
def _world(name, dtype):
    cfg = C.CONFIGS[name]
    fmt = ls.Fmt(dtype)
    no = 4 if cfg["homog"] else 3
    _, flat, act16 = C.head_inputs(dtype, cfg["homog"])
    o = 8 * 262656
    W3_16 = fmt.bits(fmt.round(flat[o:o + no * 512].view(no, 512)))
    b3 = flat[o + no * 512:].numpy().copy()
    X = ls.stand_in_X(fmt, act16, W3_16, b3, C.scalars(name, dtype, C.NBUF), no)
    assert np.isfinite(X).all()
    return fmt, no, act16, W3_16, b3, X, C.plant(name, X)


def _case(name, dtype, n, contract, mut=()):
    fmt, no, act16, W3_16, b3, X, tabs = _world(name, dtype)
    full, idx = C.batch_indices(n)
    c = C.scalars(name, dtype, n, grad_scale=GRAD_SCALE_FP16 if dtype == "fp16" else 1.0)
    ext = np.concatenate([idx, full[~np.isin(full, idx)][:1]]) if n < C.NBUF else idx      # one more row: what lies past n in the buffers
    stale = None
    if "block_past_end" in mut:      # the slots an earlier full-size batch left behind
        g = ls.stand_in(fmt, act16[full], W3_16, b3, C.batch_tables(tabs, full), c, C.NBUF, no, contract)
        stale = (g["bias_partials"], g["fc3_partials"], g["stat_partials"])
    got = ls.stand_in(fmt, act16[ext], W3_16, b3, C.batch_tables(tabs, ext), c, n, no, contract, mut, stale)
    cap = dict(out16=act16[idx], W3=W3_16, b3=b3, **got)
    V, und, o = ls.judge(fmt, cap, C.batch_tables(tabs, idx), c, n, no)
    return V, und, o, got, (fmt, no, act16[idx], W3_16, b3, X[idx], C.batch_tables(tabs, idx), c)


def _params():
    out = [(n, "bf16") for n in C.CONFIGS] + [(n, "fp16") for n in C.FP16_CONFIGS]
    return [pytest.param(n, d, k, id="%s-%s-%s" % (n, d, "fma" if k else "plain")) for n, d in out for k in (True, False)]


@pytest.mark.parametrize("name,dtype,contract", _params())
def test_the_stand_in_passes_and_the_planted_branches_are_decided(name, dtype, contract):
    und_rows, rows, branches = 0, 0, {}
    for n in C.ROWS:
        V, und, o, got, w = _case(name, dtype, n, contract)
        assert np.array_equal(got["X"].view(np.uint32), w[5].view(np.uint32)), "X changed with the planted tables"
        assert not V.failed(), "%s %s n=%d: %s" % (name, dtype, n, "\n".join(V.lines("")))
        und_rows, rows = und_rows + int(und.sum()), rows + n
        for k, v in C.branch_counts(C.CONFIGS[name], o["rec"], ~und).items():
            branches[k] = branches.get(k, 0) + v
    assert und_rows <= C.UNDECIDED_CAP * rows, "%d of %d rows undecided" % (und_rows, rows)
    thin = {k: v for k, v in branches.items() if v < C.BRANCH_MIN}
    assert not thin, "branches with fewer than %d decided rows: %r" % (C.BRANCH_MIN, thin)


@pytest.mark.parametrize("name", list(C.CONFIGS))
def test_autograd_of_a_second_forward_gives_the_midpoints_and_the_oracle_agrees(name):
    n = 357
    _, _, _, _, (fmt, no, act, W3_16, b3, X, tabs, c) = _case(name, "bf16", n, True)
    ulps = ls.math_ulps()
    # The midpoints of a ZERO-WIDTH pass: the same text with no widening at all is the float64 value of loss_rows (the midpoint of a
    # widened interval leaves it by the square of the relative half-width). s enters as points, X as the stored value, every
    # comparison is decided; autograd differentiates the second forward on the same branches.
    s = [ls.Iv(v.mid) for v in ls.phase_a_interval(fmt, act, W3_16, b3, no)]
    o, und = ls.rows_interval(s, tabs, c, X.astype(np.float64), ulps, zero_width=True)
    assert not und.any()
    st = torch.tensor(np.stack([v.mid for v in s], 1), dtype=torch.float64, requires_grad=True)
    ls.forward_torch(st, tabs, c, o["rec"], X).backward()
    auto = st.grad.numpy()
    for j in range(no):
        mid = o["ds"][j].mid
        assert np.array_equal(o["ds"][j].lo, o["ds"][j].hi)
        bad = ~(np.abs(mid - auto[:, j]) <= 1e-9 * np.abs(auto[:, j]))      # 1e-9 relative, nothing else
        assert not bad.any(), "ds[%d], row %d: midpoint %r, autograd %r" % (j, int(np.argmax(bad)), mid[np.argmax(bad)], auto[np.argmax(bad), j])
    assert np.abs(auto).max() > 0
    # ---- the oracle, fp32 mode, on the decided rows (it computes its own X from s: the rows planted on a threshold are not its business)
    # It computes its own X from s, an ulp or so from the stored one, and in a depth row that ulp is 1e-5 of target - X: for this
    # comparison the restatement goes on with its own interval of X as well (the rows whose target lies ON the stored X are then undecided)
    cfg = C.CONFIGS[name]
    o, und = ls.rows_interval(s, tabs, c, None, ulps, points=False)
    ok = ~und
    assert ok.mean() > 0.85
    sel = np.nonzero(ok)[0]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    batch = dict(target_px=T(np.stack([tabs["tu"], tabs["tv"]], 1)[sel]), aug_inv=T(tabs["A"][sel]).view(-1, 3, 4), pose_inv=T(tabs["T"][sel]).view(-1, 4, 4),
                 K=T(tabs["K"][sel]).view(-1, 3, 3), Kinv=T(tabs["Ki"][sel]).view(-1, 3, 3), target_crds=None if tabs["tc"] is None else T(tabs["tc"][sel]))
    ocfg = dict(global_batch=n, refine_calibration=cfg["calib"], focal_init=C.FOCAL_INIT, depth_min=C.DMIN, depth_max=C.DMAX, hard_clamp=C.HARD,
                loss_type=cfg["loss_type"], soft_clamp=50.0, soft_clamp_min=1.0, iterations=100, circle_schedule=True, use_depth=cfg["depth"],
                inlier_px_threshold=C.INL, depth_target=10.0)
    orc = head_oracle.HeadOracle(torch.zeros(head_oracle.num_params(1, cfg["homog"])), C.MEAN, 1, cfg["homog"], mode="fp32")
    s32 = T(np.stack([v.mid for v in s], 1)[sel][:, :no])
    res = orc.loss_and_ds(s32, batch, ocfg, 0)
    dso = res["ds"].numpy().astype(np.float64)
    scale = np.max(np.abs(np.stack([o["ds"][j].mid for j in range(no)], 1)[sel]), 1)
    for j in range(no):
        mid, rad = o["ds"][j].mid[sel], o["ds"][j].rad[sel]
        # "The oracle's own precision": it evaluates the same expressions in fp32, in another order (bmm instead of FMA chains), so
        # its error is a sum of roundings of the kind the half-width rad adds up -- one 2^-24 per operation -- but of other operations.
        # 16 rad covers a different association of every product-sum (at most four terms: each term's rounding counted up to four
        # times over) with a factor 4 to spare; 1e-6 of the row's largest |ds| = 16 x 2^-24 covers the float32 rounding of s itself,
        # which the restatement takes as exact, carried through the about ten operations from s to ds.
        bad = ~(np.abs(dso[:, j] - mid) <= 16 * rad + 1e-6 * scale)
        assert not bad.any(), "oracle ds[%d], row %d: %r against %r +- %r" % (j, int(sel[np.argmax(bad)]), dso[np.argmax(bad), j], mid[np.argmax(bad)], rad[np.argmax(bad)])
    loss_mid, loss_rad = o["loss"].mid[sel].sum(), o["loss"].rad[sel].sum()
    assert abs(res["loss_sum"] - loss_mid) <= 16 * loss_rad + 2e-6 * np.abs(o["loss"].mid[sel]).sum(), (res["loss_sum"], loss_mid)
    assert res["inliers"] == o["inl"].mid[sel].sum()


MUTANTS = [
    ("dh_not_zeroed", "tanh-homog", "bf16", 357), ("sigmoid_when_big", "tanh-homog", "bf16", 357), ("dp2_not_zeroed", "l1-homog", "bf16", 357),
    ("fc3_row3_kept", "tanh-plain", "bf16", 81), ("inlier_le", "tanh-homog", "bf16", 357), ("no_inv_batch", "l1+log-plain", "bf16", 33),
    ("grad_scale_twice", "tanh-homog", "fp16", 81), ("mask_from_d", "dyntanh-homog", "bf16", 33), ("bias_unrounded", "tanh-homog", "bf16", 33),
    ("row_past_n", "tanh-homog", "bf16", 17), ("block_past_end", "tanh-homog", "bf16", 357), ("blocks_swapped", "tanh-homog", "bf16", 1025),
    ("tu_tv_swapped", "l1+sqrt-homog", "bf16", 357), ("truncate16", "tanh-homog", "bf16", 33), ("truncate16", "tanh-homog", "fp16", 33),
    # the pose gradient rows: the transposed index leaves every other output alone, so it fails through row_dT or not at all
    ("rd_A_transposed", "pose", "bf16", 81), ("no_inv_batch", "pose-l1-plain", "bf16", 33),
]


@pytest.mark.parametrize("mut,name,dtype,n", MUTANTS, ids=["%s-%s-%s" % (m[0], m[1], m[2]) for m in MUTANTS])
def test_every_mutant_of_the_stand_in_fails(mut, name, dtype, n):
    V, _, _, _, _ = _case(name, dtype, n, True, (mut,))
    assert V.failed(), "the mutant %s passed" % mut
    if C.CONFIGS[name].get("pose"):
        assert "row_dT" in V.failed(), "the mutant %s passed the pose gradient rows" % mut
    if mut == "rd_A_transposed":
        assert set(V.failed()) == {"row_dT"}
    clean, _, _, _, _ = _case(name, dtype, n, True)
    assert not clean.failed()
