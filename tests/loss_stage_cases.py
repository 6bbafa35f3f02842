"""The inputs of the loss-stage tests (tests/test_loss_stage_cpu.py, tests/test_loss_stage_gpu.py): configurations, row counts, the head
parameters whose fc3 spans the softplus / clamp regimes, and the PLANTING of every buffer row's pose, intrinsics and targets around the
scene coordinate the code under test itself produced for that row.

Every buffer row is its own view and its own image, so each row has its own augmentation, pose, intrinsics, pixel target and target
coordinate. X depends only on the features and the weights: one pass gives the X of every buffer row (on the GPU: the kernel's own, from a
full-size backward(); on the CPU: the float32 stand-in's), `plant` then chooses, per row, the camera point the row shall have and solves
the pose translation for it, and places the pixel target at a chosen signed offset from the pixel the kernel computes from its stored X
(tests/loss_stage_restated.py pixel_points: that chain is exact). A row probes ONE threshold and sits at least 1 px or 1 cm from it; the
`exact` kind puts e on inlier_px itself (e == 10 exactly: `<` against `<=`)."""
import functools

import numpy as np
import torch

from oracle import head_oracle
from tests import loss_stage_restated as ls

ROWS = [1, 3, 4, 5, 15, 16, 17, 33, 80, 81, 357, 1025]
NBUF = 1040                    # buffer rows = max_batch: the full-size backward() that fills every buffer and partial slot
SEED = 7331
FOCAL_INIT = 500.0
MEAN = np.array([1.5, -0.5, 2.0], np.float32)
BRANCH_MIN = 8                 # decided rows every reachable branch must hold in every configuration
UNDECIDED_CAP = 0.01

CONFIGS = {}
for _lt in ("tanh", "dyntanh", "l1", "l1+sqrt", "l1+log"):
    for _h in (True, False):
        CONFIGS["%s-%s" % (_lt, "homog" if _h else "plain")] = dict(loss_type=_lt, homog=_h, calib=False, depth=False)
CONFIGS["calib"] = dict(loss_type="tanh", homog=True, calib=True, depth=False)
CONFIGS["depth"] = dict(loss_type="tanh", homog=True, calib=False, depth=True)
CONFIGS["depth-l1-plain"] = dict(loss_type="l1", homog=False, calib=False, depth=True)
# pose refinement 'naive': the world -> camera matrices are the parameters; the loss reads their orthonormalised copies and emits row_dT
CONFIGS["pose"] = dict(loss_type="tanh", homog=True, calib=False, depth=False, pose=True)
CONFIGS["pose-l1-plain"] = dict(loss_type="l1", homog=False, calib=False, depth=False, pose=True)
FP16_CONFIGS = ("tanh-homog", "l1+sqrt-plain", "calib", "depth", "pose")     # not the full cross product in fp16

# kinds of planted rows: name -> (camera depth Xc2, K[2][2], e in px or None)
SOFT, INL, HARD, DMIN, DMAX = 50.0, 10.0, 1000.0, 0.1, 1000.0
KINDS = [
    ("inlier", None, 1.0, 3.0), ("below_inlier", None, 1.0, INL - 1.25), ("above_inlier", None, 1.0, INL + 1.25), ("exact_inlier", None, 1.0, "exact"),
    ("below_wgt", None, 1.0, SOFT - 1.5), ("above_wgt", None, 1.0, SOFT + 2.5), ("large", None, 1.0, 300.0),
    ("below_hard", None, 1.0, HARD - 2.0), ("above_hard", None, 1.0, HARD + 2.0), ("far_off", None, 1.0, 2500.0),
    ("near", DMIN - 0.012, 1.0, 20.0), ("just_in_front", DMIN + 0.012, 1.0, 20.0), ("behind", -2.0, 1.0, 20.0),
    ("far", DMAX + 0.05, 1.0, 20.0), ("just_inside", DMAX - 0.05, 1.0, 20.0),
    ("zclamped", 0.15, 0.5, 6.0),          # K[2][2] = 0.5: pp[2] = 0.075 < depth_min in a row whose Xc[2] is valid
]
DEPTH_KINDS = ["none", "close", "below_10cm", "above_10cm", "distant", "on_X"]     # target_crds: absent, 3 cm, 8.8 cm, 11.2 cm, 40 cm, equal to X


def wgt_of(loss_type):
    """head_sched.h sched_prepare_hot at iteration 0 with soft_clamp 50, soft_clamp_min 1."""
    return 51.0 if loss_type == "dyntanh" else 50.0


def fmt_round(dtype, a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return t.to(torch.bfloat16 if dtype == "bf16" else torch.float16).to(torch.float32).numpy()


@functools.lru_cache(maxsize=None)
def head_inputs(dtype, homog):
    """(features [NBUF,512] representable in the format, flat fp32 parameters, out[L - 1] of the oracle's forward as uint16 patterns).
    fc3 is set from the oracle's fc2 output: s0..s2 centred with a standard deviation of 2, s3 (homogeneous) from -50 to 150 -- below
    the softplus threshold (bx <= 20: s3 <= 21.6), between it and the clamp, and past the clamp (s3 > 99.75)."""
    rng = np.random.default_rng(SEED)
    feats = fmt_round(dtype, rng.normal(0.0, 0.5, size=(NBUF, 512)))
    flat = head_oracle.init_params(SEED + 1, 1, homog).clone()
    no = 4 if homog else 3
    orc = head_oracle.HeadOracle(flat, MEAN, 1, homog, mode=dtype)
    _, tape = orc.forward(torch.from_numpy(feats))
    f2 = tape["out"][7].double().numpy()
    W3 = np.zeros((no, 512))
    b3 = np.zeros(no)
    for j in range(no):
        u = rng.normal(size=512)
        z = f2 @ u
        if j < 3:
            k, off = 2.0 / z.std(), -2.0 * z.mean() / z.std()
        else:
            k = 200.0 / (z.max() - z.min())
            off = -50.0 - k * z.min()
        W3[j], b3[j] = k * u, off
    o = 8 * 262656
    flat[o:o + no * 512] = torch.from_numpy(W3.reshape(-1).astype(np.float32))
    flat[o + no * 512:] = torch.from_numpy(b3.astype(np.float32))
    fmt = ls.Fmt(dtype)
    return feats, flat, fmt.bits(tape["out"][7])


def scalars(name, dtype, n, grad_scale=1.0, calib_g=0.0):
    c = CONFIGS[name]
    return ls.make_cfg(homog=c["homog"], loss_type=c["loss_type"], mean=MEAN, refine_calibration=c["calib"], focal_init=FOCAL_INIT, calib_g=calib_g,
                       global_batch=n, wgt=wgt_of(c["loss_type"]), grad_scale=grad_scale, f16=dtype == "fp16", pose=c.get("pose", False))


def _rot(rng, n, max_angle):
    from scipy.spatial.transform import Rotation
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    return Rotation.from_rotvec(ax * rng.uniform(0, max_angle, size=(n, 1))).as_matrix()


def plant(name, X, poses=None):
    """poses [NBUF,16]: a pose configuration's refined matrices, as the loss reads them (the device's orthonormalisation of the planted
    ones, which stay in the tables as T0: the parameters to load); the pixel targets are then planted around THEIR projection.
    The buffer tables for the scene coordinates X [NBUF,3] (float32, as stored by the code under test): dict of float32 arrays
    A [NBUF,12], T [NBUF,16], K, Ki [NBUF,9], tu, tv [NBUF], tc [NBUF,3] (depth configurations, else None), and kind [NBUF] (index into
    KINDS), dkind [NBUF] (index into DEPTH_KINDS)."""
    cfg = CONFIGS[name]
    rng = np.random.default_rng(SEED + 5)
    X = np.asarray(X, np.float32).astype(np.float64)
    kind = rng.permutation(NBUF) % len(KINDS)
    dkind = rng.permutation(NBUF) % len(DEPTH_KINDS)
    # augmentation: in-plane rotation and scale (3 x 4, no translation); pose: a rotation and the translation that puts X at the wanted camera point
    ang = rng.uniform(-0.3, 0.3, NBUF)
    sc = rng.uniform(0.8, 1.25, NBUF)
    Ra = np.zeros((NBUF, 3, 3))
    Ra[:, 0, 0], Ra[:, 0, 1], Ra[:, 1, 0], Ra[:, 1, 1], Ra[:, 2, 2] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang), 1.0
    Rt = _rot(rng, NBUF, 1.0)
    depth = np.array([KINDS[k][1] if KINDS[k][1] is not None else np.nan for k in kind])
    depth = np.where(np.isnan(depth), rng.uniform(1.0, 20.0, NBUF), depth)
    want = np.stack([depth * rng.uniform(-0.4, 0.4, NBUF), depth * rng.uniform(-0.4, 0.4, NBUF), depth], 1)
    t = np.einsum("nji,nj->ni", Ra, want) - np.einsum("nij,nj->ni", Rt, X)        # Ra^T want - Rt X
    A = np.concatenate([Ra, np.zeros((NBUF, 3, 1))], 2).astype(np.float32)
    T = np.tile(np.eye(4), (NBUF, 1, 1))
    T[:, :3, :3], T[:, :3, 3] = Rt, t
    T = T.astype(np.float32)
    f = FOCAL_INIT * sc
    K = np.zeros((NBUF, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = f, f, 320.0, 240.0
    K[:, 2, 2] = np.array([KINDS[k][2] for k in kind])
    Ki = np.linalg.inv(K).astype(np.float32)
    K = K.astype(np.float32)
    T0 = T.reshape(NBUF, 16)
    T = T0 if poses is None else np.asarray(poses, np.float32).reshape(NBUF, 16)
    tabs = dict(A=A.reshape(NBUF, 12), T=T, T0=T0, K=K.reshape(NBUF, 9), Ki=Ki.reshape(NBUF, 9), tu=np.zeros(NBUF, np.float32),
                tv=np.zeros(NBUF, np.float32), tc=None)
    # the pixel target: at a signed offset from the pixel the kernel computes from its stored X
    c = scalars(name, "bf16", NBUF)
    t64 = {k: (None if v is None else v.astype(np.float64)) for k, v in tabs.items() if k != "T0"}
    u, v, xc2, _, exact = ls.pixel_points(X, t64, c)
    assert exact.mean() > 0.99
    e_want = np.array([KINDS[k][3] if KINDS[k][3] != "exact" else INL for k in kind], np.float64)
    is_exact = np.array([KINDS[k][3] == "exact" for k in kind])
    split = np.where(is_exact, 1.0, rng.uniform(0.1, 0.9, NBUF))
    sg = rng.choice([-1.0, 1.0], size=(NBUF, 2))
    tu = (u - sg[:, 0] * split * e_want).astype(np.float32)
    tv = (v - sg[:, 1] * (1.0 - split) * e_want).astype(np.float32)
    # e == inlier_px exactly needs u - tu == +-10 in fp32: where u - 10 is not representable (it crosses a power of two), u + 10 is tried
    flip = is_exact & (np.abs(u - tu.astype(np.float64)) != INL)
    tu = np.where(flip, (u + sg[:, 0] * INL).astype(np.float32), tu)
    tabs["tu"], tabs["tv"] = tu, tv
    if cfg["depth"]:
        d = rng.normal(size=(NBUF, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        dist = np.array([0.0, 0.03, 0.088, 0.112, 0.4, 0.0])[dkind]
        tc = (X + d * dist[:, None]).astype(np.float32)
        tc[dkind == 0] = 0.0
        tabs["tc"] = tc
    tabs["kind"], tabs["dkind"] = kind, dkind
    return tabs


def batch_tables(tabs, idx):
    """The per-row tables of a batch (float64 arrays of the exact fp32 values), as loss_rows reads them."""
    return {k: (None if tabs[k] is None else np.asarray(tabs[k])[idx].astype(np.float64)) for k in ("A", "T", "K", "Ki", "tu", "tv", "tc")}


def batch_indices(n):
    """The buffer rows of the judged batch of n rows, and of the full-size batch before it."""
    rng = np.random.default_rng(SEED + 100 + n)
    return rng.permutation(NBUF), rng.permutation(NBUF)[:n]


# branch -> (reachable in configuration c?, the decided rows of a record that count)
def branch_counts(c, rec, decided):
    out = {}
    v = rec["valid"]
    add = lambda k, m: out.__setitem__(k, int((m & decided).sum()))
    if c["homog"]:
        add("softplus", ~rec["bx>20"])
        add("bx>20, not clamped", rec["bx>20"] & ~rec["hclamped"])
        add("hclamped", rec["hclamped"])
    add("e<inlier_px", rec["e<inlier"])
    add("e>=inlier_px", v & ~rec["e<inlier"])
    if "e>wgt" in rec:
        add("e>wgt", rec["e>wgt"])
        add("e<=wgt", v & ~rec["e>wgt"])
    add("e>hard_clamp", rec["e>hard_clamp"])
    add("depth<depth_min", rec["Xc2<depth_min"])
    add("depth>depth_max", rec["Xc2>depth_max"])
    add("zclamped in a valid row", rec["zclamped"])
    if c["depth"]:
        add("tavail false", ~rec["tavail"])
        add("tdist<=0.1", rec["tavail"] & ~rec["tdist>0.1"] & rec["geometry_valid"])
        add("tdist>0.1", rec["tdist>0.1"])
        add("tdist==0 in an invalid row", rec["tdist==0"])
        add("depth loss", rec["tdist>0"])
    else:
        add("proxy target", ~v)
    return out
