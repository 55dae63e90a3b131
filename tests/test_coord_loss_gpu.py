"""GPU (-m gpu): hupr_coord_loss_fwd_f32 / hupr_coord_loss_bwd_f32 (csrc/coord_loss.hip) against the fp64 statement of the rule in
include/hupr.h (``ref_coord`` in tests/test_coord_loss_cpu.py, which checks the reference itself), and every layer built on them:
``functional.CoordLossFn``, ``LossComputer`` with ``TRAINING.coordLoss``, ``TrainEngine`` eager and captured, and the Runner with its
per-epoch line.  Every raw launch writes into outputs pre-filled with NaN.

Inputs (``make_case``): before any comparison each test asserts in fp64 that |r| >= 0.05 on both axes of every valid row, so no sign
is decided by rounding and no row is left out of a comparison.

Bounds.  resid against fp64: |err| <= 5e-6 (A + |r|) + 1e-7 with A = sum p |x - a| / (S + eps): a thread adds at most 64 terms in
sequence (H = 128; 16 at H = 64), then 6 additions of the wave butterfly and 4 across the waves, 74 roundings of 6e-8 = 4.4e-6,
relative to the sum of magnitudes for N and to S for the denominator.  scale = w / (S + eps): the same 5e-6, relative.  loss3: 1e-5
of its magnitude.  dp: per plane, 5e-5 of that plane's largest |dp| in fp64 — the residual's error relative to the farthest
pixel's distance (at least (H - 1) / 2), the relative error of S and a few roundings.  Zero rows: exactly zero."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from test_coord_loss_cpu import A0, A1, CASES, G, MARGIN, STRIDE, make_case, make_weights, ref_coord, sign_margin
from test_ohkm_cpu import MARGIN as SEL_MARGIN, ref_mined, selection_margin

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def launch_fwd(p1, p2, joints, snap, w=None, a0=1.0, a1=1.0, acc=None, stride=STRIDE, eps=1.0):
    """The C ABI on outputs pre-filled with NaN, so a value the kernels do not write shows.  p1, p2: (B, K, H, H) device tensors."""
    from hupr_amd import runtime as rt
    B, K, H, _ = p1.shape
    loss3 = torch.full((3,), NAN, dtype=torch.float32, device="cuda")
    resid = torch.full((2, B, K, 2), NAN, dtype=torch.float32, device="cuda")
    scale = torch.full((2, B, K), NAN, dtype=torch.float32, device="cuda")
    rt.check(rt.lib().hupr_coord_loss_fwd_f32(rt.ptr(p1), rt.ptr(p2), rt.ptr(joints), B, K, H, stride, snap, rt.ptr(w), eps, a0, a1,
                                              rt.ptr(loss3), rt.ptr(resid), rt.ptr(scale), rt.ptr(acc), rt.stream()))
    return loss3, resid, scale


def launch_bwd(resid, scale, joints, H, snap, g, a0=1.0, a1=1.0, stride=STRIDE):
    from hupr_amd import runtime as rt
    _, B, K = scale.shape
    dp1 = torch.full((B, K, H, H), NAN, dtype=torch.float32, device="cuda")
    dp2 = torch.full((B, K, H, H), NAN, dtype=torch.float32, device="cuda")
    gd = torch.tensor([g], dtype=torch.float32, device="cuda")
    rt.check(rt.lib().hupr_coord_loss_bwd_f32(rt.ptr(resid), rt.ptr(scale), rt.ptr(joints), rt.ptr(gd), B, K, H, stride, snap, a0, a1,
                                              rt.ptr(dp1), rt.ptr(dp2), rt.stream()))
    return dp1, dp2


def f64(x):
    return x.detach().cpu().numpy().astype(np.float64)


def check_resid(got, ref, what):
    got = f64(got)
    err = np.abs(got - ref["resid"])
    bound = 5e-6 * (ref["A"] + np.abs(ref["resid"])) + 1e-7
    print("%s: resid max |err| %.3e, worst err / bound %.3f" % (what, err.max(), (err / bound).max()))
    assert (err <= bound).all(), what
    assert not got[:, ~ref["valid"]].any(), what                                           # zero rows: exactly zero


def check_scale(got, ref, what):
    got = f64(got)
    assert np.array_equal(got != 0, ref["scale"] != 0), what                               # invalid rows and zero weights exactly
    err = np.abs(got - ref["scale"])
    print("%s: scale worst relative err %.3e" % (what, (err / np.maximum(ref["scale"], 1e-300)).max()))
    assert (err <= 5e-6 * ref["scale"]).all(), what


def check_loss3(got, ref3, what, tol=1e-5):
    got = f64(got)
    err = np.abs(got - ref3)
    print("%s: loss3 %s vs %s (rel %.3e)" % (what, got, ref3, (err / np.maximum(np.abs(ref3), 1e-300)).max()))
    assert np.isfinite(got).all() and (err <= tol * np.abs(ref3)).all(), what


def check_dp(got, ref_dp, what, extra=0.0):
    """got, ref_dp: (B, K, H, H).  Per plane, |err| <= 5e-5 of the plane's largest |ref| (+ extra); a zero plane exactly zero."""
    got = f64(got) if isinstance(got, torch.Tensor) else got
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref_dp).max(axis=(-1, -2))
    top = np.abs(ref_dp).max(axis=(-1, -2))
    live = top > 0
    print("%s: worst plane err / max %.3e" % (what, (err[live] / top[live]).max() if live.any() else 0.0))
    assert (err <= 5e-5 * top + extra).all(), what
    if not extra:
        assert not got[~live].any(), what


@functools.lru_cache(maxsize=None)
def case(shape):
    return make_case(*shape, CASES[shape], STRIDE)


# ---- 1: the kernels against the rule in fp64 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("snap", [0, 1], ids=["float", "snap"])
@pytest.mark.parametrize("shape", list(CASES), ids=lambda s: "B%d-K%d-H%d" % s)
def test_kernels_against_fp64(shape, snap, weighted):
    B, K, H = shape
    p1, p2, joints = case(shape)
    w = make_weights(K) if weighted else None
    what = "B%d K%d H%d snap%d%s" % (B, K, H, snap, " weighted" if weighted else "")
    ref = ref_coord(p1, p2, joints, STRIDE, snap, w, 1.0, A0, A1, G)
    assert ref["valid"].all() and sign_margin(ref) >= MARGIN, (what, sign_margin(ref))
    d1, d2, dj, dw = dev(p1), dev(p2), dev(joints), (dev(w) if weighted else None)
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")
    loss3, resid, scale = launch_fwd(d1, d2, dj, snap, dw, A0, A1, acc)
    check_resid(resid, ref, what)
    check_scale(scale, ref, what)
    check_loss3(loss3, ref["loss3"], what)
    first = acc.cpu().numpy().copy()
    assert first[2] == 1.0 and (np.abs(first[:2] - ref["loss3"][1:]) <= 1e-5 * ref["loss3"][1:]).all(), (what, first)
    launch_fwd(d1, d2, dj, snap, dw, A0, A1, acc)
    second = acc.cpu().numpy()
    assert second[2] == 2.0 and (np.abs(second[:2] - 2 * first[:2]) <= 1e-12 * second[:2]).all(), (what, first, second)
    dp1, dp2 = launch_bwd(resid, scale, dj, H, snap, G, A0, A1)
    for h, dp in enumerate((dp1, dp2)):
        check_dp(dp, ref["dp"][h], "%s dp%d" % (what, h + 1))
    if weighted and K > 1:
        j0 = K // 3                                                                         # the zero weight: scale and every cell of dp
        assert not scale[:, :, j0].any() and not dp1[:, j0].any() and not dp2[:, j0].any()
        assert resid[:, :, j0].abs().min() > 0                                              # the residual itself is still reported


# ---- 2: invalid and degenerate rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("snap", [0, 1], ids=["float", "snap"])
@pytest.mark.parametrize("H", [8, 5], ids=["H8", "H5"])
def test_invalid_joints_give_zero_rows(H, snap):
    """Joints that are NaN, +inf, negative or past (H - 1) * stride: a zero row, a zero dp plane and finite losses although the
    planes of those rows hold NaN (they are not read); every other row keeps its bits against a run without the bad joints."""
    B, K = 2, 6
    p1, p2, joints = (x.copy() for x in make_case(B, K, H, 3, STRIDE))
    ref = ref_coord(p1, p2, joints, STRIDE, snap, None, 1.0, A0, A1, G)
    assert sign_margin(ref) >= MARGIN
    d2 = dev(p2)
    clean3, clean_r, clean_s = launch_fwd(dev(p1), d2, dev(joints), snap, None, A0, A1)
    bad = {(0, 1): (NAN, 8.0), (0, 4): (8.0, INF), (1, 0): (-8.0, 8.0), (1, 2): (8.0, (H - 1) * STRIDE + 8.0), (1, 5): (NAN, NAN)}
    for (b, j), xy in bad.items():
        joints[b, j] = xy
        p1[b, j] = NAN
    ref = ref_coord(p1, p2, joints, STRIDE, snap, None, 1.0, A0, A1, G)
    keep = ref["valid"]
    assert (~keep).sum() == len(bad) and sign_margin(ref) >= MARGIN
    dj = dev(joints)
    loss3, resid, scale = launch_fwd(dev(p1), d2, dj, snap, None, A0, A1)
    check_resid(resid, ref, "invalid H%d" % H)
    check_scale(scale, ref, "invalid H%d" % H)
    check_loss3(loss3, ref["loss3"], "invalid H%d" % H)
    kt = torch.from_numpy(keep).cuda()
    assert not resid[:, ~kt].any() and not scale[:, ~kt].any()
    assert torch.equal(resid[:, kt], clean_r[:, kt]) and torch.equal(scale[:, kt], clean_s[:, kt])
    assert (loss3[1:] < clean3[1:]).all()                                                   # the denominator is fixed: zeros count
    dp1, dp2 = launch_bwd(resid, scale, dj, H, snap, G, A0, A1)
    for h, dp in enumerate((dp1, dp2)):
        check_dp(dp, ref["dp"][h], "invalid H%d dp%d" % (H, h + 1))
        assert not dp[~kt].any() and dp[kt].abs().amax(dim=(-1, -2)).min() > 0


@pytest.mark.parametrize("H", [8, 5], ids=["H8", "H5"])
def test_empty_plane_and_nan_cell(H):
    B, K = 2, 6
    p1, p2, joints = (x.copy() for x in make_case(B, K, H, 4, STRIDE))
    d2, dj = dev(p2), dev(joints)
    _, clean_r, _ = launch_fwd(dev(p1), d2, dj, 0, None, A0, A1)
    # an all-zero plane under a valid joint: r = 0 exactly, and sgn(0) = 0 leaves its dp plane exactly zero
    p1[1, 3] = 0.0
    loss3, resid, scale = launch_fwd(dev(p1), d2, dj, 0, None, A0, A1)
    assert not resid[0, 1, 3].any() and scale[0, 1, 3].item() == 1.0 and torch.isfinite(loss3).all()
    dp1, dp2 = launch_bwd(resid, scale, dj, H, 0, G, A0, A1)
    assert not dp1[1, 3].any() and torch.isfinite(dp1).all() and torch.isfinite(dp2).all()
    keep = torch.ones((2, B, K), dtype=torch.bool, device="cuda")
    keep[0, 1, 3] = False
    assert torch.equal(resid[keep], clean_r[keep])
    # one NaN cell in a valid plane of head 0: not masked
    p1[0, 2, H // 2, 1] = NAN
    loss3, resid, scale = launch_fwd(dev(p1), d2, dj, 0, None, A0, A1)
    assert torch.isnan(loss3[0]) and torch.isnan(loss3[1]) and torch.isfinite(loss3[2])
    assert torch.isnan(resid[0, 0, 2]).all() and torch.isnan(scale[0, 0, 2])
    keep[0, 0, 2] = False
    assert torch.equal(resid[keep], clean_r[keep])
    dp1, dp2 = launch_bwd(resid, scale, dj, H, 0, G, A0, A1)
    assert torch.isnan(dp1[0, 2]).all() and int(torch.isnan(dp1).sum()) == H * H and torch.isfinite(dp2).all()


# ---- 3: run to run -----------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_equal_bits():
    shape = (3, 14, 64)
    p1, p2, joints = case(shape)
    d1, d2, dj, dw = dev(p1), dev(p2), dev(joints), dev(make_weights(14))
    outs = []
    for _ in range(2):
        acc = torch.zeros(3, dtype=torch.float64, device="cuda")
        loss3, resid, scale = launch_fwd(d1, d2, dj, 0, dw, A0, A1, acc)
        dp1, dp2 = launch_bwd(resid, scale, dj, 64, 0, G, A0, A1)
        outs.append((loss3, resid, scale, acc, dp1, dp2))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("H", [64, 5])
def test_equal_planes_with_equal_joints_give_equal_bits(H):
    B, K = 3, 14
    p1, p2, joints = (x.copy() for x in make_case(B, K, H, 11, STRIDE))
    for x in (p1, p2, joints):
        x[1, 9] = x[1, 4]
        x[2, 11] = x[0, 2]
    _, resid, scale = launch_fwd(dev(p1), dev(p2), dev(joints), 0)
    rb, sb = resid.view(torch.int32), scale.view(torch.int32)
    for h in range(2):
        assert torch.equal(rb[h, 1, 9], rb[h, 1, 4]) and torch.equal(rb[h, 2, 11], rb[h, 0, 2])
        assert sb[h, 1, 9].item() == sb[h, 1, 4].item() and sb[h, 2, 11].item() == sb[h, 0, 2].item()
    assert not torch.equal(rb[0, 1, 9], rb[0, 1, 5])


# ---- 4: the targets the loss trains towards ------------------------------------------------------------------------------------------------
def test_targets_as_predictions_leave_no_residual():
    """The sub-pixel target of a joint at least 6.5 heat-map px from every border (its window is not clipped) has its centroid on
    the joint: |r| <= 0.01 px without snap (0.0064 in fp64 over 4 000 random joints: the 13 x 13 window cuts the Gaussian's tails
    asymmetrically around a fractional centre).  The integer target of a joint on a whole map pixel is symmetric around it:
    |r| <= 1e-4 with snap."""
    from hupr_amd import functional as F_
    B, K, H = 32, 14, 64
    rng = np.random.RandomState(21)
    joints = dev(rng.uniform(6.5, H - 1 - 6.5, (B, K, 2)) * STRIDE)
    t = F_.gaussian_targets_subpixel(joints, H, int(H * STRIDE), 2)
    _, resid, scale = launch_fwd(t, t, joints, 0)
    worst = resid.abs().max().item()
    print("sub-pixel targets as predictions: max |r| %.3e" % worst)
    assert (scale > 0).all() and worst <= 0.01
    whole = torch.from_numpy(rng.randint(6, H - 6, (B, K, 2)) * int(STRIDE)).cuda()
    t = F_.gaussian_targets(whole, H, int(H * STRIDE), 2)
    _, resid, scale = launch_fwd(t, t, whole.float(), 1)
    worst = resid.abs().max().item()
    print("integer targets as predictions: max |r| %.3e" % worst)
    assert (scale > 0).all() and worst <= 1e-4


# ---- 5: the Function ---------------------------------------------------------------------------------------------------------------------
def test_function_is_the_raw_launches_bit_for_bit():
    from hupr_amd import functional as F_
    shape = (3, 14, 64)
    B, K, H = shape
    p1, p2, joints = case(shape)
    d1, d2, dj, dw = dev(p1), dev(p2), dev(joints), dev(make_weights(K))
    for snap, w, jt in ((0, None, dj), (1, dw, dj.double()), (0, dw, dj)):
        acc_raw, acc_fn = (torch.zeros(3, dtype=torch.float64, device="cuda") for _ in range(2))
        loss3, resid, scale = launch_fwd(d1, d2, dj, snap, w, A0, A1, acc_raw)
        dp1, dp2 = launch_bwd(resid, scale, dj, H, snap, G, A0, A1)
        a1, a2 = d1.clone().requires_grad_(True), d2.clone().requires_grad_(True)
        n0 = F_.rt.lib().hupr_launch_count()
        loss, heads = F_.CoordLossFn.apply(a1, a2, jt, STRIDE, bool(snap), w, A0, A1, acc_fn)
        (G * loss).backward()
        assert F_.rt.lib().hupr_launch_count() - n0 <= 3
        assert torch.equal(loss.detach(), loss3[0]) and torch.equal(heads, loss3[1:]) and not heads.requires_grad
        assert torch.equal(a1.grad, dp1) and torch.equal(a2.grad, dp2) and torch.equal(acc_raw, acc_fn)
        res = F_.CoordLossFn.last_residual
        assert torch.equal(res, resid) and not res.requires_grad and tuple(res.shape) == (2, B, K, 2)
    # what it cannot run raises; there is no fallback
    a1 = d1.clone().requires_grad_(True)
    ok = (a1, d2, dj, STRIDE, False, None, 1.0, 1.0, None)
    F_.CoordLossFn.apply(*ok)

    def but(**kw):
        names = ("p1", "p2", "joints", "stride", "snap", "joint_w", "a0", "a1", "acc")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))
    for args in (but(p2=d2[:, :7]), but(p2=d2.double()), but(p2=d2.cpu()), but(p1=d1.half(), p2=d2.half()), but(p2=d2[..., :32]),
                 but(p1=d1.reshape(B, K, -1), p2=d2.reshape(B, K, -1)), but(p2=p2),
                 but(joints=dj.cpu()), but(joints=dj[:, :7]), but(joints=dj.reshape(B, 2, K)), but(joints=dj > 0), but(joints=joints),
                 but(stride=0.0), but(stride=-4.0), but(stride=NAN), but(stride="4"),
                 but(joint_w=torch.ones(K)), but(joint_w=torch.ones(K + 1, device="cuda")),
                 but(joint_w=torch.ones(K, device="cuda", dtype=torch.float64)),
                 but(acc=torch.zeros(3, dtype=torch.float32, device="cuda")), but(acc=torch.zeros(4, dtype=torch.float64, device="cuda")),
                 but(acc=torch.zeros(3, dtype=torch.float64))):
        with pytest.raises(ValueError):
            F_.CoordLossFn.apply(*args)


# ---- 6: LossComputer -----------------------------------------------------------------------------------------------------------------------
def _cfg(**training):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    for k, v in training.items():
        setattr(cfg.TRAINING, k, v)
    return cfg


JOINT_W = [1.0, 1.0, 1.5, 1.0, 1.0, 1.5, 0.0, 0.5, 1.0, 2.0, 2.5, 1.0, 2.0, 2.5]
LAM = 0.5


def _loss_inputs(lc, k, w, B=2):
    """Integer joints, the targets LossComputer forms from them and predictions around them with a per-plane noise level (the
    inputs of tests/test_ohkm_gpu.py); the first seed that leaves the 1e-3 selection margin for (k, w) and |r| >= 0.05 everywhere."""
    from hupr_amd import synth
    K, H = 14, 64
    for seed in range(20):
        joints = torch.from_numpy(synth.keypoints(B, 40 + seed))
        T = lc.targets(joints.cuda()).cpu().numpy().reshape(B, K, H * H)
        rng = np.random.RandomState(50 + seed)
        a = np.stack([rng.permutation(np.linspace(0.05, 0.6, K)) for _ in range(B)])
        p = [np.clip(T + s * a[..., None] * rng.uniform(-1.0, 1.0, T.shape), 1e-4, 1.0 - 1e-4).astype(np.float32) for s in (1.0, 0.8)]
        coord = ref_coord(p[0].reshape(B, K, H, H), p[1].reshape(B, K, H, H), joints.numpy(), STRIDE, 1, w, 1.0, LAM, LAM, 1.0)
        if selection_margin(ref_mined(p[0], p[1], T, k, w)["v"], k) >= SEL_MARGIN and sign_margin(coord) >= MARGIN and coord["valid"].all():
            return joints, T, p[0], p[1], coord
    raise AssertionError("no seed in 0..19 leaves both margins")


def _run_loss(lc, joints, p1, p2, B=2, K=14, H=64):
    a1 = dev(p1).reshape(B, K, 1, H, H).requires_grad_(True)
    a2 = dev(p2).reshape(B, 1, K, H, H).requires_grad_(True)
    loss, loss2, _, _ = lc.computeLoss((a1, a2), joints.cuda(), decode="device")
    loss.backward()
    return loss.detach(), loss2.detach(), a1.grad.reshape(B, K, H, H), a2.grad.reshape(B, K, H, H)


@pytest.mark.parametrize("setting", ["plain", "weights", "ohkm"])
def test_loss_computer_adds_the_coordinate_term(setting):
    """loss and both gradients = the heat-map loss without the key + 0.5 times the fp64 coordinate term over all 14 joints, within
    the kernels' bounds plus the heat-map loss's 1e-6; loss2 stays the second head's BCE bit for bit.  The heat-map part is this
    LossComputer's own result on the same inputs with the key absent (plain, weights) or ``ref_mined`` in fp64 (ohkm: 8)."""
    from hupr_amd.misc.losses import LossComputer
    B, K, H = 2, 14, 64
    training = dict(plain={}, weights=dict(jointWeights=JOINT_W), ohkm=dict(ohkm=8))[setting]
    cfg = _cfg(coordLoss=LAM, **training)
    assert cfg.TRAINING.lossDecay == -1 and not hasattr(cfg.TRAINING, "targets")           # head weights (1, 1); integer targets: snap
    lc, base = LossComputer(cfg, "cuda"), LossComputer(_cfg(**training), "cuda")
    assert lc.coordLoss == LAM and base.coordLoss is None and lc.coord_residual is None
    k = 8 if setting == "ohkm" else K
    w = np.array(JOINT_W) if setting == "weights" else None
    joints, T, p1, p2, coord = _loss_inputs(lc, k, w)
    loss, loss2, g1, g2 = _run_loss(lc, joints, p1, p2)
    bl, bl2, bg1, bg2 = _run_loss(base, joints, p1, p2)
    assert base.coord_residual is None and torch.equal(loss2, bl2)
    if setting == "ohkm":
        mined = ref_mined(p1, p2, T, k, w, 1.0, 1.0, 1.0, None)
        heat, heat_dp = mined["loss3"][0], mined["dp_autograd"].reshape(2, B, K, H, H)
    else:
        heat, heat_dp = float(bl), np.stack([f64(bg1), f64(bg2)])
    want = heat + coord["loss3"][0]
    print("%s: loss %.7f vs %.7f (heat-map %.7f + coordinate %.7f)" % (setting, float(loss), want, heat, coord["loss3"][0]))
    assert abs(float(loss) - want) <= 1e-6 * abs(heat) + 1e-5 * abs(coord["loss3"][0])
    for h, g in enumerate((g1, g2)):
        check_dp(f64(g) - heat_dp[h], coord["dp"][h], "%s dpreds%d" % (setting, h + 1), extra=1e-6 * np.abs(heat_dp[h]).max())
    check_resid(lc.coord_residual, coord, setting)
    assert not lc.coord_residual.requires_grad and tuple(lc.coord_residual.shape) == (2, B, K, 2)
    acc = lc.coord_acc.cpu().numpy()                                                        # C_h itself, before lambda
    assert acc[2] == 1.0 and (np.abs(acc[:2] - coord["loss3"][1:]) <= 1e-5 * coord["loss3"][1:]).all(), acc
    # evaluation shows the trained loss and does not move the accumulator
    a1, a2 = dev(p1).reshape(B, K, 1, H, H), dev(p2).reshape(B, 1, K, H, H)
    with torch.no_grad():
        le, le2, _, _ = lc.computeLoss((a1, a2), joints.cuda(), decode=False)
    assert torch.equal(le, loss) and torch.equal(le2, loss2)
    assert np.array_equal(lc.coord_acc.cpu().numpy(), acc)
    lc.computeLoss((a1, a2), joints.cuda(), decode=False)                                   # gradients enabled: it counts
    assert lc.coord_acc[2].item() == 2.0


def test_loss_computer_without_the_key_is_the_pair_loss():
    from hupr_amd import functional as F_
    from hupr_amd.misc.losses import LossComputer
    B, K, H = 2, 14, 64
    for training in ({}, dict(coordLoss=-1)):
        lc = LossComputer(_cfg(**training), "cuda")
        assert lc.coordLoss is None and lc.coord_acc is None
        joints, T, p1, p2, _ = _loss_inputs(lc, K, None)
        a1 = dev(p1).reshape(B, K, 1, H, H).requires_grad_(True)
        a2 = dev(p2).reshape(B, 1, K, H, H).requires_grad_(True)
        n0 = F_.rt.lib().hupr_launch_count()
        loss, loss2, _, _ = lc.computeLoss((a1, a2), joints.cuda(), decode=False)
        loss.backward()
        moved = F_.rt.lib().hupr_launch_count() - n0
        b1, b2 = dev(p1).reshape(B, K, H, H).requires_grad_(True), dev(p2).reshape(B, K, H, H).requires_grad_(True)
        n0 = F_.rt.lib().hupr_launch_count()
        ref, ref2 = F_.PairBCEFn.apply(b1, b2, lc.targets(joints.cuda()), 1.0, 1.0)
        ref.backward()
        assert moved == F_.rt.lib().hupr_launch_count() - n0                               # today's launches (the targets count once each)
        assert torch.equal(loss, ref) and torch.equal(loss2, ref2)
        assert torch.equal(a1.grad.reshape(b1.shape), b1.grad) and torch.equal(a2.grad.reshape(b2.shape), b2.grad)
        assert lc.coord_residual is None


# ---- 7: the engine, eager and captured ---------------------------------------------------------------------------------------------------
def test_graph_replay_matches_eager_steps_with_the_coordinate_loss():
    """tests/test_ohkm_gpu.py::test_graph_replay_matches_eager_steps_with_mining at its size (B = 4, bf16) and with its bounds, with
    ``TRAINING.coordLoss: 0.5`` and ``TRAINING.targets: subpixel``: five eager steps against 2 eager + capture (1 warm-up step) +
    2 replays.  The accumulator replays with the step: both engines have counted five steps, and their sums agree."""
    from hupr_amd import functional as F_, synth
    from hupr_amd.tools.engine import TrainEngine
    try:
        F_.set_math("bf16")
        cfg = _cfg(coordLoss=LAM, targets="subpixel")
        dev0 = torch.device("cuda", 0)
        B, G_, K = 4, cfg.DATASET.numGroupFrames, 14
        adc_h = torch.from_numpy(synth.adc_cube_int16(31, sensor=0, nframes=B * G_)).to(dev0)
        adc_v = torch.from_numpy(synth.adc_cube_int16(31, sensor=1, nframes=B * G_)).to(dev0)
        frac = torch.rand((B, K, 2), generator=torch.Generator().manual_seed(33))
        joints = (torch.from_numpy(synth.keypoints(B, 32)).float() + frac).to(dev0)
        e1 = TrainEngine(cfg, device=dev0, seed=0)
        st = e1.coord_stats()
        assert st["weight"] == LAM and st["sum"] == (0.0, 0.0) and st["steps"] == 0 and st["residual"] is None
        for _ in range(5):
            l1, _ = e1.train_step_from_adc(adc_h, adc_v, joints)
        e2 = TrainEngine(cfg, device=dev0, seed=0)
        for _ in range(2):
            e2.train_step_from_adc(adc_h, adc_v, joints)
        e2.capture(adc_h, adc_v, joints, warmup=1)                                          # the warm-up step is the third step
        for _ in range(2):
            l2, _ = e2.train_step_from_adc(adc_h, adc_v, joints)
        torch.cuda.synchronize()
        s1, s2 = e1.coord_stats(), e2.coord_stats()
        p1 = torch.cat([p.detach().flatten() for p in e1.model.parameters()])
        p2 = torch.cat([p.detach().flatten() for p in e2.model.parameters()])
        rel = ((p1 - p2).norm() / p1.norm()).item()
        print("after 5 steps: parameters rel %.3e, loss %.6f vs %.6f, coordinate sums %s vs %s" % (
            rel, float(l1.detach()), float(l2.detach()), s1["sum"], s2["sum"]))
        assert s1["steps"] == 5 and s2["steps"] == 5
        for a, b in zip(s1["sum"], s2["sum"]):
            assert np.isfinite(a) and a > 0 and abs(a - b) <= 1e-4 * abs(a)
        for s in (s1, s2):
            assert s["residual"].shape == (2, B, K, 2) and s["residual"].dtype == np.float32 and np.isfinite(s["residual"]).all()
        assert torch.isfinite(p2).all()
        assert rel <= 1e-5, rel
        assert abs(float(l1.detach()) - float(l2.detach())) <= 1e-4 * abs(float(l1.detach()))
    finally:
        F_.set_math("f32")


def test_engine_without_the_key_has_no_coord_stats():
    from hupr_amd.tools.engine import TrainEngine
    e = TrainEngine(_cfg(), device=torch.device("cuda", 0), seed=0)
    assert e.coord_stats() is None
    e.close()


# ---- 8: the Runner -----------------------------------------------------------------------------------------------------------------------
def _run_main(tmp_path, monkeypatch, name, **training):
    import yaml
    from hupr_amd import main as hmain
    from hupr_amd.config_tree import CONFIG_DIR
    cfgd = yaml.safe_load(open(os.path.join(CONFIG_DIR, "mscsa_prgcn.yaml")))
    cfgd["DATASET"]["dataDir"] = "synthetic"
    cfgd["TRAINING"].update(batchSize=2, epochs=1, **training)
    cfgd["TEST"]["batchSize"] = 2
    for d in ("config", "logs", "visualization"):
        (tmp_path / d).mkdir(exist_ok=True)
    yaml.safe_dump(cfgd, open(tmp_path / "config" / (name + ".yaml"), "w"))
    monkeypatch.chdir(tmp_path)
    hmain.main(["--config", name + ".yaml", "--dir", name, "--synthetic_length", "4", "--max_steps", "2"])
    return tmp_path / "logs" / name


def test_runner_prints_the_coordinate_loss_of_every_epoch(tmp_path, monkeypatch, capsys):
    run = _run_main(tmp_path, monkeypatch, "coord", coordLoss=LAM)
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if "Coordinate loss in epoch" in l]
    assert len(lines) == 1, out                                                             # one epoch, one line
    m = re.fullmatch(r"==========>Coordinate loss in epoch 0: first head (\d+\.\d{4})  PRGCN head (\d+\.\d{4}) heat-map px "
                     r"\(weight 0\.5, 2 steps\)", lines[0])
    assert m, lines[0]
    assert float(m.group(1)) >= 0 and float(m.group(2)) >= 0
    assert "AP: " in out and "MPJPE: " in out and os.path.exists(run / "checkpoint.pth")
    coord_keys = list(torch.load(run / "checkpoint.pth"))
    plain = _run_main(tmp_path, monkeypatch, "plain")
    out = capsys.readouterr().out
    assert "AP: " in out and "Coordinate loss" not in out and "MPJPE" not in out
    assert list(torch.load(plain / "checkpoint.pth")) == coord_keys                         # no new checkpoint keys
    with pytest.raises(ValueError) as e:
        _run_main(tmp_path, monkeypatch, "zero", coordLoss=0)
    assert "TRAINING.coordLoss" in str(e.value)
    assert not os.path.exists(tmp_path / "logs" / "zero" / "checkpoint.pth")               # before any step
