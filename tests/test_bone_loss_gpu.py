"""GPU (-m gpu): hupr_bone_loss_fwd_f32 / hupr_bone_loss_bwd_f32 (csrc/bone_loss.hip) against the fp64 statement of the rule in
include/hupr.h (``ref_bone`` in tests/bone_loss_ref.py; tests/test_bone_loss_cpu.py checks the reference itself), and every layer
built on them: ``functional.BoneLossFn``, ``LossComputer`` with ``TRAINING.boneLoss``, ``TrainEngine`` eager and captured, and the
Runner with its per-epoch line and its ``Bone error`` line.  Every raw launch writes into outputs pre-filled with NaN.

Inputs (``make_case``): before any comparison each test asserts in fp64 that |d| >= 50 (bound_u + bound_v) on both axes of every
valid bone, so no sign of d is decided by rounding and no bone is left out of a comparison.

Bounds.  resid against fp64: the coordinate loss's, |err| <= bound = 5e-6 (A + |r|) + 1e-7 with A = sum p |x - a| / (S + eps)
(tests/test_coord_loss_gpu.py: at most 64 sequential terms, 6 additions of the butterfly, 4 across the waves).  inv_den: 5e-6,
relative (the same sum S).  bone_resid: bound_u + bound_v + 1.2e-7 |d|, the two residuals' errors and the subtraction's rounding.
gcoef: the signs are exact by the margin, so what is left is the fp32 sum of at most 32 weights, 1e-6 of the summed incident |w_e|.
loss3: 1e-5 of its magnitude.  dp: per plane, 5e-5 of that plane's largest |dp| in fp64.  Zero planes: exactly zero."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from bone_loss_ref import (A0, A1, CASES, FACTOR, G, SKELETON0, STRIDE, bone_bound, bones_for, make_bone_weights, make_case, ref_bone,
                           sign_margin)
from test_coord_loss_cpu import ref_coord
from test_coord_loss_gpu import launch_fwd as coord_fwd

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def launch_fwd(p1, p2, joints, snap, bones, w=None, a0=1.0, a1=1.0, acc=None, stride=STRIDE, eps=1.0):
    """The C ABI on outputs pre-filled with NaN, so a value the kernels do not write shows.  p1, p2: (B, K, H, H) device tensors.
    -> loss3, resid (2, B, K, 2), inv_den (2, B, K), bone_resid (2, B, E, 2), gcoef (2, B, K, 2)."""
    from hupr_amd import runtime as rt
    B, K, H, _ = p1.shape
    E = len(bones)
    nan = lambda *shape: torch.full(shape, NAN, dtype=torch.float32, device="cuda")
    loss3, resid, inv_den, bone_resid, gcoef = nan(3), nan(2, B, K, 2), nan(2, B, K), nan(2, B, E, 2), nan(2, B, K, 2)
    table = (ctypes.c_int * (2 * E))(*[i for uv in bones for i in uv])
    rt.check(rt.lib().hupr_bone_loss_fwd_f32(rt.ptr(p1), rt.ptr(p2), rt.ptr(joints), B, K, H, stride, snap, table, E, rt.ptr(w), eps, a0, a1,
                                             rt.ptr(loss3), rt.ptr(resid), rt.ptr(inv_den), rt.ptr(bone_resid), rt.ptr(gcoef), rt.ptr(acc),
                                             rt.stream()))
    return loss3, resid, inv_den, bone_resid, gcoef


def launch_bwd(resid, inv_den, gcoef, joints, E, H, snap, g, a0=1.0, a1=1.0, stride=STRIDE):
    from hupr_amd import runtime as rt
    _, B, K = inv_den.shape
    dp1 = torch.full((B, K, H, H), NAN, dtype=torch.float32, device="cuda")
    dp2 = torch.full((B, K, H, H), NAN, dtype=torch.float32, device="cuda")
    gd = torch.tensor([g], dtype=torch.float32, device="cuda")
    rt.check(rt.lib().hupr_bone_loss_bwd_f32(rt.ptr(resid), rt.ptr(inv_den), rt.ptr(gcoef), rt.ptr(joints), rt.ptr(gd), B, K, E, H, stride,
                                             snap, a0, a1, rt.ptr(dp1), rt.ptr(dp2), rt.stream()))
    return dp1, dp2


def f64(x):
    return x.detach().cpu().numpy().astype(np.float64)


def check_forward(out, ref, what):
    """loss3, resid, inv_den, bone_resid, gcoef of one forward against ``ref_bone``, each within its bound of the module docstring."""
    loss3, resid, inv_den, bone_resid, gcoef = (f64(x) for x in out)
    err = np.abs(resid - ref["resid"])
    print("%s: resid max |err| %.3e, worst err / bound %.3f" % (what, err.max(), (err / ref["bound"]).max()))
    assert (err <= ref["bound"]).all() and not resid[:, ~ref["valid"]].any(), what
    assert np.array_equal(inv_den != 0, ref["inv_den"] != 0), what                              # invalid joints exactly
    err = np.abs(inv_den - ref["inv_den"])
    print("%s: inv_den worst relative err %.3e" % (what, (err / np.maximum(ref["inv_den"], 1e-300)).max()))
    assert (err <= 5e-6 * ref["inv_den"]).all(), what
    err = np.abs(bone_resid - ref["bone_resid"])
    bound = bone_bound(ref) + 1.2e-7 * np.abs(ref["bone_resid"])
    print("%s: bone_resid max |err| %.3e, worst err / bound %.3f" % (what, err.max(), (err / bound).max()))
    assert (err <= bound).all() and not bone_resid[:, ~ref["bone_valid"]].any(), what
    err = np.abs(gcoef - ref["gcoef"])
    print("%s: gcoef max |err| %.3e" % (what, err.max()))
    assert (err <= 1e-6 * ref["incident"][None, None, :, None]).all(), what
    check_loss3(loss3, ref["loss3"], what)


def check_loss3(got, ref3, what, tol=1e-5):
    got = f64(got) if isinstance(got, torch.Tensor) else got
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


@functools.lru_cache(maxsize=None)
def small_case(B, K, H):
    """make_case with the first seed of range(20) that leaves the margin with snap 0 and 1 (an AssertionError if none does)."""
    for seed in range(20):
        p1, p2, joints = make_case(B, K, H, seed, STRIDE)
        if all(sign_margin(ref_bone(p1, p2, joints, STRIDE, snap, bones_for(K))) >= FACTOR for snap in (0, 1)):
            return p1, p2, joints
    raise AssertionError("no seed in 0..19 leaves the margin at B%d K%d H%d" % (B, K, H))


# ---- 1: the kernels against the rule in fp64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("snap", [0, 1], ids=["float", "snap"])
@pytest.mark.parametrize("shape", list(CASES), ids=lambda s: "B%d-K%d-H%d" % s)
def test_kernels_against_fp64(shape, snap, weighted):
    B, K, H = shape
    p1, p2, joints = case(shape)
    bones = bones_for(K)
    E = len(bones)
    w = make_bone_weights(E) if weighted else None
    what = "B%d K%d H%d snap%d%s" % (B, K, H, snap, " weighted" if weighted else "")
    ref = ref_bone(p1, p2, joints, STRIDE, snap, bones, w, 1.0, A0, A1, G)
    assert ref["bone_valid"].all() and sign_margin(ref) >= FACTOR, (what, sign_margin(ref))
    d1, d2, dj, dw = dev(p1), dev(p2), dev(joints), (dev(w) if weighted else None)
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")
    out = launch_fwd(d1, d2, dj, snap, bones, dw, A0, A1, acc)
    check_forward(out, ref, what)
    first = acc.cpu().numpy().copy()
    assert first[2] == 1.0 and (np.abs(first[:2] - ref["loss3"][1:]) <= 1e-5 * ref["loss3"][1:]).all(), (what, first)
    launch_fwd(d1, d2, dj, snap, bones, dw, A0, A1, acc)
    second = acc.cpu().numpy()
    assert second[2] == 2.0 and (np.abs(second[:2] - 2 * first[:2]) <= 1e-12 * second[:2]).all(), (what, first, second)
    _, resid, inv_den, bone_resid, gcoef = out
    assert np.array_equal(np.sign(f64(bone_resid)), np.sign(ref["bone_resid"])), what          # the signs are exact by the margin
    dp1, dp2 = launch_bwd(resid, inv_den, gcoef, dj, E, H, snap, G, A0, A1)
    for h, dp in enumerate((dp1, dp2)):
        check_dp(dp, ref["dp"][h], "%s dp%d" % (what, h + 1))


# ---- 2: the residual is the coordinate loss's, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(CASES), ids=lambda s: "B%d-K%d-H%d" % s)
def test_residual_is_the_coordinate_loss_residual_bit_for_bit(shape):
    B, K, H = shape
    p1, p2, joints = (x.copy() for x in case(shape))
    joints[0, 0] = (NAN, 8.0)                                                                   # an invalid joint: zeros on both sides
    d1, d2, dj = dev(p1), dev(p2), dev(joints)
    for snap in (0, 1):
        for eps in (1.0, 0.25):
            _, resid, inv_den, _, _ = launch_fwd(d1, d2, dj, snap, bones_for(K), eps=eps)
            _, coord_resid, coord_scale = coord_fwd(d1, d2, dj, snap, eps=eps)
            assert torch.equal(resid.view(torch.int32), coord_resid.view(torch.int32)), (shape, snap, eps)
            assert not resid[:, 0, 0].any() and not inv_den[:, 0, 0].any() and int((inv_den > 0).sum()) == 2 * B * K - 2
            assert torch.allclose(inv_den, coord_scale, rtol=2e-7, atol=0)                      # 1 / den, unweighted, rounded once each


# ---- 3: invalid and degenerate joints ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("snap", [0, 1], ids=["float", "snap"])
@pytest.mark.parametrize("H", [8, 5], ids=["H8", "H5"])
def test_invalid_joints_silence_their_bones(H, snap):
    """Joints that are NaN, +inf, negative or past (H - 1) * stride, over NaN-filled planes (which are not read): their bones report
    zero and add nothing to the coefficient of the joint at the other end; every untouched bone keeps its bits against a clean
    run; the loss is finite and, the denominator being fixed, smaller than the clean one."""
    B, K = 2, 14
    p1, p2, joints = (x.copy() for x in small_case(B, K, H))
    bones, E = SKELETON0, len(SKELETON0)
    d1c, d2c = dev(p1), dev(p2)
    clean = launch_fwd(d1c, d2c, dev(joints), snap, bones, None, A0, A1)
    bad = {(0, 1): (NAN, 8.0), (0, 4): (8.0, INF), (1, 0): (-8.0, 8.0), (1, 2): (8.0, (H - 1) * STRIDE + 8.0), (1, 5): (NAN, NAN)}
    for (b, j), xy in bad.items():
        joints[b, j] = xy
        p1[b, j] = NAN
        p2[b, j] = NAN
    ref = ref_bone(p1, p2, joints, STRIDE, snap, bones, None, 1.0, A0, A1, G)
    assert (~ref["valid"]).sum() == len(bad) and sign_margin(ref) >= FACTOR
    dead = ~ref["bone_valid"]
    assert dead.sum() == 8 and dead[1, 12] and dead[1, 11] and dead[1, 7]                       # (1, 0), (2, 1), (6, 0) of sample 1, ...
    dj = dev(joints)
    out = launch_fwd(dev(p1), dev(p2), dj, snap, bones, None, A0, A1)
    what = "invalid H%d snap%d" % (H, snap)
    check_forward(out, ref, what)
    loss3, resid, inv_den, bone_resid, gcoef = out
    kt, bt = torch.from_numpy(ref["valid"]).cuda(), torch.from_numpy(ref["bone_valid"]).cuda()
    assert not resid[:, ~kt].any() and not inv_den[:, ~kt].any() and not gcoef[:, ~kt].any() and not bone_resid[:, ~bt].any()
    assert torch.equal(resid[:, kt], clean[1][:, kt]) and torch.equal(inv_den[:, kt], clean[2][:, kt])
    assert torch.equal(bone_resid[:, bt], clean[3][:, bt])
    # sample 1, joint 1 (R_Knee) sits between the invalid joints 0 and 2: nothing is left of its coefficient; joint 6 (Neck) of
    # sample 1 lost bone 7 = (6, 0), where it is u and carried - sgn(d), and keeps the other three (unit weights: exact integers)
    assert not gcoef[:, 1, 1].any() and (gcoef[:, 1, 6] != 0).all()
    assert torch.equal(gcoef[:, 1, 6], clean[4][:, 1, 6] + torch.sign(clean[3][:, 1, 7]))
    assert torch.isfinite(loss3).all() and (loss3[1:] < clean[0][1:]).all()
    dp1, dp2 = launch_bwd(resid, inv_den, gcoef, dj, E, H, snap, G, A0, A1)
    for h, dp in enumerate((dp1, dp2)):
        check_dp(dp, ref["dp"][h], "%s dp%d" % (what, h + 1))
        assert not dp[~kt].any() and not dp[1, 1].any()


# ---- 4, 5: an empty plane and a NaN cell ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [8, 5], ids=["H8", "H5"])
def test_empty_plane_and_nan_cell(H):
    B, K = 2, 14
    bones, E = SKELETON0, len(SKELETON0)
    p1, p2, joints = (x.copy() for x in small_case(B, K, H))
    d2, dj = dev(p2), dev(joints)
    clean = launch_fwd(dev(p1), d2, dj, 0, bones, None, A0, A1)
    # an all-zero plane under a valid joint (sample 1, joint 3): r = 0 exactly, 1 / den = 1, everything stays finite
    p1[1, 3] = 0.0
    loss3, resid, inv_den, bone_resid, gcoef = launch_fwd(dev(p1), d2, dj, 0, bones, None, A0, A1)
    assert not resid[0, 1, 3].any() and inv_den[0, 1, 3].item() == 1.0
    assert all(torch.isfinite(x).all() for x in (loss3, resid, inv_den, bone_resid, gcoef))
    touched = torch.tensor([3 in uv for uv in bones], device="cuda")                            # (6, 3) and (4, 3)
    keep = torch.ones((2, B, E), dtype=torch.bool, device="cuda")
    keep[0, 1] = ~touched
    assert torch.equal(bone_resid[keep], clean[3][keep])
    assert torch.equal(bone_resid[0, 1, 8], resid[0, 1, 3] - resid[0, 1, 6]) and torch.equal(bone_resid[0, 1, 10], resid[0, 1, 3] - resid[0, 1, 4])
    dp1, dp2 = launch_bwd(resid, inv_den, gcoef, dj, E, H, 0, G, A0, A1)
    assert torch.isfinite(dp1).all() and torch.isfinite(dp2).all() and torch.equal(loss3[2], clean[0][2])
    # one NaN cell in a valid plane of head 0 (sample 0, joint 2, whose only bone is (2, 1)): not masked
    p1[0, 2, H // 2, 1] = NAN
    loss3, resid, inv_den, bone_resid, gcoef = launch_fwd(dev(p1), d2, dj, 0, bones, None, A0, A1)
    assert torch.isnan(loss3[0]) and torch.isnan(loss3[1]) and torch.isfinite(loss3[2]) and torch.equal(loss3[2], clean[0][2])
    assert torch.isnan(resid[0, 0, 2]).all() and torch.isnan(inv_den[0, 0, 2]) and int(torch.isnan(resid).sum()) == 2
    assert torch.isnan(bone_resid[0, 0, 11]).all() and int(torch.isnan(bone_resid).sum()) == 2
    keep[0, 0, 11] = False
    assert torch.equal(bone_resid[keep], clean[3][keep])
    assert torch.isnan(gcoef[0, 0, 2]).all() and torch.isnan(gcoef[0, 0, 1]).all() and int(torch.isnan(gcoef).sum()) == 4
    dp1, dp2 = launch_bwd(resid, inv_den, gcoef, dj, E, H, 0, G, A0, A1)
    # the NaN reaches the planes of the joint itself and of joint 1, which shares the bone, and no others; the other head stays finite
    assert torch.isnan(dp1[0, 2]).all() and torch.isnan(dp1[0, 1]).all() and int(torch.isnan(dp1).sum()) == 2 * H * H
    assert torch.isfinite(dp2).all()


# ---- 6: a pose displaced as a whole costs nothing ------------------------------------------------------------------------------------------
def test_a_common_shift_costs_no_bone_loss():
    """The sub-pixel targets of all 14 joints of a sample, displaced by one whole-pixel offset per sample (3 or 4 px per axis,
    either sign) and used as predictions.  The joints are at least 10.5 heat-map px from every border, so no 13 x 13 window is
    clipped before or after the shift.  Every residual is then the shift times S / (S + eps) plus at most the 0.01 px that
    tests/test_coord_loss_gpu.py::test_targets_as_predictions_leave_no_residual allows, so a bone's error is at most 0.02 px and
    so is their weighted mean, while the coordinate loss of the same inputs sees the shift: at least 2 px."""
    from hupr_amd import functional as F_
    B, K, H = 8, 14, 64
    rng = np.random.RandomState(21)
    joints = rng.uniform(10.5, H - 1 - 10.5, (B, K, 2)) * STRIDE
    shift = rng.choice([-4.0, -3.0, 3.0, 4.0], (B, 1, 2))
    t = F_.gaussian_targets_subpixel(dev(joints + shift * STRIDE), H, int(H * STRIDE), 2)
    dj = dev(joints)
    loss3, resid, inv_den, bone_resid, gcoef = launch_fwd(t, t, dj, 0, SKELETON0)
    coord3, _, _ = coord_fwd(t, t, dj, 0)
    print("common shift: bone loss %s, largest |d| %.3e, coordinate loss %s" % (f64(loss3), bone_resid.abs().max().item(), f64(coord3)))
    assert (inv_den > 0).all() and torch.isfinite(bone_resid).all()
    assert (resid.abs().amin(dim=(1, 2, 3)) >= 2.5).all()                                      # every centroid is off by the shift
    assert (loss3[1:] <= 0.02).all() and loss3[0] <= 0.04 and bone_resid.abs().max() <= 0.02
    assert (coord3[1:] >= 2.0).all()


# ---- 7: run to run -----------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_equal_bits():
    shape = (3, 14, 64)
    p1, p2, joints = (x.copy() for x in case(shape))
    for x in (p1, p2, joints):                                                                  # equal planes with equal joints
        x[1, 9] = x[1, 4]
        x[2, 11] = x[0, 2]
    d1, d2, dj, dw = dev(p1), dev(p2), dev(joints), dev(make_bone_weights(13))
    outs = []
    for _ in range(2):
        acc = torch.zeros(3, dtype=torch.float64, device="cuda")
        out = launch_fwd(d1, d2, dj, 0, SKELETON0, dw, A0, A1, acc)
        dp1, dp2 = launch_bwd(out[1], out[2], out[4], dj, 13, 64, 0, G, A0, A1)
        outs.append(out + (acc, dp1, dp2))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                           b.view(torch.int64 if b.dtype == torch.float64 else torch.int32))
    rb, sb = outs[0][1].view(torch.int32), outs[0][2].view(torch.int32)
    for h in range(2):
        assert torch.equal(rb[h, 1, 9], rb[h, 1, 4]) and torch.equal(rb[h, 2, 11], rb[h, 0, 2])
        assert sb[h, 1, 9].item() == sb[h, 1, 4].item() and sb[h, 2, 11].item() == sb[h, 0, 2].item()
    assert not torch.equal(rb[0, 1, 9], rb[0, 1, 5])


# ---- 8: the Function ---------------------------------------------------------------------------------------------------------------------
def test_function_is_the_raw_launches_bit_for_bit():
    from hupr_amd import functional as F_
    shape = (3, 14, 64)
    B, K, H = shape
    p1, p2, joints = case(shape)
    chain = tuple((j, j + 1) for j in range(K - 1))
    d1, d2, dj, dw = dev(p1), dev(p2), dev(joints), dev(make_bone_weights(13))
    for snap, bones, w, jt in ((0, None, None, dj), (1, SKELETON0, dw, dj.double()), (0, [list(uv) for uv in chain], dw, dj)):
        table = SKELETON0 if bones is None else tuple(tuple(uv) for uv in bones)
        acc_raw, acc_fn = (torch.zeros(3, dtype=torch.float64, device="cuda") for _ in range(2))
        loss3, resid, inv_den, bone_resid, gcoef = launch_fwd(d1, d2, dj, snap, table, w, A0, A1, acc_raw)
        dp1, dp2 = launch_bwd(resid, inv_den, gcoef, dj, 13, H, snap, G, A0, A1)
        a1, a2 = d1.clone().requires_grad_(True), d2.clone().requires_grad_(True)
        n0 = F_.rt.lib().hupr_launch_count()
        loss, heads = F_.BoneLossFn.apply(a1, a2, jt, STRIDE, bool(snap), bones, w, A0, A1, acc_fn)
        (G * loss).backward()
        assert F_.rt.lib().hupr_launch_count() - n0 <= 3
        assert torch.equal(loss.detach(), loss3[0]) and torch.equal(heads, loss3[1:]) and not heads.requires_grad
        assert torch.equal(a1.grad, dp1) and torch.equal(a2.grad, dp2) and torch.equal(acc_raw, acc_fn)
        res = F_.BoneLossFn.last_residual
        assert torch.equal(res, bone_resid) and not res.requires_grad and tuple(res.shape) == (2, B, 13, 2)
    # what it cannot run raises; there is no fallback
    a1 = d1.clone().requires_grad_(True)
    ok = (a1, d2, dj, STRIDE, False, None, None, 1.0, 1.0, None)
    F_.BoneLossFn.apply(*ok)

    def but(**kw):
        names = ("p1", "p2", "joints", "stride", "snap", "bones", "bone_w", "a0", "a1", "acc")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))
    for args in (but(p2=d2[:, :7]), but(p2=d2.double()), but(p2=d2.cpu()), but(p1=d1.half(), p2=d2.half()), but(p2=d2[..., :32]),
                 but(p1=d1.reshape(B, K, -1), p2=d2.reshape(B, K, -1)), but(p2=p2), but(p1=d1[:, :13], p2=d2[:, :13], joints=dj[:, :13]),
                 but(joints=dj.cpu()), but(joints=dj[:, :7]), but(joints=dj.reshape(B, 2, K)), but(joints=dj > 0), but(joints=joints),
                 but(stride=0.0), but(stride=-4.0), but(stride=NAN), but(stride="4"),
                 but(bones=[]), but(bones=[(0, 14)]), but(bones=[(2, 2)]), but(bones=[(0, 1)] * 33), but(bones=[(0, 1.0)]), but(bones=7),
                 but(bone_w=torch.ones(13)), but(bone_w=torch.ones(14, device="cuda")),
                 but(bone_w=torch.ones(13, device="cuda", dtype=torch.float64)),
                 but(acc=torch.zeros(3, dtype=torch.float32, device="cuda")), but(acc=torch.zeros(4, dtype=torch.float64, device="cuda")),
                 but(acc=torch.zeros(3, dtype=torch.float64))):
        with pytest.raises(ValueError):
            F_.BoneLossFn.apply(*args)


# ---- 9: LossComputer -----------------------------------------------------------------------------------------------------------------------
def _cfg(**training):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    for k, v in training.items():
        setattr(cfg.TRAINING, k, v)
    return cfg


JOINT_W = [1.0, 1.0, 1.5, 1.0, 1.0, 1.5, 0.0, 0.5, 1.0, 2.0, 2.5, 1.0, 2.0, 2.5]
MU = 0.5


def _loss_inputs(lc, w, B=2):
    """Integer joints, the targets LossComputer forms from them and predictions around them with a per-plane noise level (the
    inputs of tests/test_coord_loss_gpu.py); the first seed of range(20) that leaves the bone margin."""
    from hupr_amd import synth
    K, H = 14, 64
    for seed in range(20):
        joints = torch.from_numpy(synth.keypoints(B, 40 + seed))
        T = lc.targets(joints.cuda()).cpu().numpy().reshape(B, K, H * H)
        rng = np.random.RandomState(50 + seed)
        a = np.stack([rng.permutation(np.linspace(0.05, 0.6, K)) for _ in range(B)])
        p = [np.clip(T + s * a[..., None] * rng.uniform(-1.0, 1.0, T.shape), 1e-4, 1.0 - 1e-4).astype(np.float32) for s in (1.0, 0.8)]
        bone = ref_bone(p[0].reshape(B, K, H, H), p[1].reshape(B, K, H, H), joints.numpy(), STRIDE, 1, SKELETON0, w, 1.0, MU, MU, 1.0)
        if bone["bone_valid"].all() and sign_margin(bone) >= FACTOR:
            return joints, p[0], p[1], bone
    raise AssertionError("no seed in 0..19 leaves the margin")


def _run_loss(lc, joints, p1, p2, B=2, K=14, H=64):
    a1 = dev(p1).reshape(B, K, 1, H, H).requires_grad_(True)
    a2 = dev(p2).reshape(B, 1, K, H, H).requires_grad_(True)
    loss, loss2, _, _ = lc.computeLoss((a1, a2), joints.cuda(), decode="device")
    loss.backward()
    return loss.detach(), loss2.detach(), a1.grad.reshape(B, K, H, H), a2.grad.reshape(B, K, H, H)


@pytest.mark.parametrize("setting", ["plain", "weights", "ohkm", "coord"])
def test_loss_computer_adds_the_bone_term(setting):
    """loss and both gradients = the same LossComputer without the key on the same inputs + 0.5 times the fp64 bone term over all
    13 bones (whatever ``ohkm`` keeps; with ``jointWeights`` a bone weighs sqrt(w_u w_v)), within the kernels' bounds plus the
    heat-map loss's 1e-6; loss2 stays the second head's BCE bit for bit."""
    from hupr_amd.misc.losses import LossComputer, bone_weights
    B, K, H = 2, 14, 64
    training = dict(plain={}, weights=dict(jointWeights=JOINT_W), ohkm=dict(ohkm=8), coord=dict(coordLoss=0.25))[setting]
    cfg = _cfg(boneLoss=MU, **training)
    assert cfg.TRAINING.lossDecay == -1 and not hasattr(cfg.TRAINING, "targets")           # head weights (1, 1); integer targets: snap
    lc, base = LossComputer(cfg, "cuda"), LossComputer(_cfg(**training), "cuda")
    assert lc.boneLoss == MU and base.boneLoss is None and lc.bone_residual is None and lc.bones == SKELETON0
    w = np.array(bone_weights(JOINT_W, SKELETON0)) if setting == "weights" else None
    joints, p1, p2, bone = _loss_inputs(lc, w)
    loss, loss2, g1, g2 = _run_loss(lc, joints, p1, p2)
    bl, bl2, bg1, bg2 = _run_loss(base, joints, p1, p2)
    assert base.bone_residual is None and torch.equal(loss2, bl2)
    heat, heat_dp = float(bl), np.stack([f64(bg1), f64(bg2)])
    want = heat + bone["loss3"][0]
    print("%s: loss %.7f vs %.7f (without the key %.7f + bone %.7f)" % (setting, float(loss), want, heat, bone["loss3"][0]))
    assert abs(float(loss) - want) <= 1e-6 * abs(heat) + 1e-5 * abs(bone["loss3"][0])
    for h, g in enumerate((g1, g2)):
        check_dp(f64(g) - heat_dp[h], bone["dp"][h], "%s dpreds%d" % (setting, h + 1), extra=1e-6 * np.abs(heat_dp[h]).max())
    err = np.abs(f64(lc.bone_residual) - bone["bone_resid"])
    assert (err <= bone_bound(bone) + 1.2e-7 * np.abs(bone["bone_resid"])).all()
    assert not lc.bone_residual.requires_grad and tuple(lc.bone_residual.shape) == (2, B, 13, 2)
    if setting == "weights":                                                                    # joint 6 (Neck) weighs 0: its four bones
        assert lc._bone_w.tolist() == w.tolist() and (lc._bone_w == 0).sum().item() == 4
    if setting == "coord":
        assert lc.coord_acc[2].item() == 1.0 and base.coord_acc[2].item() == 1.0
    acc = lc.bone_acc.cpu().numpy()                                                             # B_h itself, before mu
    assert acc[2] == 1.0 and (np.abs(acc[:2] - bone["loss3"][1:]) <= 1e-5 * bone["loss3"][1:]).all(), acc
    # evaluation shows the trained loss and does not move the accumulator
    a1, a2 = dev(p1).reshape(B, K, 1, H, H), dev(p2).reshape(B, 1, K, H, H)
    with torch.no_grad():
        le, le2, _, _ = lc.computeLoss((a1, a2), joints.cuda(), decode=False)
    assert torch.equal(le, loss) and torch.equal(le2, loss2)
    assert np.array_equal(lc.bone_acc.cpu().numpy(), acc)
    lc.computeLoss((a1, a2), joints.cuda(), decode=False)                                       # gradients enabled: it counts
    assert lc.bone_acc[2].item() == 2.0


def test_loss_computer_without_the_key_is_the_pair_loss():
    from hupr_amd import functional as F_
    from hupr_amd.misc.losses import LossComputer
    B, K, H = 2, 14, 64
    for training in ({}, dict(boneLoss=-1)):
        lc = LossComputer(_cfg(**training), "cuda")
        assert lc.boneLoss is None and lc.bone_acc is None and "computeLoss" not in vars(lc)   # today's method object
        joints, p1, p2, _ = _loss_inputs(lc, None)
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
        assert moved == F_.rt.lib().hupr_launch_count() - n0                                   # today's launches (the targets count once each)
        assert torch.equal(loss, ref) and torch.equal(loss2, ref2)
        assert torch.equal(a1.grad.reshape(b1.shape), b1.grad) and torch.equal(a2.grad.reshape(b2.shape), b2.grad)
        assert lc.bone_residual is None


# ---- 10: the engine, eager and captured ------------------------------------------------------------------------------------------------------
def test_graph_replay_matches_eager_steps_with_the_bone_loss():
    """tests/test_coord_loss_gpu.py::test_graph_replay_matches_eager_steps_with_the_coordinate_loss at its size (B = 4, bf16) and with
    its bounds, with ``TRAINING.boneLoss: 0.5`` and ``TRAINING.targets: subpixel``: five eager steps against 2 eager + capture
    (1 warm-up step) + 2 replays.  The accumulator replays with the step: both engines have counted five steps, and their sums agree."""
    from hupr_amd import functional as F_, synth
    from hupr_amd.tools.engine import TrainEngine
    try:
        F_.set_math("bf16")
        cfg = _cfg(boneLoss=MU, targets="subpixel")
        dev0 = torch.device("cuda", 0)
        B, G_, K = 4, cfg.DATASET.numGroupFrames, 14
        adc_h = torch.from_numpy(synth.adc_cube_int16(31, sensor=0, nframes=B * G_)).to(dev0)
        adc_v = torch.from_numpy(synth.adc_cube_int16(31, sensor=1, nframes=B * G_)).to(dev0)
        frac = torch.rand((B, K, 2), generator=torch.Generator().manual_seed(33))
        joints = (torch.from_numpy(synth.keypoints(B, 32)).float() + frac).to(dev0)
        e1 = TrainEngine(cfg, device=dev0, seed=0)
        st = e1.bone_stats()
        assert st["weight"] == MU and st["sum"] == (0.0, 0.0) and st["steps"] == 0 and st["residual"] is None
        assert e1.coord_stats() is None
        for _ in range(5):
            l1, _ = e1.train_step_from_adc(adc_h, adc_v, joints)
        e2 = TrainEngine(cfg, device=dev0, seed=0)
        for _ in range(2):
            e2.train_step_from_adc(adc_h, adc_v, joints)
        e2.capture(adc_h, adc_v, joints, warmup=1)                                          # the warm-up step is the third step
        for _ in range(2):
            l2, _ = e2.train_step_from_adc(adc_h, adc_v, joints)
        torch.cuda.synchronize()
        s1, s2 = e1.bone_stats(), e2.bone_stats()
        p1 = torch.cat([p.detach().flatten() for p in e1.model.parameters()])
        p2 = torch.cat([p.detach().flatten() for p in e2.model.parameters()])
        rel = ((p1 - p2).norm() / p1.norm()).item()
        print("after 5 steps: parameters rel %.3e, loss %.6f vs %.6f, bone sums %s vs %s" % (
            rel, float(l1.detach()), float(l2.detach()), s1["sum"], s2["sum"]))
        assert s1["steps"] == 5 and s2["steps"] == 5
        for a, b in zip(s1["sum"], s2["sum"]):
            assert np.isfinite(a) and a > 0 and abs(a - b) <= 1e-4 * abs(a)
        for s in (s1, s2):
            assert s["residual"].shape == (2, B, 13, 2) and s["residual"].dtype == np.float32 and np.isfinite(s["residual"]).all()
        assert torch.isfinite(p2).all()
        assert rel <= 1e-5, rel
        assert abs(float(l1.detach()) - float(l2.detach())) <= 1e-4 * abs(float(l1.detach()))
    finally:
        F_.set_math("f32")


def test_engine_without_the_key_has_no_bone_stats():
    from hupr_amd.tools.engine import TrainEngine
    e = TrainEngine(_cfg(), device=torch.device("cuda", 0), seed=0)
    assert e.bone_stats() is None
    e.close()


# ---- 11: the Runner ----------------------------------------------------------------------------------------------------------------------
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


def test_runner_prints_the_bone_loss_of_every_epoch(tmp_path, monkeypatch, capsys):
    run = _run_main(tmp_path, monkeypatch, "bone", boneLoss=MU)
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if "Bone loss in epoch" in l]
    assert len(lines) == 1, out                                                             # one epoch, one line
    m = re.fullmatch(r"==========>Bone loss in epoch 0: first head (\d+\.\d{4})  PRGCN head (\d+\.\d{4}) heat-map px "
                     r"\(weight 0\.5, 2 steps\)", lines[0])
    assert m, lines[0]
    assert float(m.group(1)) >= 0 and float(m.group(2)) >= 0
    assert "AP: " in out and "MPJPE: " in out and os.path.exists(run / "checkpoint.pth")
    errs = [l for l in out.splitlines() if l.startswith("Bone error: ")]
    assert errs and all(re.fullmatch(r"Bone error: \d+\.\d{3} px \(n = \d+\)", l) for l in errs), out
    assert "Coordinate loss" not in out
    bone_keys = list(torch.load(run / "checkpoint.pth"))
    plain = _run_main(tmp_path, monkeypatch, "plain")
    out = capsys.readouterr().out
    assert "AP: " in out and "Bone loss" not in out and "MPJPE" not in out and "Bone error" not in out
    assert list(torch.load(plain / "checkpoint.pth")) == bone_keys                          # no new checkpoint keys
    with pytest.raises(ValueError) as e:
        _run_main(tmp_path, monkeypatch, "zero", boneLoss=0)
    assert "TRAINING.boneLoss" in str(e.value)
    assert not os.path.exists(tmp_path / "logs" / "zero" / "checkpoint.pth")               # before any step
