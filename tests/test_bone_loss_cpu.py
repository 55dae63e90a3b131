"""CPU (-m "not gpu"): the bone-vector loss at every layer short of a launch — ``TRAINING.boneLoss`` where the config is read, the
skeleton table, ``misc.oks_eval.mean_bone_error``, the argument checks of hupr_bone_loss_fwd_f32 / hupr_bone_loss_bwd_f32 through
ctypes, ``functional.BoneLossFn``'s refusals, the register / scratch metadata of csrc/bone_loss.hip — and the fp64 statement of the
rule (``ref_bone`` in tests/bone_loss_ref.py) that tests/test_bone_loss_gpu.py compares the kernels with.  The rule is new, so the
reference is its own statement; it is checked here against torch's fp64 autograd of the same forward and on hand-built planes.
The sign margin the GPU cases rely on is asserted here too, so the seeds they fix can be checked without a GPU."""
import ctypes
import re

import numpy as np
import pytest
import torch

from bone_loss_ref import (A0, A1, CASES, FACTOR, G, SKELETON0, STRIDE, bone_bound, bones_for, make_bone_weights, make_case, ref_bone,
                           ref_position, sign_margin)
from listing import kernel_metadata

NAN, INF = float("nan"), float("inf")


# ---- the sign margin of the GPU cases ----------------------------------------------------------------------------------------------------
def test_the_fixed_seeds_leave_no_sign_to_rounding():
    """|d| >= 50 (bound_u + bound_v) on both axes of every bone of both heads, with snap 0 and 1: no sign of d is decided by an fp32
    residual's rounding, and no bone is left out of a comparison."""
    for (B, K, H), seed in CASES.items():
        p1, p2, joints = make_case(B, K, H, seed, STRIDE)
        for snap in (0, 1):
            ref = ref_bone(p1, p2, joints, STRIDE, snap, bones_for(K))
            assert ref["valid"].all() and ref["bone_valid"].all(), ((B, K, H), snap)
            d, bound = np.abs(ref["bone_resid"]), bone_bound(ref)
            print("B%d K%d H%d seed %d snap %d: smallest |d| %.4g, largest joint bound %.2g, margin %.1f" % (
                B, K, H, seed, snap, d.min(), ref["bound"].max(), sign_margin(ref)))
            assert (d >= FACTOR * bound).all(), ((B, K, H), seed, snap, sign_margin(ref))


# ---- the reference's own properties ------------------------------------------------------------------------------------------------------
def autograd_bone(p1, p2, joints, stride, snap, bones, w=None, eps=1.0, a0=1.0, a1=1.0, g=1.0):
    """The same forward written in torch fp64 -> (loss3[0], its gradient times g with respect to both maps (2, B, K, H, H))."""
    p = torch.from_numpy(np.stack([np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)])).requires_grad_(True)
    _, B, K, H, _ = p.shape
    a, valid = ref_position(joints, stride, snap, H)
    a, valid = torch.from_numpy(np.where(valid[..., None], a, 0.0)), torch.from_numpy(valid)
    uv = torch.tensor(bones, dtype=torch.int64).reshape(-1, 2)
    E = len(uv)
    wv = torch.ones(E, dtype=torch.float64) if w is None else torch.from_numpy(np.asarray(w, dtype=np.float64))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(H, dtype=torch.float64), indexing="ij")
    pm = torch.where(valid[None, :, :, None, None], p, torch.zeros_like(p))
    den = pm.sum(dim=(-1, -2)) + eps
    r = torch.stack([(pm * (xs - a[..., 0, None, None])).sum(dim=(-1, -2)) / den,
                     (pm * (ys - a[..., 1, None, None])).sum(dim=(-1, -2)) / den], dim=-1)                  # (2, B, K, 2)
    ok = (valid[:, uv[:, 0]] & valid[:, uv[:, 1]])[None, :, :, None]
    d = torch.where(ok, r[:, :, uv[:, 1]] - r[:, :, uv[:, 0]], torch.zeros(1, dtype=torch.float64))
    Bh = (wv[None, None, :, None] * d.abs()).sum(dim=(1, 2, 3)) / (2 * B * E)
    loss = a0 * Bh[0] + a1 * Bh[1]
    (g * loss).backward()
    return loss.item(), p.grad.numpy()


@pytest.mark.parametrize("shape", list(CASES), ids=lambda s: "B%d-K%d-H%d" % s)
def test_reference_backward_is_the_gradient_of_its_forward(shape):
    """The analytic dp of ref_bone against torch's fp64 autograd of the same forward: with and without snap and bone weights, and
    with an invalid joint, whose bones drop out of both."""
    B, K, H = shape
    p1, p2, joints = make_case(B, K, H, CASES[shape], STRIDE)
    bones = bones_for(K)
    broken = joints.copy()
    broken[0, K - 1] = (NAN, 8.0)
    for snap in (0, 1):
        for w in (None, make_bone_weights(len(bones))):
            for jt in (joints, broken):
                ref = ref_bone(p1, p2, jt, STRIDE, snap, bones, w, 1.0, A0, A1, G)
                loss, grad = autograd_bone(p1, p2, jt, STRIDE, snap, bones, w, 1.0, A0, A1, G)
                assert np.isclose(ref["loss3"][0], loss, rtol=1e-13, atol=1e-300)
                assert np.allclose(ref["dp"], grad, rtol=1e-9, atol=1e-18), np.abs(ref["dp"] - grad).max()
            assert not ref["dp"][:, 0, K - 1].any() and not ref["gcoef"][:, 0, K - 1].any() and not ref["inv_den"][:, 0, K - 1].any()


def test_reference_on_hand_built_planes():
    """Two planes that are one-hot at known cells: with eps -> 0, d = (c_v - c_u) - (a_v - a_u).  Then the fixed denominator, the
    weights, the coefficients of a three-joint chain, an invalid joint, the accumulator and a common shift."""
    H, stride = 8, 4.0
    p = np.zeros((1, 2, H, H))
    p[0, 0, 2, 1] = 0.7                                                             # c_0 = (x, y) = (1, 2)
    p[0, 1, 5, 6] = 0.4                                                             # c_1 = (6, 5)
    joints = np.array([[[6.0, 10.0], [22.0, 14.0]]])                                # a_0 = (1.5, 2.5), a_1 = (5.5, 3.5)
    r = ref_bone(p, p, joints, stride, 0, [(0, 1)], eps=1e-12)
    want = (np.array([6.0, 5.0]) - np.array([1.0, 2.0])) - (np.array([5.5, 3.5]) - np.array([1.5, 2.5]))     # (1, 2)
    assert np.allclose(r["bone_resid"][0, 0, 0], want, rtol=1e-11) and np.allclose(r["bone_resid"][1], r["bone_resid"][0])
    assert np.allclose(r["loss3"], [2 * 3.0 / 2, 3.0 / 2, 3.0 / 2], rtol=1e-11)    # (|1| + |2|) / (2 B E) with B = E = 1
    assert r["gcoef"][0, 0].tolist() == [[-1.0, -1.0], [1.0, 1.0]]                  # d > 0: + at v = 1, - at u = 0
    # eps = 1: each residual shrinks by S / (S + 1)
    r = ref_bone(p, p, joints, stride, 0, [(0, 1)], eps=1.0)
    r0, r1 = 0.7 / 1.7 * np.array([-0.5, -0.5]), 0.4 / 1.4 * np.array([0.5, 1.5])
    assert np.allclose(r["resid"][0, 0], [r0, r1], rtol=1e-14) and np.allclose(r["bone_resid"][0, 0, 0], r1 - r0, rtol=1e-14)
    assert np.allclose(r["inv_den"][0, 0], [1 / 1.7, 1 / 1.4], rtol=1e-15)
    # the backward at plane 0's own cell: f (gcoef_x (x - a_x - r_x) + gcoef_y (y - a_y - r_y)), f = 1 / 1.7 / 2
    want = (1 / 1.7 / 2) * (-1.0 * (1 - 1.5 - r0[0]) + -1.0 * (2 - 2.5 - r0[1]))
    assert np.isclose(r["dp"][0, 0, 0, 2, 1], want, rtol=1e-14)
    # a chain of three with weights: joint 1 is v of bone 0 and u of bone 1; the invalid joint 2 silences bone 1 only
    q = np.zeros((1, 3, H, H))
    q[0, 0, 2, 1], q[0, 1, 5, 6], q[0, 2, 1, 1] = 0.7, 0.4, 0.9
    j3 = np.array([[[6.0, 10.0], [22.0, 14.0], [8.0, 8.0]]])
    w = np.array([2.0, 3.0])
    c = ref_bone(q, 2 * q, j3, stride, 0, [(0, 1), (1, 2)], w, eps=1.0, a0=0.25, a1=2.0, calls=3)
    d = c["bone_resid"][0, 0]
    assert (d[0] > 0).all() and (d[1] < 0).all()
    assert c["gcoef"][0, 0].tolist() == [[-2.0, -2.0], [2.0 + 3.0, 2.0 + 3.0], [-3.0, -3.0]]
    assert c["incident"].tolist() == [2.0, 5.0, 3.0]
    B0 = (2.0 * np.abs(d[0]).sum() + 3.0 * np.abs(d[1]).sum()) / 4                  # 2 B E = 4
    assert np.isclose(c["loss3"][1], B0, rtol=1e-14) and np.isclose(c["loss3"][0], 0.25 * B0 + 2.0 * c["loss3"][2], rtol=1e-14)
    assert np.allclose(c["acc"], [3 * B0, 3 * c["loss3"][2], 3.0], rtol=1e-14)
    q[0, 2] = NAN
    j3[0, 2] = (8.0, -8.0)
    k = ref_bone(q, 2 * q, j3, stride, 0, [(0, 1), (1, 2)], w, eps=1.0)
    assert k["bone_valid"].tolist() == [[True, False]] and not k["bone_resid"][:, 0, 1].any() and not k["dp"][:, 0, 2].any()
    assert np.array_equal(k["bone_resid"][:, 0, 0], c["bone_resid"][:, 0, 0])
    assert k["gcoef"][0, 0].tolist() == [[-2.0, -2.0], [2.0, 2.0], [0.0, 0.0]]
    assert np.isclose(k["loss3"][1], 2.0 * np.abs(d[0]).sum() / 4, rtol=1e-14) and np.isfinite(k["dp"]).all()
    # a NaN cell is not masked: it reaches both joints of its bones
    q[0, 2] = 0.0
    q[0, 0, 0, 0] = NAN
    j3[0, 2] = (8.0, 8.0)
    n = ref_bone(q, np.nan_to_num(q), j3, stride, 0, [(0, 1), (1, 2)], w)
    assert np.isnan(n["loss3"][:2]).all() and np.isfinite(n["loss3"][2])
    assert np.isnan(n["dp"][0, 0, 0]).all() and np.isnan(n["dp"][0, 0, 1]).all() and np.isfinite(n["dp"][0, 0, 2]).all()
    assert np.isfinite(n["dp"][1]).all()
    # every joint displaced by the same whole offset: the same d (up to the planes' equal shrink), so no cost where r_u = r_v
    s = np.zeros((1, 2, H, H))
    s[0, 0, 3, 2], s[0, 1, 6, 7] = 0.5, 0.5                                        # the cells one pixel right and below their joints
    z = ref_bone(s, s, np.array([[[4.0, 8.0], [24.0, 20.0]]]), stride, 0, [(0, 1)])
    assert not z["bone_resid"].any() and not z["loss3"].any() and not z["dp"].any() and z["resid"].all()


# ---- the setting, the skeleton and the metric --------------------------------------------------------------------------------------------
def _cfg(**training):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    for k, v in training.items():
        setattr(cfg.TRAINING, k, v)
    return cfg


def test_bone_loss_is_validated_where_the_config_is_read():
    from hupr_amd.misc.losses import LossComputer, bone_loss_setting, bone_weights
    cfg = _cfg()
    assert not hasattr(cfg.TRAINING, "boneLoss")                                    # the shipped YAML is the reference's
    assert bone_loss_setting(cfg) is None and bone_loss_setting(_cfg(boneLoss=-1)) is None
    assert bone_loss_setting(_cfg(boneLoss=-1.0)) is None
    for off in (cfg, _cfg(boneLoss=-1), _cfg(coordLoss=0.5)):
        lc = LossComputer(off, "cpu")
        assert lc.boneLoss is None and lc.bone_acc is None and lc.bone_residual is None
        assert ("computeLoss" in vars(lc)) == hasattr(off.TRAINING, "coordLoss")    # without either key: the class's own method
    for mu in (0.5, 1, 2, 1e-3, 100.0):
        got = bone_loss_setting(_cfg(boneLoss=mu))
        assert got == mu and isinstance(got, float)
        lc = LossComputer(_cfg(boneLoss=mu), "cpu")
        assert lc.boneLoss == mu and lc.bone_residual is None and not lc.mined and lc.coordLoss is None and lc._bone_w is None
        assert lc.bones == SKELETON0
        assert lc.bone_acc.dtype == torch.float64 and tuple(lc.bone_acc.shape) == (3,) and not lc.bone_acc.any()
    for bogus in (0, 0.0, -2, -0.5, NAN, INF, -INF, True, False, "0.5", "", None, [0.5], {"weight": 0.5}):
        with pytest.raises(ValueError) as e:
            bone_loss_setting(_cfg(boneLoss=bogus))
        assert "TRAINING.boneLoss" in str(e.value)
        with pytest.raises(ValueError):
            LossComputer(_cfg(boneLoss=bogus), "cpu")
    # both keys, and the bone weights from jointWeights: sqrt(w_u w_v) in fp64, stored as fp32; a zero joint silences its bones
    jw = [1.0, 1.0, 1.5, 1.0, 1.0, 1.5, 0.0, 0.5, 1.0, 2.0, 2.5, 1.0, 2.0, 2.5]
    lc = LossComputer(_cfg(boneLoss=0.5, coordLoss=0.25, jointWeights=jw), "cpu")
    assert lc.boneLoss == 0.5 and lc.coordLoss == 0.25
    want = np.array([np.sqrt(np.float64(jw[u]) * np.float64(jw[v])) for u, v in SKELETON0]).astype(np.float32)
    assert lc._bone_w.dtype == torch.float32 and np.array_equal(lc._bone_w.numpy(), want)
    assert bone_weights(jw, SKELETON0) == want.tolist()
    assert [w == 0 for w in want] == [6 in uv for uv in SKELETON0] and want[0] == np.float32(np.sqrt(5.0))


def test_skeleton_is_a_spanning_tree_of_the_joints():
    from hupr_amd import functional as F_
    from hupr_amd.datasets.base import JOINT_NAMES, SKELETON
    assert len(JOINT_NAMES) == 14 and len(SKELETON) == 13
    bones = F_.default_bones()
    assert bones == SKELETON0 == tuple((u - 1, v - 1) for u, v in SKELETON)
    assert all(0 <= u < 14 and 0 <= v < 14 and u != v for u, v in bones)
    reached, grew = {0}, True                                                       # 13 edges that connect 14 joints: a tree
    while grew:
        new = {b for a, b in bones if a in reached} | {a for a, b in bones if b in reached}
        grew = not new <= reached
        reached |= new
    assert reached == set(range(14))
    assert F_.bone_table(None, 14) == bones and F_.bone_table([[0, 1], (2, np.int64(1))], 3) == ((0, 1), (2, 1))
    for bad, K in ((None, 13), ([], 14), ([(0, 1)] * 33, 14), ([(0, 14)], 14), ([(-1, 0)], 14), ([(3, 3)], 14), ([(0.0, 1)], 14),
                   ([(True, 0)], 14), ([(0, 1, 2)], 14), (5, 14), ([3], 14)):
        with pytest.raises(ValueError):
            F_.bone_table(bad, K)


def test_mean_bone_error_on_hand_computed_numbers():
    from hupr_amd.misc.oks_eval import make_gt, mean_bone_error, mean_position_error
    g = np.zeros((14, 2))
    g[:, 0] = 10.0 * np.arange(14)                                                  # joint j at (10 j, 0)
    det = lambda iid, xy: {"image_id": iid, "keypoints": np.concatenate([xy, np.ones((14, 1))], axis=1).reshape(-1), "score": 1.0}
    gts = [make_gt(1, g, (0, 0, 130, 10)), make_gt(2, g, (0, 0, 130, 10)), make_gt(3, g, (0, 0, 130, 10))]
    shifted = g + np.array([7.0, -3.0])                                             # the whole pose displaced: no bone error
    mean, per_bone, n = mean_bone_error(gts, [det(1, shifted)])
    assert n == 1 and mean < 1e-12 and per_bone.shape == (13,) and mean_position_error(gts, [det(1, shifted)])[0] > 7.0
    stretched = g.copy()
    stretched[13] = (133.0, 4.0)                                                    # R_Wrist: bone (13, 12) is 13 x 4 -> sqrt(185), was 10
    mean, per_bone, n = mean_bone_error(gts, [det(1, shifted), det(2, stretched), det(2, g), det(9, g)])
    e = np.sqrt(13.0 ** 2 + 4.0 ** 2) - 10.0
    assert n == 2 and np.isclose(mean, e / 26, rtol=1e-14)                          # 2 images x 13 bones; the second record of image 2
    assert np.isclose(per_bone[0], e / 2, rtol=1e-14) and not per_bone[1:].any()    # and the unmatched image 9 do not count
    # a table of one's own, zero-based: |‖p_2 - p_0‖ - ‖g_2 - g_0‖| = |sqrt(20^2 + 15^2) - 20| = 5
    bent = g.copy()
    bent[2] = (20.0, 15.0)
    mean, per_bone, n = mean_bone_error(gts, [det(3, bent)], bones=[(0, 2), (0, 1)])
    assert n == 1 and per_bone.tolist() == [5.0, 0.0] and mean == 2.5
    mean, per_bone, n = mean_bone_error(gts, [det(9, g)])
    assert n == 0 and np.isnan(mean) and np.isnan(per_bone).all() and per_bone.shape == (13,)


# ---- the C ABI and the Function, short of a launch ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


P = 4096                                                   # any non-null address: every call below returns before it launches


def _table(pairs):
    flat = [i for uv in pairs for i in uv]
    return (ctypes.c_int * max(len(flat), 1))(*flat)


def _fwd(L, p1=P, p2=P, joints=P, B=3, K=14, H=64, stride=4.0, snap=0, bones=SKELETON0, E=None, w=None, eps=1.0, loss3=P, resid=P,
         inv_den=P, bone_resid=P, gcoef=P, acc=None):
    table = _table(bones) if bones is not None else None
    return L.hupr_bone_loss_fwd_f32(p1, p2, joints, B, K, H, stride, snap, table, len(bones) if E is None else E, w, eps, 1.0, 1.0,
                                    loss3, resid, inv_den, bone_resid, gcoef, acc, None)


def _bwd(L, resid=P, inv_den=P, gcoef=P, joints=P, g=P, B=3, K=14, E=13, H=64, stride=4.0, snap=0, dp1=P, dp2=P):
    return L.hupr_bone_loss_bwd_f32(resid, inv_den, gcoef, joints, g, B, K, E, H, stride, snap, 1.0, 1.0, dp1, dp2, None)


def test_entry_points_check_their_arguments_on_the_host(L):
    n0 = L.hupr_launch_count()
    shapes = [dict(B=0), dict(B=-3), dict(K=0), dict(K=65), dict(K=-14), dict(H=0), dict(H=-64), dict(H=4097), dict(B=1 << 60),
              dict(B=1 << 50, H=4096), dict(stride=0.0), dict(stride=-4.0), dict(stride=NAN), dict(stride=INF), dict(E=0), dict(E=33),
              dict(E=-1)]
    chain33 = tuple((j, j + 1) for j in range(33))
    fwd_refused = [dict(p1=None), dict(p2=None), dict(joints=None), dict(bones=None, E=13), dict(loss3=None), dict(resid=None),
                   dict(inv_den=None), dict(bone_resid=None), dict(gcoef=None), dict(eps=0.0), dict(eps=-1.0), dict(eps=NAN),
                   dict(eps=INF), dict(bones=chain33, K=64), dict(bones=((0, 14),)), dict(bones=((14, 0),)), dict(bones=((-1, 0),)),
                   dict(bones=SKELETON0[:5] + ((3, 3),)), dict(bones=SKELETON0, K=13), dict(bones=((0, 1), (1, 0), (0, 1 << 30)))] + shapes
    for kw in fwd_refused:
        assert _fwd(L, **kw) == -1, kw
        msg = L.hupr_last_error()
        assert msg.startswith(b"hupr_bone_loss_fwd_f32: ") and len(msg) > 35, (kw, msg)
    bwd_refused = [dict(resid=None), dict(inv_den=None), dict(gcoef=None), dict(joints=None), dict(g=None), dict(dp1=None),
                   dict(dp2=None)] + shapes
    for kw in bwd_refused:
        assert _bwd(L, **kw) == -1, kw
        msg = L.hupr_last_error()
        assert msg.startswith(b"hupr_bone_loss_bwd_f32: ") and len(msg) > 35, (kw, msg)
    assert _fwd(L, p1=None) == -1 and b"null" in L.hupr_last_error()
    assert _fwd(L, bones=None, E=13) == -1 and b"null" in L.hupr_last_error()
    assert _fwd(L, E=0) == -1 and b"E 0" in L.hupr_last_error()
    assert _fwd(L, E=33) == -1 and b"E 33" in L.hupr_last_error()
    assert _fwd(L, bones=((0, 14),)) == -1 and b"bone 0 = (0, 14)" in L.hupr_last_error()
    assert _fwd(L, bones=SKELETON0[:5] + ((3, 3),)) == -1 and b"bone 5 = (3, 3)" in L.hupr_last_error()
    assert _fwd(L, K=65) == -1 and b"K 65" in L.hupr_last_error()
    assert _fwd(L, eps=0.0) == -1 and b"eps" in L.hupr_last_error()
    assert _bwd(L, stride=0.0) == -1 and b"stride" in L.hupr_last_error()
    assert _bwd(L, E=33) == -1 and b"E 33" in L.hupr_last_error()
    assert _bwd(L, inv_den=None) == -1 and b"null" in L.hupr_last_error()
    assert L.hupr_launch_count() == n0                        # refused before any launch


def test_function_refuses_what_it_cannot_run():
    from hupr_amd import functional as F_
    import __graft_entry__ as g
    g.build()
    x, j = torch.full((2, 14, 8, 8), 0.5), torch.zeros((2, 14, 2))
    for args in ((x, x, j, 4.0, False, None, None, 1.0, 1.0, None),                    # CPU tensors: no fallback
                 (x.double(), x.double(), j, 4.0, False, None, None, 1.0, 1.0, None),
                 (x.numpy(), x, j, 4.0, False, None, None, 1.0, 1.0, None)):
        with pytest.raises(ValueError):
            F_.BoneLossFn.apply(*args)


def test_bone_loss_kernels_use_no_scratch():
    """The listing the build keeps for csrc/bone_loss.hip: the plane and backward kernels in their 16-byte and 4-byte forms and the
    one-workgroup kernel, nothing else; 0 spilled registers, 0 bytes of scratch (the bone table is read from the kernel's arguments,
    not copied to private memory), 256 threads, at most 64 VGPRs (eight waves per SIMD fit)."""
    meta = kernel_metadata("bone_loss")
    kinds = sorted(re.search(r"hupr_k_bone_loss_[a-z]+(ILb[01]E)?", name).group(0) for name in meta)
    assert kinds == ["hupr_k_bone_loss_bwdILb0E", "hupr_k_bone_loss_bwdILb1E", "hupr_k_bone_loss_planeILb0E",
                     "hupr_k_bone_loss_planeILb1E", "hupr_k_bone_loss_sum"], sorted(meta)
    for name, m in meta.items():
        assert m["spill"] == 0 and m["sspill"] == 0 and m["scratch"] == 0, (name, m)
        assert m["threads"] == 256 and m["vgpr"] <= 64 and m["lds"] <= 1024, (name, m)
