"""GPU (-m gpu): hupr_bce_mined_fwd_f32 / hupr_bce_mined_bwd_f32 (csrc/bce_mined.hip) against the fp64 statement of the rule in
include/hupr.h (``ref_mined`` in tests/test_ohkm_cpu.py, which checks the reference itself), and every layer built on them:
``functional.MinedBCEFn``, ``LossComputer`` with ``TRAINING.ohkm`` / ``TRAINING.jointWeights``, ``TrainEngine`` eager and captured,
and the Runner with its per-epoch line.

Inputs (``make_case``): every plane has its own difficulty, and before any comparison each test asserts in fp64 that the k-th and
(k + 1)-th largest weighted plane losses of every (head, sample) differ by at least 1e-3 relative, so the selection is never decided
by rounding and no plane is left out of a comparison.

Bounds.  plane_loss against fp64: |err| <= 2.5e-7 + 2.5e-6 l.  Each term carries about 1.2e-7 of absolute error (logf within a few
ulp of a value of order 1; 1 - p is exact for p >= 0.5 and rounds once below), and the plane sum is a sum of non-negative terms
through at most 16 (a thread's cells at HW = 4096) + 6 (the wave butterfly) fp32 additions, the four waves and the division by HW in
fp64 and one rounding of the mean: 23 roundings of 6e-8 = 1.4e-6 relative.  The 1e-3 selection margin is 400 times that bound.
loss3, and the gradients: 1e-6 of the reference's largest magnitude, the figure of
tests/test_ops_gpu.py::test_both_losses_and_their_weighted_sum_as_one_node.  coef: the zero pattern exactly, values 1e-6 relative.
counts: exactly."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from test_ohkm_cpu import CASES, MARGIN, ks, make_case, make_weights, ref_mined, ref_select, selection_margin

pytestmark = pytest.mark.gpu
NAN = float("nan")


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def launch_fwd(p1, p2, t, k, w=None, alpha=1.0, beta=1.0, counts=None):
    """The C ABI on outputs pre-filled with NaN, so a value the kernels do not write shows.  p1, p2, t: (B, K, HW) device tensors."""
    from hupr_amd import runtime as rt
    B, K, HW = p1.shape
    loss3 = torch.full((3,), NAN, dtype=torch.float32, device="cuda")
    plane_loss = torch.full((2, B, K), NAN, dtype=torch.float32, device="cuda")
    coef = torch.full((2, B, K), NAN, dtype=torch.float32, device="cuda")
    rt.check(rt.lib().hupr_bce_mined_fwd_f32(rt.ptr(p1), rt.ptr(p2), rt.ptr(t), B, K, HW, k, rt.ptr(w), alpha, beta, rt.ptr(loss3),
                                             rt.ptr(plane_loss), rt.ptr(coef), rt.ptr(counts), rt.stream()))
    return loss3, plane_loss, coef


def launch_bwd(p1, p2, t, coef, g, g2=None, alpha=1.0, beta=1.0):
    from hupr_amd import runtime as rt
    B, K, HW = p1.shape
    dp1, dp2 = torch.full_like(p1, NAN), torch.full_like(p2, NAN)
    gd = torch.tensor([g], dtype=torch.float32, device="cuda")
    g2d = torch.tensor([g2], dtype=torch.float32, device="cuda") if g2 is not None else None
    rt.check(rt.lib().hupr_bce_mined_bwd_f32(rt.ptr(p1), rt.ptr(p2), rt.ptr(t), rt.ptr(coef), rt.ptr(gd), rt.ptr(g2d), alpha, beta,
                                             rt.ptr(dp1), rt.ptr(dp2), B, K, HW, rt.stream()))
    return dp1, dp2


def check_plane_loss(got, ref, what):
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    worst = float((err / (2.5e-7 + 2.5e-6 * ref)).max())
    print("%s: plane_loss max |err| %.3e, worst err / bound %.3f" % (what, err.max(), worst))
    assert worst <= 1.0, what


def check_scaled(got, ref, what, tol=1e-6):
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), what
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print("%s: max err %.3e vs scale %.3e (rel %.3e)" % (what, err, scale, err / max(scale, 1e-300)))
    assert err <= tol * scale, what


@functools.lru_cache(maxsize=None)
def case(shape):
    return make_case(*shape, CASES[shape])


# ---- 1: the kernels against the rule in fp64 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("shape", list(CASES), ids=lambda s: "B%d-K%d-H%d" % s)
def test_kernels_against_fp64(shape, weighted):
    """Every k in {1, K // 2, K - 1, K}; alpha, beta not 1; the gradient of the second loss present and absent; the counters
    accumulated over two calls.  (3, 14, 64) is the model's plane, H = 5 the 4-byte path at K = 17 and at the K limit, (33, 14, 8)
    more samples than one pass of the selection kernel's four waves, (1, 1, 5) the smallest problem."""
    B, K, H = shape
    p1, p2, t = case(shape)
    w = make_weights(K) if weighted else None
    d1, d2, dt, dw = dev(p1), dev(p2), dev(t), (dev(w) if weighted else None)
    alpha, beta, g, g2 = 0.3, 0.7, 1.7, 0.5
    for k in ks(K):
        what = "B%d K%d H%d k%d%s" % (B, K, H, k, " weighted" if weighted else "")
        for with_g2 in (True, False):
            ref = ref_mined(p1, p2, t, k, w, alpha, beta, g, g2 if with_g2 else None)
            if with_g2:
                margin = selection_margin(ref["v"], k)
                assert margin >= MARGIN, (what, margin)
                counts = torch.zeros((2, K), dtype=torch.int64, device="cuda")
                loss3, plane_loss, coef = launch_fwd(d1, d2, dt, k, dw, alpha, beta, counts)
                check_plane_loss(plane_loss, ref["plane_loss"], what)
                check_scaled(loss3, ref["loss3"], what + " loss3")
                c = coef.cpu().numpy().astype(np.float64)
                assert np.array_equal(c != 0, ref["coef"] != 0), what                      # the selection (and the zero weight) exactly
                assert (np.abs(c - ref["coef"]) <= 1e-6 * ref["coef"]).all(), what
                assert np.array_equal(counts.cpu().numpy(), ref["counts"]), what
                launch_fwd(d1, d2, dt, k, dw, alpha, beta, counts)
                assert np.array_equal(counts.cpu().numpy(), 2 * ref["counts"]), what
                assert ref["counts"].sum() == 2 * B * k
            dp1, dp2 = launch_bwd(d1, d2, dt, coef, g, g2 if with_g2 else None, alpha, beta)
            assert np.allclose(ref["dp_autograd"], ref["dp_rule"], rtol=1e-10, atol=0)      # no clamp acts on these inputs
            for h, dp in enumerate((dp1, dp2)):
                check_scaled(dp, ref["dp_autograd"][h], "%s dp%d%s" % (what, h + 1, " +g2" if with_g2 else ""))
                off = ref["coef"][h] == 0
                assert not dp.cpu().numpy()[off].any(), what                                # exactly zero outside the selection


def test_clamps_and_floor():
    """One plane holds p exactly 0 and exactly 1 against t in {0, 1}: the -100 clamp of both logs and the 1e-12 floor of the
    backward, against the same rule in fp64, on the 16-byte (HW = 8) and the 4-byte (HW = 5) path."""
    for HW in (8, 5):
        p = np.full((1, 2, HW), 0.25, dtype=np.float32)
        t = np.full((1, 2, HW), 0.5, dtype=np.float32)
        p[0, 0, :5] = [0.0, 0.0, 1.0, 1.0, 0.5]
        t[0, 0, :5] = [0.0, 1.0, 0.0, 1.0, 1.0]
        q = p.copy()
        q[0, 0] = p[0, 0, ::-1]                                                             # head 1: the same cells against other targets
        ref = ref_mined(p, q, t, 2, None, 0.3, 0.7, 1.7, 0.5)
        assert ref["plane_loss"][0, 0, 0] > 200.0 / HW - 1e-9                               # both clamps acted
        d1, d2, dt = dev(p), dev(q), dev(t)
        loss3, plane_loss, coef = launch_fwd(d1, d2, dt, 2, None, 0.3, 0.7)
        check_plane_loss(plane_loss, ref["plane_loss"], "clamps HW %d" % HW)
        check_scaled(loss3, ref["loss3"], "clamps loss3")
        dp1, dp2 = launch_bwd(d1, d2, dt, coef, 1.7, 0.5, 0.3, 0.7)
        assert np.abs(ref["dp_rule"]).max() > 1e9                                           # the floor acted
        for h, dp in enumerate((dp1, dp2)):
            check_scaled(dp, ref["dp_rule"][h], "clamps dp%d" % (h + 1))
        assert dp1[0, 0, 0].item() == 0.0 and dp1[0, 0, 3].item() == 0.0                   # p == t at the clamp: no gradient


@pytest.mark.parametrize("H", [64, 5])
def test_ties_go_to_the_lower_joint(H):
    """Two joints of one sample with identical p and t planes: equal plane_loss bits, and with k cutting between them the lower
    index is kept."""
    B, K = 2, 14
    p1, p2, t = (x.copy() for x in make_case(B, K, H, 11))
    lo, hi = 4, 9
    for x in (p1, p2, t):
        x[1, hi] = x[1, lo]
    l64 = ref_mined(p1, p2, t, 1)["plane_loss"]
    d1, d2, dt = dev(p1), dev(p2), dev(t)
    for h in range(2):
        k = int((l64[h, 1] > l64[h, 1, lo]).sum()) + 1                                      # the planes ahead of the pair, and one more
        ref = ref_mined(p1, p2, t, k)
        assert ref["sel"][h, 1, lo] and not ref["sel"][h, 1, hi]
        others = np.delete(l64[h, 1], [lo, hi])
        assert (np.abs(others - l64[h, 1, lo]) >= MARGIN * l64[h, 1, lo]).all()             # only the tie is close to the cut
        _, plane_loss, coef = launch_fwd(d1, d2, dt, k)
        bits = plane_loss.view(torch.int32)
        assert bits[h, 1, lo].item() == bits[h, 1, hi].item()
        got = coef[h, 1].cpu().numpy() != 0
        assert got[lo] and not got[hi] and got.sum() == k
        assert np.array_equal(got, ref["sel"][h, 1])


def test_nan_plane_is_always_kept():
    """One NaN cell in one plane of head 0: that plane is kept for every k, the loss is NaN (it reaches the gradient guard, it is
    not mined away), the gradient of its cell is NaN, and every other plane's loss keeps its bits."""
    B, K, H = 2, 6, 8
    p1, p2, t = (x.copy() for x in make_case(B, K, H, 4))
    d1, d2, dt = dev(p1), dev(p2), dev(t)
    _, clean, _ = launch_fwd(d1, d2, dt, K)
    b, j = 1, int(np.argmin(ref_mined(p1, p2, t, K)["plane_loss"][0, 1]))                   # the easiest plane of the sample
    p1[b, j, 13] = NAN
    d1 = dev(p1)
    for k in range(1, K + 1):
        counts = torch.zeros((2, K), dtype=torch.int64, device="cuda")
        loss3, plane_loss, coef = launch_fwd(d1, d2, dt, k, None, 0.3, 0.7, counts)
        assert coef[0, b, j].item() != 0 and int((coef[0, b] != 0).sum()) == k
        assert torch.isnan(loss3[0]) and torch.isnan(loss3[1]) and torch.isfinite(loss3[2])
        assert torch.isnan(plane_loss[0, b, j])
        keep = torch.ones((2, B, K), dtype=torch.bool, device="cuda")
        keep[0, b, j] = False
        assert torch.equal(plane_loss[keep], clean[keep])
        assert counts.cpu().numpy().sum() == 2 * B * k and counts[0, j].item() >= 1
        dp1, dp2 = launch_bwd(d1, d2, dt, coef, 1.0, None, 0.3, 0.7)
        assert torch.isnan(dp1[b, j, 13]) and int(torch.isnan(dp1).sum()) == 1 and torch.isfinite(dp2).all()


def test_two_runs_give_equal_bits():
    shape = (3, 14, 64)
    p1, p2, t = case(shape)
    d1, d2, dt, dw = dev(p1), dev(p2), dev(t), dev(make_weights(14))
    outs = []
    for _ in range(2):
        counts = torch.zeros((2, 14), dtype=torch.int64, device="cuda")
        loss3, plane_loss, coef = launch_fwd(d1, d2, dt, 7, dw, 0.3, 0.7, counts)
        dp1, dp2 = launch_bwd(d1, d2, dt, coef, 1.7, 0.5, 0.3, 0.7)
        outs.append((loss3, plane_loss, coef, counts, dp1, dp2))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- 2: the Function, beside PairBCEFn --------------------------------------------------------------------------------------------------
def test_every_joint_kept_agrees_with_the_pair_loss_and_launches_as_often():
    """k = K and no weights: the losses and both gradients of PairBCEFn to 1e-6 of their magnitude (not bit for bit: the order of
    summation differs), and hupr_launch_count() moves by the same amount for one forward + backward of either Function."""
    from hupr_amd import functional as F_
    B, K, H = 3, 14, 64
    p1, p2, t = (dev(x).reshape(B, K, H, H) for x in case((B, K, H)))
    alpha, beta = 0.3, 0.7
    moved, res = [], []
    for fn in ("pair", "mined"):
        a1, a2 = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
        n0 = F_.rt.lib().hupr_launch_count()
        if fn == "pair":
            loss, loss2 = F_.PairBCEFn.apply(a1, a2, t, alpha, beta)
        else:
            loss, loss2 = F_.MinedBCEFn.apply(a1, a2, t, K, None, alpha, beta, None)
        (1.7 * loss + 0.5 * loss2).backward()
        moved.append(F_.rt.lib().hupr_launch_count() - n0)
        res.append((loss.detach(), loss2.detach(), a1.grad, a2.grad))
    assert moved == [3, 3], moved
    for name, ref, got in zip(("loss", "loss2", "dp1", "dp2"), *res):
        check_scaled(got, ref.cpu().numpy().astype(np.float64), "pair vs mined " + name)
    pl = F_.MinedBCEFn.last_plane_loss
    assert tuple(pl.shape) == (2, B, K) and not pl.requires_grad and pl.dtype == torch.float32
    # what it cannot run raises; nothing falls back to the plain loss
    a1 = p1.clone().requires_grad_(True)
    for args in ((a1, p2, t, 0, None, 1.0, 1.0, None), (a1, p2, t, K + 1, None, 1.0, 1.0, None), (a1, p2, t, True, None, 1.0, 1.0, None),
                 (a1, p2, t, 8.0, None, 1.0, 1.0, None), (a1, p2[:, :7], t, 4, None, 1.0, 1.0, None),
                 (a1, p2.double(), t, 8, None, 1.0, 1.0, None), (a1, p2.cpu(), t, 8, None, 1.0, 1.0, None),
                 (a1, p2, t, 8, torch.ones(K), 1.0, 1.0, None), (a1, p2, t, 8, torch.ones(K + 1, device="cuda"), 1.0, 1.0, None),
                 (a1, p2, t, 8, torch.ones(K, device="cuda", dtype=torch.float64), 1.0, 1.0, None),
                 (a1, p2, t, 8, None, 1.0, 1.0, torch.zeros((2, K), dtype=torch.int32, device="cuda")),
                 (a1, p2, t, 8, None, 1.0, 1.0, torch.zeros((K, 2), dtype=torch.int64, device="cuda")),
                 (a1, p2, t, 8, None, 1.0, 1.0, torch.zeros((2, K), dtype=torch.int64))):
        with pytest.raises(ValueError):
            F_.MinedBCEFn.apply(*args)


# ---- 3: LossComputer ---------------------------------------------------------------------------------------------------------------------
def _cfg(**training):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    for k, v in training.items():
        setattr(cfg.TRAINING, k, v)
    return cfg


JOINT_W = [1.0, 1.0, 1.5, 1.0, 1.0, 1.5, 0.0, 0.5, 1.0, 2.0, 2.5, 1.0, 2.0, 2.5]


def _loss_inputs(lc, k, w, B=2):
    """Integer joints, the targets LossComputer forms from them (the reference's, not under test here) and predictions around them
    with make_case's per-plane difficulties; the first seed whose fp64 selection margin holds for (k, w)."""
    from hupr_amd import synth
    K, H = 14, 64
    for seed in range(10):
        joints = torch.from_numpy(synth.keypoints(B, 40 + seed))
        T = lc.targets(joints.cuda()).cpu().numpy().reshape(B, K, H * H)
        rng = np.random.RandomState(50 + seed)
        a = np.stack([rng.permutation(np.linspace(0.05, 0.6, K)) for _ in range(B)])
        p = [np.clip(T + s * a[..., None] * rng.uniform(-1.0, 1.0, T.shape), 1e-4, 1.0 - 1e-4).astype(np.float32) for s in (1.0, 0.8)]
        if selection_margin(ref_mined(p[0], p[1], T, k, w)["v"], k) >= MARGIN:
            return joints, T, p[0], p[1]
    raise AssertionError("no seed in 0..9 leaves a 1e-3 selection margin")


@pytest.mark.parametrize("setting", ["ohkm", "weights", "both"])
def test_loss_computer_with_mining_and_weights(setting):
    from hupr_amd.misc.losses import LossComputer
    B, K, H = 2, 14, 64
    training = dict(ohkm=dict(ohkm=8), weights=dict(jointWeights=JOINT_W), both=dict(ohkm=8, jointWeights=JOINT_W))[setting]
    cfg = _cfg(**training)
    assert cfg.TRAINING.lossDecay == -1                                                     # the plain sum of both losses
    lc = LossComputer(cfg, "cuda")
    k = 8 if "ohkm" in training else K
    w = np.array(JOINT_W) if "jointWeights" in training else None
    assert lc.mined and lc.mined_k == k
    joints, T, p1, p2 = _loss_inputs(lc, k, w)
    ref = ref_mined(p1, p2, T, k, w, 1.0, 1.0, 1.0, None)
    assert selection_margin(ref["v"], k) >= MARGIN
    a1 = dev(p1).reshape(B, K, 1, H, H).requires_grad_(True)
    a2 = dev(p2).reshape(B, 1, K, H, H).requires_grad_(True)
    loss, loss2, _, _ = lc.computeLoss((a1, a2), joints.cuda(), decode="device")
    loss.backward()
    check_scaled(loss, ref["loss3"][:1], setting + " loss")
    check_scaled(loss2, ref["loss3"][2:], setting + " loss2")
    check_scaled(a1.grad.reshape(B, K, -1), ref["dp_autograd"][0], setting + " dpreds1")
    check_scaled(a2.grad.reshape(B, K, -1), ref["dp_autograd"][1], setting + " dpreds2")
    check_plane_loss(lc.plane_loss, ref["plane_loss"], setting)
    assert not lc.plane_loss.requires_grad and tuple(lc.plane_loss.shape) == (2, B, K)
    assert np.array_equal(lc.mining_counts.cpu().numpy(), ref["counts"])
    # evaluation shows the trained loss and does not count
    with torch.no_grad():
        le, le2, _, _ = lc.computeLoss((a1.detach(), a2.detach()), joints.cuda(), decode=False)
    assert torch.equal(le, loss.detach()) and torch.equal(le2, loss2.detach())
    assert np.array_equal(lc.mining_counts.cpu().numpy(), ref["counts"])
    lc.computeLoss((a1.detach(), a2.detach()), joints.cuda(), decode=False)                 # gradients enabled: it counts
    assert np.array_equal(lc.mining_counts.cpu().numpy(), 2 * ref["counts"])


def test_loss_computer_without_the_keys_is_the_pair_loss():
    from hupr_amd import functional as F_
    from hupr_amd.misc.losses import LossComputer
    B, K, H = 2, 14, 64
    for training in ({}, dict(ohkm=-1, jointWeights=-1)):
        lc = LossComputer(_cfg(**training), "cuda")
        assert not lc.mined and lc.mining_counts is None
        joints, T, p1, p2 = _loss_inputs(lc, K, None)
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
        assert lc.plane_loss is None


# ---- 4: the engine, eager and captured ---------------------------------------------------------------------------------------------------
def test_graph_replay_matches_eager_steps_with_mining():
    """tests/test_targets_subpixel_gpu.py::test_graph_replay_matches_eager_steps_with_subpixel_targets at its size (B = 4, bf16) and
    with its bounds, with ``TRAINING.ohkm: 8``: five eager steps against 2 eager + capture (1 warm-up step) + 2 replays.  The
    counters replay with the step: after every step of either engine they have moved by exactly the selection that the step's own
    plane_loss implies, 5 B k per head in all.  The two engines may keep different joints only in a (step, head, sample) whose k-th and
    (k + 1)-th plane losses are within 1e-3 relative; the number of such samples is printed (measured: 7 of the 40 (step, head,
    sample) triples are that close — an untrained network gives every joint nearly the same loss — and the two engines kept the
    same joints in all 40; parameters rel 0, losses equal)."""
    from hupr_amd import functional as F_, synth
    from hupr_amd.tools.engine import TrainEngine
    try:
        F_.set_math("bf16")
        k = 8
        cfg = _cfg(ohkm=k)
        dev0 = torch.device("cuda", 0)
        B, G, K = 4, cfg.DATASET.numGroupFrames, 14
        adc_h = torch.from_numpy(synth.adc_cube_int16(31, sensor=0, nframes=B * G)).to(dev0)
        adc_v = torch.from_numpy(synth.adc_cube_int16(31, sensor=1, nframes=B * G)).to(dev0)
        joints = torch.from_numpy(synth.keypoints(B, 32)).to(dev0)

        def record(e, log):
            st = e.mining_stats()
            assert st["k"] == k and st["counts"].dtype == np.int64 and st["counts"].shape == (2, K)
            assert st["plane_loss"].shape == (2, B, K) and st["samples"] == B * (len(log) + 1)
            log.append((st["counts"].copy(), st["plane_loss"].copy()))

        e1, log1 = TrainEngine(cfg, device=dev0, seed=0), []
        assert e1.mining_stats()["samples"] == 0 and not e1.mining_stats()["counts"].any()
        for _ in range(5):
            l1, _ = e1.train_step_from_adc(adc_h, adc_v, joints)
            record(e1, log1)
        e2, log2 = TrainEngine(cfg, device=dev0, seed=0), []
        for _ in range(2):
            e2.train_step_from_adc(adc_h, adc_v, joints)
            record(e2, log2)
        e2.capture(adc_h, adc_v, joints, warmup=1)                                          # the warm-up step is the third step
        torch.cuda.synchronize()
        record(e2, log2)
        log2[-1] = (log2[-1][0], None)                      # its plane_loss is the captured buffer, which no step has filled yet
        for _ in range(2):
            l2, _ = e2.train_step_from_adc(adc_h, adc_v, joints)
            record(e2, log2)

        rel = ((torch.cat([p.detach().flatten() for p in e1.model.parameters()]) -
                torch.cat([p.detach().flatten() for p in e2.model.parameters()])).norm() /
               torch.cat([p.detach().flatten() for p in e1.model.parameters()]).norm()).item()
        print("after 5 steps: parameters rel %.3e, loss %.6f vs %.6f" % (rel, float(l1.detach()), float(l2.detach())))

        kept = []                                           # per engine and step: (the step's move of the counters, its selection)
        for name, log in (("eager", log1), ("captured", log2)):
            prev, mine = np.zeros((2, K), dtype=np.int64), []
            for step, (counts, plane_loss) in enumerate(log):
                moved = counts - prev
                assert (moved >= 0).all() and np.array_equal(moved.sum(axis=1), [B * k, B * k]), (name, step)
                sel = None
                if plane_loss is not None:
                    sel = ref_select(plane_loss.astype(np.float64), k)                     # fp32 -> fp64 is exact: the kernel's own order
                    assert np.array_equal(moved, sel.sum(axis=1)), (name, step)
                prev = counts
                mine.append((moved, sel))
            assert np.array_equal(log[-1][0].sum(axis=1), [5 * B * k, 5 * B * k]), name
            kept.append(mine)
        close, differ, differ_far = 0, 0, 0
        for step in range(5):
            s = -np.sort(-log1[step][1].astype(np.float64), axis=-1)
            near = (s[..., k - 1] - s[..., k]) <= 1e-3 * s[..., k - 1]                      # (2, B)
            close += int(near.sum())
            if kept[1][step][1] is None:                    # the warm-up step: only its counters are known
                if not near.any():
                    assert np.array_equal(kept[0][step][0], kept[1][step][0]), step
                continue
            diff = (kept[0][step][1] != kept[1][step][1]).any(axis=-1)
            differ += int(diff.sum())
            differ_far += int((diff & ~near).sum())
        print("samples (of %d) whose k-th and (k+1)-th plane losses are within 1e-3: %d; kept differently by the two engines: %d, "
              "of which outside those: %d" % (5 * 2 * B, close, differ, differ_far))
        assert differ_far == 0
        if close == 0:
            assert np.array_equal(log1[-1][0], log2[-1][0])
        assert torch.isfinite(torch.cat([p.detach().flatten() for p in e2.model.parameters()])).all()
        assert rel <= 1e-5, rel
        assert abs(float(l1.detach()) - float(l2.detach())) <= 1e-4 * abs(float(l1.detach()))
    finally:
        F_.set_math("f32")


def test_engine_without_the_keys_has_no_mining_stats():
    from hupr_amd.tools.engine import TrainEngine
    e = TrainEngine(_cfg(), device=torch.device("cuda", 0), seed=0)
    assert e.mining_stats() is None
    e.close()


# ---- 5: the Runner -----------------------------------------------------------------------------------------------------------------------
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


def test_runner_prints_the_mined_share_of_every_joint(tmp_path, monkeypatch, capsys):
    from hupr_amd.config_tree import load_config
    names = load_config().DATASET.idxToJoints
    run = _run_main(tmp_path, monkeypatch, "mined", ohkm=8)
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if "Mined joints" in l]
    assert len(lines) == 1, out                                                             # one epoch, one line
    head, _, body = lines[0].partition("): ")
    assert head == "==========>Mined joints in epoch 0 (PRGCN head, 8 of 14 kept, 4 samples", lines[0]
    pairs = re.findall(r"(\S+): (\d\.\d{3})", body)
    assert [n for n, _ in pairs] == list(names) and len(names) == 14, lines[0]
    shares = np.array([float(s) for _, s in pairs])
    assert ((shares >= 0) & (shares <= 1)).all() and abs(shares.sum() - 8.0) <= 14 * 5e-4, lines[0]
    assert np.allclose(shares * 4, np.round(shares * 4), atol=2e-3)                         # counts over four samples
    assert "AP: " in out and os.path.exists(run / "checkpoint.pth")
    mined_keys = list(torch.load(run / "checkpoint.pth"))
    plain = _run_main(tmp_path, monkeypatch, "plain")
    out = capsys.readouterr().out
    assert "AP: " in out and "Mined" not in out
    assert list(torch.load(plain / "checkpoint.pth")) == mined_keys                         # the counters are not checkpointed
    with pytest.raises(ValueError) as e:
        _run_main(tmp_path, monkeypatch, "zero", ohkm=0)
    assert "TRAINING.ohkm" in str(e.value)
    assert not os.path.exists(tmp_path / "logs" / "zero" / "checkpoint.pth")               # before any step
