"""GPU (-m gpu): hupr_gaussian_targets_subpixel_f32 (csrc/targets.hip) against an fp64 NumPy statement of the rule in include/hupr.h,
written here, and every layer built on it: ``functional.gaussian_targets_subpixel``, ``LossComputer`` with ``TRAINING.targets:
subpixel``, ``TrainEngine`` eager and captured, and the Runner with its ``MPJPE:`` line.

The reference forms ``ac = joint / stride``, ``mu = (int)(ac + 0.5f)`` and ``f = ac - (float)mu`` in fp32 with the kernel's own
operations (IEEE division, addition, subtraction; a truncating cast), so window membership has no borderline case and no cell is
excluded.  Everything after that is fp64.

Bounds.  Values: 1e-6 absolute.  A value is at most 1; expf is within 2 ulp (<= 2.4e-7 at 1); the fp32 argument
((dx - f)^2 + (dy - f)^2) / (2 sigma^2) carries a relative error of a few 6e-8, which expf turns into that much times a * exp(-a)
<= 0.37 of absolute error: about 3e-7 in all.  An indexing, sign or window error costs at least exp(-(rad + 1)^2 / (2 sigma^2)), about
2e-3.  Cells outside the window are +0.0 bit for bit.  Encode -> decode: 4e-3 image pixel = 1e-3 heat-map pixel, the bound
tests/test_pose_decode_gpu.py derives for inputs >= 1e-3 whose log has a smallest Hessian eigenvalue >= 0.02: here the 3 x 3
neighbourhood of the peak is >= exp(-2 * 1.5^2 / 8) = 0.57 and the Hessian of the log is -I / sigma^2 = -0.25 I."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-6
TOL_DECODE_PX = 4e-3


# ---- the rule in fp64 ----------------------------------------------------------------------------------------------------------------
def ref_targets(joints, H, sigma, rad, stride):
    """joints (BK, 2) float32 image pixels -> (targets (BK, H, H) float64, window (BK, H, H) bool: the cells the rule gives a value)."""
    joints = np.asarray(joints, dtype=np.float32)
    BK = joints.shape[0]
    out, win = np.zeros((BK, H, H)), np.zeros((BK, H, H), bool)
    for r in range(BK):
        mu, f = [], []
        for axis in range(2):
            with np.errstate(all="ignore"):
                ac = joints[r, axis] / np.float32(stride)                # fp32 division
                t = ac + np.float32(0.5)                                 # fp32 addition
            if not np.isfinite(joints[r, axis]) or not (-2.0 ** 31 <= float(t) < 2.0 ** 31):
                break                                                    # not finite, or the cast would overflow: zeros
            m = int(t)                                                   # truncates towards zero, as the cast does
            mu.append(m)
            f.append(float(ac - np.float32(m)))                          # fp32 subtraction
        if len(mu) < 2:
            continue
        if mu[0] - rad >= H or mu[1] - rad >= H or mu[0] + rad + 1 < 0 or mu[1] + rad + 1 < 0:
            continue
        d = np.arange(-rad, rad + 1)
        xs, ys = mu[0] + d, mu[1] + d
        kx, ky = (xs >= 0) & (xs < H), (ys >= 0) & (ys < H)
        gx, gy = (d[kx] - f[0]) ** 2, (d[ky] - f[1]) ** 2
        out[r][np.ix_(ys[ky], xs[kx])] = np.exp(-(gx[None, :] + gy[:, None]) / (2.0 * float(sigma) ** 2))
        win[r][np.ix_(ys[ky], xs[kx])] = True
    return out, win


def launch(joints, H, sigma, rad, stride):
    """The C ABI on an output pre-filled with NaN, so a cell the kernel does not write shows.  -> (BK, H, H) float32 ndarray."""
    from hupr_amd import runtime as rt
    j = torch.from_numpy(np.ascontiguousarray(joints, dtype=np.float32)).cuda()
    t = torch.full((j.shape[0], H, H), float("nan"), dtype=torch.float32, device="cuda")
    rt.check(rt.lib().hupr_gaussian_targets_subpixel_f32(rt.ptr(j), rt.ptr(t), j.shape[0], H, float(sigma), rad, float(stride), rt.stream()))
    return t.cpu().numpy()


def check(joints, H, sigma, rad, stride):
    joints = np.asarray(joints, dtype=np.float32)
    got = launch(joints, H, sigma, rad, stride)
    ref, win = ref_targets(joints, H, sigma, rad, stride)
    assert not np.isnan(got).any(), "unwritten cells or a NaN in rows %s" % sorted(set(np.argwhere(np.isnan(got))[:, 0]))
    err = np.abs(got.astype(np.float64) - ref)
    worst = np.unravel_index(err.argmax(), err.shape)
    print("H %d sigma %g rad %d stride %g: max |err| %.3e at row %d (joint %s), %d cells in windows" %
          (H, sigma, rad, stride, err.max(), worst[0], joints[worst[0]], win.sum()))
    assert err.max() <= TOL, (err.max(), worst, joints[worst[0]])
    assert (got.view(np.int32)[~win] == 0).all(), "a cell outside the window is not +0.0"
    assert (got[win] > 0).all()
    return got, ref, win


# ---- 1: the rule at the model's shape ------------------------------------------------------------------------------------------------
def model_shape_joints():
    rng = np.random.RandomState(11)
    nan, inf = float("nan"), float("inf")
    rows = [rng.uniform(0, 256, 2) for _ in range(6)]                                   # random
    rows += [4.0 * rng.randint(0, 64, 2) for _ in range(3)]                             # whole heat-map pixels
    rows += [4.0 * rng.randint(0, 64, 2) + 2.0 for _ in range(3)]                       # fraction exactly one half: the cast decides
    rows += [(0.0, 1.3), (255.99, 0.0), (1.3, 255.99)]
    rows += [(-10.0, 270.0), (270.0, -10.0), (-10.0, 100.3)]                            # the window is partly inside
    rows += [(-40.0, 300.0), (300.0, -40.0)]                                            # the window is outside: zeros
    rows += [(100.5, -40.0), (300.0, 77.25)]                                            # one coordinate fine, the other outside
    rows += [(nan, 100.0), (100.0, nan), (inf, -inf), (-inf, 50.0), (1e30, 100.0), (100.0, -1e30)]
    return np.array(rows, dtype=np.float32)


def test_rule_at_the_model_shape():
    joints = model_shape_joints()
    assert joints.shape == (28, 2)
    got, ref, win = check(joints, 64, 2.0, 6, 4.0)
    assert not got[18:].any() and not win[18:].any()                                    # outside, not finite, too large: zero planes
    assert win[:18].reshape(18, -1).any(axis=1).all()
    assert win[6:9].reshape(3, -1).sum(axis=1).max() <= 169 and win[0].sum() > 0
    assert (ref[6:9].reshape(3, -1).max(axis=1) == 1.0).all() and (got[6:9].reshape(3, -1).max(axis=1) == 1.0).all()


# ---- 2: other shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,sigma,rad,stride,BK", [(128, 3.0, 9, 2.0, 3), (6, 2.0, 6, 4.0, 5), (1, 2.0, 6, 4.0, 1)])
def test_other_shapes(H, sigma, rad, stride, BK):
    rng = np.random.RandomState(H)
    joints = rng.uniform(0, H * stride, (BK, 2)).astype(np.float32)
    if BK >= 3:
        joints[1] = (-3.0 * stride + 0.7, H * stride + 1.1)                              # windows that hang over two corners
        joints[2] = (H * stride - 0.01, 0.0)
    if BK >= 5:
        joints[3] = (stride * (H + rad) + 0.3, stride)                                   # just outside: zeros
        joints[4] = (2.0 * stride, float("nan"))
    got, ref, win = check(joints, H, sigma, rad, stride)
    if H == 6:
        assert win[0].all()                                                              # the window covers the whole map
        assert not win[3].any() and not win[4].any()
    if H == 1:
        assert win.all() and got.shape == (1, 1, 1)


def test_many_planes_per_workgroup_and_an_unaligned_output():
    """More planes than the launch has workgroups (8192), and H % 4 == 0 on an output that is not 16-byte aligned: the 4-byte form."""
    from hupr_amd import runtime as rt
    BK, H = 8192 + 37, 4
    rng = np.random.RandomState(5)
    joints = rng.uniform(-8, 24, (BK, 2)).astype(np.float32)
    check(joints, H, 2.0, 6, 4.0)
    j = torch.from_numpy(joints[:9]).cuda()
    buf = torch.full((9 * 16 + 1,), float("nan"), dtype=torch.float32, device="cuda")
    t = buf[1:]
    assert t.data_ptr() % 16 == 4
    rt.check(rt.lib().hupr_gaussian_targets_subpixel_f32(rt.ptr(j), t.data_ptr(), 9, H, 2.0, 6, 4.0, rt.stream()))
    ref, _ = ref_targets(joints[:9], H, 2.0, 6, 4.0)
    out = buf.cpu().numpy()
    assert np.isnan(out[0]) and np.abs(out[1:].reshape(9, H, H) - ref).max() <= TOL


# ---- 3: whole-pixel joints agree with today's targets -----------------------------------------------------------------------------------
def test_whole_pixel_joints_agree_with_the_integer_targets():
    """int64 joints: the same zero pattern as today's targets for every joint, and today's values where f == 0, i.e. for a joint on
    a whole heat-map pixel >= 0, on the map or beyond its far edge.  A NEGATIVE whole pixel is not such a joint: the truncating cast
    of both kernels gives mu = ac + 1 there (ac = -3: (int)(-2.5) = -2), so f = -1 — the same window, and by the rule the Gaussian
    on the joint where today's patch sits on mu.  Those planes are held to the rule's fp64 statement like every other."""
    from hupr_amd import functional as F_
    m = np.random.RandomState(7).randint(-12, 76, (2, 14, 2))                            # heat-map pixels, some outside the map
    m[0, 0], m[0, 1], m[0, 2], m[0, 3], m[0, 4] = (0, 0), (63, 63), (-7, 30), (70, 64), (-3, -1)
    j = torch.from_numpy(4 * m).cuda()
    assert j.dtype == torch.int64
    new, old = F_.gaussian_targets_subpixel(j.float()), F_.gaussian_targets(j)
    assert new.shape == old.shape == (2, 14, 64, 64) and new.dtype == torch.float32
    assert torch.equal(new == 0, old == 0)
    ref, win = ref_targets((4.0 * m).reshape(-1, 2), 64, 2.0, 6, 4.0)
    assert np.abs(new.cpu().numpy().reshape(28, 64, 64) - ref).max() <= TOL
    assert np.array_equal(new.cpu().numpy().reshape(28, 64, 64) != 0, win)
    whole = torch.from_numpy((m >= 0).all(axis=2))                                       # f == 0 on both axes
    assert 8 <= int(whole.sum()) < 28
    err = (new.double() - old.double())[whole].abs().max().item()
    print("whole-pixel joints: max |subpixel - integer| %.3e over %d planes" % (err, int(whole.sum())))
    assert err <= TOL
    assert torch.equal(F_.gaussian_targets_subpixel(j), new) and torch.equal(F_.gaussian_targets_subpixel(j.double()), new)
    for hsize, sigma in ((64, 2), (128, 3)):                                             # both sizes LossComputer knows
        jj = torch.from_numpy((256 // hsize) * np.random.RandomState(hsize).randint(0, hsize + 12, (1, 14, 2))).cuda()
        a, b = F_.gaussian_targets_subpixel(jj.float(), hsize, 256, sigma), F_.gaussian_targets(jj, hsize, 256, sigma)
        assert torch.equal(a == 0, b == 0) and (a - b).abs().max().item() <= TOL


# ---- 4: encode and decode are inverses -------------------------------------------------------------------------------------------------
def test_decode_returns_the_joints_that_were_encoded():
    from hupr_amd import functional as F_
    joints = np.random.RandomState(13).uniform(6.0, 246.0, (28 * 4, 2)).astype(np.float32)
    t = F_.gaussian_targets_subpixel(torch.from_numpy(joints.reshape(8, 14, 2)).cuda())
    _, mx, raw, _, _ = F_.pose_decode(t, 4.0, refine=True)
    err = np.abs(raw.cpu().numpy().reshape(-1, 2).astype(np.float64) - joints.astype(np.float64))
    print("encode -> decode: max |error| %.3e image pixel, mean %.3e" % (err.max(), err.mean()))
    assert err.max() <= TOL_DECODE_PX
    assert (mx.cpu().numpy() > 0.93).all()                                               # the peak: |f| <= 0.5 per axis, exp(-1/16)
    # the decode without refinement loses the fraction
    _, _, coarse, _, _ = F_.pose_decode(t, 4.0, refine=False)
    assert np.abs(coarse.cpu().numpy().reshape(-1, 2) - joints).max() > 1.5


# ---- 5: LossComputer -------------------------------------------------------------------------------------------------------------------
def _cfg(**training):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    for k, v in training.items():
        setattr(cfg.TRAINING, k, v)
    return cfg


def test_loss_computer_with_subpixel_targets():
    from hupr_amd.misc.losses import LossComputer
    import torch.nn.functional as F
    B, K, H = 2, 14, 64
    cfg = _cfg(targets="subpixel")
    lc = LossComputer(cfg, "cuda")
    assert lc.targets_mode == "subpixel"
    g = torch.Generator().manual_seed(21)
    p1 = torch.rand((B, K, 1, H, H), generator=g) * 0.98 + 0.01
    p2 = torch.rand((B, 1, K, H, H), generator=g) * 0.98 + 0.01
    # heat-map pixel m + fraction in [-0.45, 0.45]: the peak of the target is the pixel m, without a tie
    rng = np.random.RandomState(22)
    m, frac = rng.randint(3, 61, (B, K, 2)), rng.uniform(-0.45, 0.45, (B, K, 2))
    joints = torch.from_numpy((4.0 * (m + frac)).astype(np.float32))
    ref_t, _ = ref_targets(joints.numpy().reshape(-1, 2), H, 2.0, 6, 4.0)
    T = torch.from_numpy(ref_t).reshape(B, K, H, H)
    r1, r2 = p1.double().requires_grad_(True), p2.double().requires_grad_(True)
    l1, l2 = F.binary_cross_entropy(r1.reshape(B, K, H, H), T), F.binary_cross_entropy(r2.reshape(B, K, H, H), T)
    assert cfg.TRAINING.lossDecay == -1
    (l1 + l2).backward()                                                                 # lossDecay == -1: the plain sum
    a1, a2 = p1.cuda().requires_grad_(True), p2.cuda().requires_grad_(True)
    loss, loss2, pred, gt = lc.computeLoss((a1, a2), joints.cuda(), decode="device")
    loss.backward()
    # Tolerances: tests/test_ops_gpu.py::test_both_losses_and_their_weighted_sum_as_one_node checks these quantities with
    # close(..., 1e-6) (1e-6 of the reference's largest magnitude) where it does not ask for equal bits; an fp64 reference cannot
    # be met bit for bit, so 1e-6 it is, for the losses and for both gradients.
    for name, got, ref in (("loss", loss, l1 + l2), ("loss2", loss2, l2), ("dpreds1", a1.grad, r1.grad), ("dpreds2", a2.grad, r2.grad)):
        got, ref = got.detach().cpu().double(), ref.detach()
        err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
        print("%s: max err %.3e vs scale %.3e (rel %.3e)" % (name, err, scale, err / scale))
        assert err <= 1e-6 * scale, name
    # decode="device": the arg-max of the prediction and of the new targets
    want = (m[..., 1] * H + m[..., 0]).reshape(-1)
    assert np.array_equal(ref_t.reshape(B * K, -1).argmax(axis=1), want)
    assert np.array_equal(gt[0].cpu().numpy().astype(np.int64), want)
    assert np.array_equal(pred[0].cpu().numpy(), p2.reshape(B * K, -1).numpy().argmax(axis=1))
    # the host decode: gt2d is the arg-max of the same targets; integer joints mean whole pixels
    _, _, _, gt2d = lc.computeLoss((a1.detach(), a2.detach()), joints.cuda())
    assert np.array_equal(gt2d, m.astype(np.float32))
    whole = torch.from_numpy(4 * m)
    la, _, _, _ = lc.computeLoss((a1.detach(), a2.detach()), whole.cuda(), decode=False)
    lb, _, _, _ = lc.computeLoss((a1.detach(), a2.detach()), whole.float().cuda(), decode=False)
    assert torch.equal(la, lb)
    # the default is untouched by the new setting's existence
    li = LossComputer(_cfg(), "cuda")
    from hupr_amd import functional as F_
    assert li.targets_mode == "integer" and torch.equal(li.targets(whole), F_.gaussian_targets(whole.cuda()))


# ---- 6: the engine, eager and captured -------------------------------------------------------------------------------------------------
def test_graph_replay_matches_eager_steps_with_subpixel_targets():
    """tests/test_fullsize_gpu.py::test_graph_replay_matches_eager_steps at its size and with its bounds, the joints carrying a
    fraction: five eager steps against 2 eager + capture (1 warm-up step) + 2 replays, then one more step on OTHER joints, eager
    against replay — the static joints buffer of the graph is refilled, and keeps the joints' dtype."""
    from hupr_amd import functional as F_, synth
    from hupr_amd.tools.engine import TrainEngine
    try:
        F_.set_math("bf16")
        cfg = _cfg(targets="subpixel")
        dev = torch.device("cuda", 0)
        B, G = 4, cfg.DATASET.numGroupFrames
        adc_h = torch.from_numpy(synth.adc_cube_int16(31, sensor=0, nframes=B * G)).to(dev)
        adc_v = torch.from_numpy(synth.adc_cube_int16(31, sensor=1, nframes=B * G)).to(dev)
        frac = torch.rand((B, 14, 2), generator=torch.Generator().manual_seed(33))
        joints = (torch.from_numpy(synth.keypoints(B, 32)).float() + frac).to(dev)
        other = (torch.from_numpy(synth.keypoints(B, 34)).float() + frac.flip(0)).to(dev)
        assert joints.dtype == torch.float32 and (joints != joints.floor()).any()
        e1 = TrainEngine(cfg, device=dev, seed=0)
        assert e1.lossComputer.targets_mode == "subpixel"
        for _ in range(5):
            l1, _ = e1.train_step_from_adc(adc_h, adc_v, joints)
        e2 = TrainEngine(cfg, device=dev, seed=0)
        for _ in range(2):
            e2.train_step_from_adc(adc_h, adc_v, joints)
        with pytest.raises(RuntimeError):
            e2.capture(adc_h, adc_v, joints.long(), warmup=1)                            # an integer buffer would truncate
        e2.capture(adc_h, adc_v, joints, warmup=1)
        for _ in range(2):
            l2, _ = e2.train_step_from_adc(adc_h, adc_v, joints)
        torch.cuda.synchronize()

        def rel_params():
            p1 = torch.cat([p.detach().flatten() for p in e1.model.parameters()])
            p2 = torch.cat([p.detach().flatten() for p in e2.model.parameters()])
            assert torch.isfinite(p2).all()
            return ((p1 - p2).norm() / p1.norm()).item()
        rel = rel_params()
        print("after 5 steps: parameters rel %.3e, loss %.6f vs %.6f" % (rel, float(l1.detach()), float(l2.detach())))
        assert rel <= 1e-5, rel
        assert abs(float(l1.detach()) - float(l2.detach())) <= 1e-4 * abs(float(l1.detach()))
        # a sixth step on other joints
        assert e2._g_in[2].dtype == torch.float32 and torch.equal(e2._g_in[2], joints)
        l1, _ = e1.train_step_from_adc(adc_h, adc_v, other)
        l2, _ = e2.train_step_from_adc(adc_h, adc_v, other)
        torch.cuda.synchronize()
        assert torch.equal(e2._g_in[2], other)
        rel = rel_params()
        print("after a step on other joints: parameters rel %.3e, loss %.6f vs %.6f" % (rel, float(l1.detach()), float(l2.detach())))
        assert abs(float(l1.detach()) - float(l2.detach())) <= 1e-4 * abs(float(l1.detach()))
        assert rel <= 1e-5, rel
    finally:
        F_.set_math("f32")


# ---- 7: the Runner ---------------------------------------------------------------------------------------------------------------------
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


def test_runner_trains_on_subpixel_targets_and_prints_the_position_error(tmp_path, monkeypatch, capsys):
    import json
    import re
    run = _run_main(tmp_path, monkeypatch, "sub", targets="subpixel")
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("MPJPE:")]
    assert len(lines) == 1 and re.fullmatch(r"MPJPE: \d+\.\d{3} px \(n = 4\)", lines[0]), out
    assert "AP: " in out and len(json.load(open(run / "val_results.json"))) == 4
    assert os.path.exists(run / "checkpoint.pth") and os.path.exists(run / "train_loss_list_0.json")
    _run_main(tmp_path, monkeypatch, "plain")
    out = capsys.readouterr().out
    assert "AP: " in out and "MPJPE" not in out
