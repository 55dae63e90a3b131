"""CPU (-m "not gpu"): the sub-pixel Gaussian targets at every layer short of a launch — the argument checks of
hupr_gaussian_targets_subpixel_f32 through ctypes, ``TRAINING.targets`` / ``LossComputer.targets_mode``, ``tools.run.loss_labels``,
``functional.gaussian_targets_subpixel``'s argument handling, ``misc.oks_eval.mean_position_error`` on hand-built records, and the
register / scratch metadata of csrc/targets.hip."""
import copy

import numpy as np
import pytest
import torch

from listing import kernel_metadata


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


P = 4096                                                   # any non-null address: every call below returns before it launches


def _call(L, joints=P, t=P, BK=28, H=64, sigma=2.0, rad=6, stride=4.0):
    return L.hupr_gaussian_targets_subpixel_f32(joints, t, BK, H, sigma, rad, stride, None)


def test_entry_point_checks_its_arguments_on_the_host(L):
    inf, nan = float("inf"), float("nan")
    # BK == 0 is a no-op whatever else is passed
    assert _call(L, None, None, BK=0, H=0, sigma=nan, rad=0, stride=-1.0) == 0
    refused = [dict(joints=None), dict(t=None), dict(joints=None, t=None),
               dict(BK=-1), dict(BK=-(1 << 40)), dict(BK=1 << 62, H=4096), dict(BK=(1 << 63) - 1, H=1), dict(BK=1 << 40, H=4096),
               dict(H=0), dict(H=-64), dict(H=4097), dict(H=1 << 30),
               dict(rad=0), dict(rad=-6),
               dict(sigma=0.0), dict(sigma=-2.0), dict(sigma=nan), dict(sigma=inf), dict(sigma=-inf),
               dict(stride=0.0), dict(stride=-4.0), dict(stride=nan), dict(stride=inf), dict(stride=-inf)]
    for kw in refused:
        assert _call(L, **kw) == -1, kw
        msg = L.hupr_last_error()
        assert msg.startswith(b"hupr_gaussian_targets_subpixel_f32: ") and len(msg) > 40, (kw, msg)
    assert _call(L, joints=None) == -1 and b"null" in L.hupr_last_error()
    assert _call(L, H=4097) == -1 and b"H 4097" in L.hupr_last_error()
    assert _call(L, BK=-1) == -1 and b"BK -1" in L.hupr_last_error()
    assert _call(L, rad=0) == -1 and b"rad 0" in L.hupr_last_error()
    assert _call(L, sigma=nan) == -1 and b"sigma" in L.hupr_last_error()
    assert _call(L, stride=0.0) == -1 and b"stride" in L.hupr_last_error()


def test_training_targets_is_validated_where_the_config_is_read():
    from hupr_amd.config_tree import load_config
    from hupr_amd.misc.losses import LossComputer, targets_setting
    cfg = load_config()
    assert not hasattr(cfg.TRAINING, "targets")                  # the shipped YAML is the reference's
    assert targets_setting(cfg) == "integer" and LossComputer(cfg, "cpu").targets_mode == "integer"
    for name in ("integer", "subpixel"):
        c = copy.deepcopy(cfg)
        c.TRAINING.targets = name
        assert targets_setting(c) == name and LossComputer(c, "cpu").targets_mode == name
    for bogus in ("dark", "", None, 1, "Subpixel"):
        c = copy.deepcopy(cfg)
        c.TRAINING.targets = bogus
        with pytest.raises(ValueError):
            targets_setting(c)
        with pytest.raises(ValueError):
            LossComputer(c, "cpu")


def test_loss_labels_picks_the_joints_the_setting_asks_for():
    from hupr_amd.tools.run import loss_labels
    ints = torch.tensor([[[10, 20], [30, 41]]], dtype=torch.int64)
    flts = torch.tensor([[[10.25, 20.75], [30.5, 41.999]]], dtype=torch.float64)
    batch = {"jointsGroup": ints, "jointsFloat": flts}
    assert loss_labels(batch, "integer") is ints
    got = loss_labels(batch, "subpixel")
    assert got.dtype == torch.float32 and torch.equal(got, flts.float())
    assert not torch.equal(got, ints.float())                    # the fractions are kept
    assert loss_labels({"jointsGroup": ints}, "integer") is ints
    with pytest.raises(KeyError) as e:
        loss_labels({"jointsGroup": ints}, "subpixel")
    assert "TRAINING.targets" in str(e.value) and "jointsFloat" in str(e.value)
    with pytest.raises(ValueError):
        loss_labels(batch, "dark")


def test_functional_refuses_bad_arguments_and_cpu_tensors():
    from hupr_amd import functional as F_
    from hupr_amd.runtime import HuprError
    import __graft_entry__ as g
    g.build()
    for bad in (torch.zeros(14, 2), torch.zeros(2, 14, 3), torch.zeros(2, 14, 2, 1), torch.zeros(28), [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            F_.gaussian_targets_subpixel(bad)
    for dtype in (torch.bool, torch.complex64):
        with pytest.raises(ValueError):
            F_.gaussian_targets_subpixel(torch.zeros((2, 14, 2), dtype=dtype))
    for dtype in (torch.float32, torch.float64, torch.float16, torch.int64, torch.int32):
        with pytest.raises(HuprError):                                           # no CPU fallback
            F_.gaussian_targets_subpixel(torch.zeros((2, 14, 2), dtype=dtype))


def test_mean_position_error_on_hand_built_records():
    from hupr_amd.misc.oks_eval import make_gt, mean_position_error
    K = 14
    base = np.stack([np.arange(K) * 10.0, np.arange(K) * 5.0 + 0.5], axis=1)     # (K, 2)

    def det(iid, xy):
        return {"image_id": iid, "keypoints": np.concatenate([xy, np.ones((K, 1))], axis=1).reshape(-1).tolist(), "score": 1.0}

    off_345 = np.tile([3.0, 4.0], (K, 1))                                        # every joint 5 px away
    off_one = np.zeros((K, 2))
    off_one[2] = [0.0, -2.0]                                                     # joint 2 alone, 2 px away
    gts = [{"image_id": 1, "keypoints": base, "bbox": np.array([0.0, 0.0, 100.0, 100.0])},       # the Runner's (K, 2) form
           make_gt(2, base + 100.0, [0, 0, 50, 80]),                                               # the full COCO-style form
           {"image_id": 3, "keypoints": base, "bbox": np.array([0.0, 0.0, 100.0, 100.0])}]       # no detection: not counted
    dts = [det(1, base + off_345), det(2, base + 100.0 + off_one), det(9, base)]                   # 9: no ground truth
    mean, per_joint, n = mean_position_error(gts, dts)
    assert n == 2
    want = np.full(K, 2.5)
    want[2] = 3.5
    assert isinstance(per_joint, np.ndarray) and per_joint.shape == (K,) and np.array_equal(per_joint, want)
    assert mean == (5.0 * K + 2.0) / (2 * K)
    # an exact hit is 0; nothing matched is not a number, not an error
    mean, per_joint, n = mean_position_error(gts[:1], [det(1, base)])
    assert mean == 0.0 and n == 1 and not per_joint.any()
    mean, per_joint, n = mean_position_error(gts, dts[2:])
    assert n == 0 and np.isnan(mean) and np.isnan(per_joint).all()


def test_targets_kernels_use_no_scratch():
    """The listing the build keeps for csrc/targets.hip: the two forms of its one kernel (16-byte and 4-byte stores) and nothing else,
    0 spilled registers, 0 bytes of scratch, no LDS, at most 64 VGPRs."""
    meta = kernel_metadata("targets")
    assert len(meta) == 2 and all("hupr_k_gaussian_targets_subpixel" in name for name in meta), sorted(meta)
    assert {name[name.index("subpixelILb"):][:13] for name in meta} == {"subpixelILb0E", "subpixelILb1E"}, sorted(meta)
    for name, m in meta.items():
        assert m["spill"] == 0 and m["sspill"] == 0 and m["scratch"] == 0 and m["lds"] == 0, (name, m)
        assert m["threads"] == 256 and m["vgpr"] <= 64, (name, m)
