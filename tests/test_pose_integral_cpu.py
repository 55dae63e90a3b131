"""CPU (-m "not gpu"): the integral decode without a launch — the argument checks at every layer (C ABI through ctypes,
``functional.pose_decode_integral``, ``TEST.decode: integral`` / ``TEST.decodeRadius``, ``PoseStream``, the stream command), the
register / scratch metadata of csrc/pose_integral.hip, and what the rule is worth, on its fp64 restatement (tests/pose_integral_ref.py):
against the restated Taylor decode under noise, and on clean targets."""
import copy

import numpy as np
import pytest
import torch

import pose_integral_ref as ref
from hupr_amd.misc.metrics import default_decode_radius
from test_pose_decode_gpu import ref_decode as ref_taylor          # the fp64 restatement of hupr_pose_decode_f32's Taylor step
from listing import kernel_metadata

GOOD = (10.0, 1.0, 0.01, 1.0, 0.0)      # rate_hz, min_cutoff, beta, d_cutoff, min_score


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


def _call(L, heat, rows, state, params, idx, mx, raw, kp=None, vel=None, H=64, W=64, radius=6):
    return L.hupr_pose_decode_integral_f32(heat, rows, H, W, 4.0, radius, state, *params, idx, mx, raw, kp, vel, None)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_entry_point_checks_its_arguments_on_the_host(L):
    p = 4096                                               # any non-null address: every call below returns before it launches
    # rows == 0 is a no-op whatever else is passed
    assert _call(L, None, 0, None, (0.0,) * 5, None, None, None) == 0
    assert _call(L, None, 0, p, (-1.0,) * 5, None, None, None, radius=-1) == 0
    for heat, idx, mx, raw in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert _call(L, heat, 14, None, (0.0,) * 5, idx, mx, raw) == -1
        assert b"null" in L.hupr_last_error()
    for radius in (-1, -6, -(1 << 31)):
        assert _call(L, p, 14, None, (0.0,) * 5, p, p, p, radius=radius) == -1 and b"radius" in L.hupr_last_error()
    assert _call(L, p, -1, None, (0.0,) * 5, p, p, p) == -1 and b"shape" in L.hupr_last_error()
    assert _call(L, p, 1 << 31, None, (0.0,) * 5, p, p, p) == -1
    assert _call(L, p, 14, None, (0.0,) * 5, p, p, p, H=0) == -1 and b"shape" in L.hupr_last_error()
    assert _call(L, p, 14, None, (0.0,) * 5, p, p, p, W=0) == -1
    assert _call(L, p, 14, None, (0.0,) * 5, p, p, p, W=-2) == -1
    assert _call(L, p, 14, None, (0.0,) * 5, p, p, p, H=1 << 16, W=1 << 16) == -1
    # filtered outputs need a filter state
    assert _call(L, p, 14, None, GOOD, p, p, p, kp=p) == -1 and b"filter state" in L.hupr_last_error()
    assert _call(L, p, 14, None, GOOD, p, p, p, vel=p) == -1


@pytest.mark.parametrize("params", [(0.0, 1.0, 0.01, 1.0, 0.0), (-10.0, 1.0, 0.01, 1.0, 0.0), (10.0, 0.0, 0.01, 1.0, 0.0),
                                    (10.0, -1.0, 0.01, 1.0, 0.0), (10.0, 1.0, -0.01, 1.0, 0.0), (10.0, 1.0, 0.01, 0.0, 0.0),
                                    (10.0, 1.0, 0.01, -2.0, 0.0), (float("nan"), 1.0, 0.01, 1.0, 0.0),
                                    (float("inf"), 1.0, 0.01, 1.0, 0.0), (10.0, 1.0, float("nan"), 1.0, 0.0),
                                    (10.0, 1.0, 0.01, 1.0, float("nan"))])
def test_a_bad_filter_parameter_is_refused(L, params):
    """The filter-argument errors of hupr_pose_decode_f32, the same list as tests/test_pose_decode_cpu.py."""
    p = 4096
    assert _call(L, p, 14, p, params, p, p, p, kp=p, vel=p) == -1
    assert b"filter parameter" in L.hupr_last_error()


def test_functional_pose_decode_integral_refuses_what_pose_decode_refuses(L):
    from hupr_amd import functional as F_
    from hupr_amd.runtime import HuprError
    from hupr_amd.tools.stream import PoseSmoothing
    heat = torch.zeros((2, 8, 8))
    with pytest.raises(ValueError):
        F_.pose_decode_integral(torch.zeros(8), 4.0, 2)
    with pytest.raises(ValueError):
        F_.pose_decode_integral(heat.double(), 4.0, 2)
    for radius in (-1, 1.0, "2", None, True):
        with pytest.raises(ValueError):
            F_.pose_decode_integral(heat, 4.0, radius)
    with pytest.raises(ValueError):
        F_.pose_decode_integral(heat, 4.0, 2, smoothing=PoseSmoothing(10.0))         # a filter needs its state
    with pytest.raises(ValueError):
        F_.pose_decode_integral(heat, 4.0, 2, filter_state=torch.zeros((2, 8)))
    with pytest.raises(ValueError):
        F_.pose_decode_integral(heat, 4.0, 2, filter_state=torch.zeros((3, 8)), smoothing=PoseSmoothing(10.0))
    with pytest.raises(HuprError):                                                   # no CPU fallback
        F_.pose_decode_integral(heat, 4.0, 2)
    with pytest.raises(HuprError):
        F_.pose_decode_integral(heat, 4.0, 0)


# ---- the config ---------------------------------------------------------------------------------------------------------------------------
def test_test_decode_integral_and_its_radius_are_validated_where_the_config_is_read():
    from hupr_amd.config_tree import load_config
    from hupr_amd.misc.losses import LossComputer
    from hupr_amd.misc.metrics import DECODES, decode_radius_setting, decode_setting
    assert DECODES == ("argmax", "subpixel", "integral")
    cfg = load_config()
    assert not hasattr(cfg.TEST, "decode") and not hasattr(cfg.TEST, "decodeRadius")       # the shipped YAML is the reference's
    lc = LossComputer(cfg, "cpu")
    assert lc.decode == "argmax" and lc.decodeRadius is None and decode_radius_setting(cfg) is None

    def with_keys(size=64, **test):
        c = copy.deepcopy(cfg)
        c.DATASET.heatmapSize = size
        for k, v in test.items():
            setattr(c.TEST, k, v)
        return c

    # the default per map size: the targets' patch radius, 3 sigma
    for size, want in ((64, 6), (128, 9)):
        c = with_keys(size, decode="integral")
        assert decode_setting(c) == "integral" and decode_radius_setting(c) == want
        lc = LossComputer(c, "cpu")
        assert lc.decode == "integral" and lc.decodeRadius == want and type(lc.decodeRadius) is int
    for size, radius in ((64, 0), (64, 1), (64, 6), (64, 63), (128, 127), (128, 0)):
        lc = LossComputer(with_keys(size, decode="integral", decodeRadius=radius), "cpu")
        assert lc.decodeRadius == radius and type(lc.decodeRadius) is int
    for size, bad in ((64, True), (64, False), (64, 6.0), (64, 0.0), (64, "6"), (64, None), (64, -1), (64, 64), (64, 1000), (128, 128),
                      (64, [6]), (64, float("nan"))):
        with pytest.raises(ValueError):
            LossComputer(with_keys(size, decode="integral", decodeRadius=bad), "cpu")
    # the radius belongs to the integral decode alone
    for other in ({}, {"decode": "argmax"}, {"decode": "subpixel"}):
        with pytest.raises(ValueError):
            LossComputer(with_keys(decodeRadius=6, **other), "cpu")
        with pytest.raises(ValueError):
            LossComputer(with_keys(decodeRadius=0, **other), "cpu")
    # the other decodes are what they were, and an unknown one is still refused
    for name in ("argmax", "subpixel"):
        lc = LossComputer(with_keys(decode=name), "cpu")
        assert lc.decode == name and lc.decodeRadius is None
    for bogus in ("dark", "", None, 1, "Integral", "centroid"):
        with pytest.raises(ValueError):
            LossComputer(with_keys(decode=bogus), "cpu")
    with pytest.raises(ValueError):
        LossComputer(with_keys(decode="dark", decodeRadius=6), "cpu")


# ---- the session and the command ------------------------------------------------------------------------------------------------------------
def test_session_argument_errors_come_before_the_gpu_check():
    from hupr_amd import tools
    from hupr_amd.config_tree import load_config
    from hupr_amd.runtime import HuprError
    from hupr_amd.tools import stream as st

    class _Cpu(torch.nn.Module):
        math_mode, numFilters = None, 32

        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

    cfg = load_config()
    assert st.DECODES == ("argmax", "subpixel", "integral")
    with pytest.raises(tools.TrackingError):
        tools.PoseStream(_Cpu(), cfg, decode="integral", track=tools.PoseTracking(10.0))
    with pytest.raises(tools.TrackingError):
        tools.PoseStream(_Cpu(), cfg, decode="integral", decode_radius=3, track=tools.PoseTracking(10.0), predict_now=True)
    for other in ("argmax", "subpixel"):
        with pytest.raises(tools.DecodeError):
            tools.PoseStream(_Cpu(), cfg, decode=other, decode_radius=6)
        with pytest.raises(tools.DecodeError):
            tools.PoseStream(_Cpu(), cfg, decode=other, decode_radius=0, smooth=tools.PoseSmoothing(10.0))
    with pytest.raises(tools.DecodeError):
        tools.PoseStream(_Cpu(), cfg, decode_radius=6)
    for bad in (-1, 64, 1000, 6.0, "6", True):
        with pytest.raises(tools.DecodeError):
            tools.PoseStream(_Cpu(), cfg, decode="integral", decode_radius=bad)
    with pytest.raises(tools.DecodeError):
        tools.PoseStream(_Cpu(), cfg, decode="dark")
    with pytest.raises(tools.SmoothingError):
        tools.PoseStream(_Cpu(), cfg, decode="integral", smooth=10.0)
    # valid arguments reach the GPU check
    for kw in (dict(), dict(decode_radius=0), dict(decode_radius=63), dict(smooth=tools.PoseSmoothing(10.0)),
               dict(decode_radius=3, smooth=tools.PoseSmoothing(10.0))):
        with pytest.raises(HuprError):
            tools.PoseStream(_Cpu(), cfg, decode="integral", **kw)
    # the radius the session would run at
    assert st.check_decode("integral", None, None, 64) == 6 and st.check_decode("integral", None, None, 128) == 9
    assert st.check_decode("integral", None, 0, 64) == 0 and st.check_decode("integral", None, 11, 64) == 11
    assert st.check_decode("subpixel", None) is None and st.check_decode("argmax", None, None, 64) is None


def test_pose_frame_is_unchanged():
    from hupr_amd.tools.stream import PoseFrame
    assert PoseFrame.__slots__ == ("frame", "keypoints", "scores", "indices", "heatmap", "gcn_heatmap", "raw_keypoints", "velocity")


def test_stream_command_takes_the_integral_decode():
    from hupr_amd.tools import stream as st
    a = st.parse(["--raw", "x"])
    assert a.decode == "argmax" and a.decode_radius is None
    a = st.parse(["--raw", "x", "--decode", "integral"])
    assert a.decode == "integral" and a.decode_radius is None and not a.smooth
    a = st.parse(["--raw", "x", "--decode", "integral", "--decode-radius", "4", "--smooth", "--rate", "10"])
    assert a.decode == "integral" and a.decode_radius == 4 and a.smooth and a.rate == 10.0
    assert st.parse(["--raw", "x", "--decode", "integral", "--decode-radius", "0"]).decode_radius == 0
    for bad in (["--decode-radius", "4"], ["--decode", "subpixel", "--decode-radius", "4"], ["--decode", "argmax", "--decode-radius", "0"],
                ["--decode", "integral", "--decode-radius", "-1"], ["--decode", "integral", "--decode-radius", "2.5"],
                ["--decode", "integral", "--track", "--rate", "10"], ["--decode", "integral", "--decode-radius", "3", "--track", "--rate", "10"],
                ["--decode", "dark"]):
        with pytest.raises(SystemExit):
            st.parse(["--raw", "x"] + bad)


# ---- the listing ----------------------------------------------------------------------------------------------------------------------------
def test_pose_integral_kernel_uses_no_scratch():
    """The listing the build keeps for csrc/pose_integral.hip: its one kernel, 64 threads, with 0 spilled registers, 0 bytes of scratch
    and no LDS — read from the code-object metadata only."""
    meta = kernel_metadata("pose_integral")
    assert len(meta) == 1 and "hupr_k_pose_decode_integral" in next(iter(meta)), sorted(meta)
    m = next(iter(meta.values()))
    print(m)
    assert m["spill"] == 0 and m["sspill"] == 0 and m["scratch"] == 0 and m["lds"] == 0, m
    assert m["threads"] == 64 and m["vgpr"] <= 64, m


# ---- what the rule is worth, on its restatement ---------------------------------------------------------------------------------------------
def test_the_restatement_on_hand_worked_planes():
    """Windows clipped by a corner, the whole plane, a NaN and a negative pixel in the window, a tie, an empty and a negative plane:
    the restatement against answers worked by hand.  tests/test_pose_integral_gpu.py holds the kernel to the restatement."""
    m = np.zeros((7, 5, 7), dtype=np.float32)
    m[0, 0, 0], m[0, 0, 1], m[0, 1, 0] = 0.5, 0.25, 0.25            # corner (0, 0): mass 1, Mx = My = 0.25
    m[1, 4, 6], m[1, 4, 5], m[1, 2, 6] = 0.5, 0.25, 0.25            # corner (6, 4): (6 - 0.25, 4 - 0.5) at r >= 2, y untouched at r = 1
    m[2, 2, 3], m[2, 2, 4], m[2, 2, 2], m[2, 1, 3] = 0.75, np.nan, -3.0, 0.25   # the NaN and the negative weigh nothing
    m[3, 1, 2] = m[3, 3, 5] = 0.75                                   # a tie: the first wins, the second lies outside r = 1
    m[5] = -1.0
    m[6, 2, 3], m[6, 0, 0] = 0.5, 0.5                                # whole plane: the far corner counts; tie -> (0, 0) is the peak
    r1, r2, r0 = ref.ref_integral(m, 1), ref.ref_integral(m, 2), ref.ref_integral(m, 0)
    assert r1["idx"].tolist() == [0, 34, 17, 9, 0, 0, 0] and np.array_equal(r1["idx"], r0["idx"])
    assert r1["pos"][0].tolist() == [0.25, 0.25] and r1["cells"][0] == 4 and r2["cells"][0] == 9
    assert r1["pos"][1].tolist() == [6 - 1.0 / 3.0, 4.0] and r2["pos"][1].tolist() == [5.75, 3.5]
    assert r1["pos"][2].tolist() == [3.0, 1.75]
    assert r1["pos"][3].tolist() == [2.0, 1.0] and r0["pos"][3].tolist() == [3.5, 2.0]
    for r in (r1, r2, r0):
        assert not r["pos"][4].any() and not r["pos"][5].any() and not r["off"][4].any() and r["cells"][4] == 0
    assert r1["pos"][6].tolist() == [0.0, 0.0] and r0["pos"][6].tolist() == [1.5, 1.0] and r0["cells"][6] == 35
    for big in (6, 7, 1000):                                         # any radius >= max(H, W) - 1 is the whole plane
        rb = ref.ref_integral(m, big)
        assert np.array_equal(rb["pos"], r0["pos"]) and np.array_equal(rb["cells"], r0["cells"])


@pytest.mark.parametrize("level", ref.NOISE_LEVELS)
def test_the_windowed_centroid_beats_the_taylor_step_under_noise(level):
    """2 000 planes of 0.8 * target + N(0, level), clipped to [1e-4, 1]: the integral decode at radius 6 has a strictly smaller mean
    and 99th-percentile error than the Taylor decode, both as their fp64 restatements."""
    planes, centres = ref.noise_case(level)
    radius = default_decode_radius(64)                               # what TEST.decode: integral and PoseStream run at
    assert planes.shape == (2000, 64, 64) and radius == 6
    integral = ref.error_stats(ref.ref_integral(planes, radius)["pos"], centres)
    taylor = ref.error_stats(ref_taylor(planes)["pos"], centres)
    argmax = ref.error_stats(ref_taylor(planes, refine=False)["pos"], centres)
    print("noise %.2f: mean (p99) error in heat-map px: arg-max %.3f (%.3f), Taylor %.3f (%.3f), centroid r = 6 %.3f (%.3f)"
          % ((level,) + argmax + taylor + integral))
    assert integral[0] < taylor[0] and integral[1] < taylor[1]
    assert taylor[0] < argmax[0]                                     # the planes are such that refinement helps at all


def test_clean_targets_are_inverted_to_a_hundredth_of_a_pixel():
    """Clean targets whose patch is unclipped (centres in [6, 57]): the window of radius 6 around the peak is the patch, and its centroid
    is the joint up to the truncation of the Gaussian's tails, at most 0.01 heat-map px — the bound tests/test_coord_loss_gpu.py uses
    for the same truncation over the whole plane, which is the same sum here (the plane is zero outside the patch)."""
    centres = np.random.RandomState(7).uniform(6.0, 57.0, (2000, 2))
    planes = ref.target_planes(centres)
    assert default_decode_radius(64) == 6
    got = ref.ref_integral(planes, default_decode_radius(64))
    err = np.abs(got["pos"] - centres)
    print("clean targets: max |error| %.4f px per axis, %.4f px Euclidean" % (err.max(), np.sqrt((err ** 2).sum(axis=1)).max()))
    assert np.sqrt((err ** 2).sum(axis=1)).max() <= 0.01
    assert np.abs(ref.ref_integral(planes, 0)["pos"] - got["pos"]).max() < 1e-12         # the plane is zero outside the patch
    # a radius of 3 is too small for sigma 2: it shrinks the offset
    small = np.abs(ref.ref_integral(planes, 3)["pos"] - centres)
    assert small.mean() > 10 * err.mean()
