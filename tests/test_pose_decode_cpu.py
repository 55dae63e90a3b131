"""CPU (-m "not gpu"): the argument checks of the sub-pixel decode / One-Euro filter at every layer (C ABI through ctypes,
``PoseSmoothing``, ``TEST.decode``, ``PoseStream``), and the register / scratch metadata of csrc/pose_decode.hip.  No launch."""
import copy

import pytest
import torch

from listing import kernel_metadata


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


def _call(L, heat, rows, state, params, idx, mx, raw, kp=None, vel=None, H=64, W=64):
    return L.hupr_pose_decode_f32(heat, rows, H, W, 4.0, 1, state, *params, idx, mx, raw, kp, vel, None)


GOOD = (10.0, 1.0, 0.01, 1.0, 0.0)      # rate_hz, min_cutoff, beta, d_cutoff, min_score


def test_entry_points_check_their_arguments_on_the_host(L):
    p = 4096                                               # any non-null address: every call below returns before it launches
    assert L.hupr_pose_filter_state_bytes(0) == 0 and L.hupr_pose_filter_state_bytes(-3) == 0
    assert L.hupr_pose_filter_state_bytes(28) == 28 * 8 * 4
    # rows == 0 is a no-op whatever else is passed
    assert _call(L, None, 0, None, (0.0,) * 5, None, None, None) == 0
    assert _call(L, None, 0, p, (-1.0,) * 5, None, None, None) == 0
    # null pointers
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        heat, idx, mx, raw = args
        assert _call(L, heat, 14, None, (0.0,) * 5, idx, mx, raw) == -1
        assert b"null" in L.hupr_last_error()
    # shapes
    assert _call(L, p, -1, None, (0.0,) * 5, p, p, p) == -1 and b"shape" in L.hupr_last_error()
    assert _call(L, p, 1 << 31, None, (0.0,) * 5, p, p, p) == -1
    assert _call(L, p, 14, None, (0.0,) * 5, p, p, p, H=0) == -1
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
    p = 4096
    assert _call(L, p, 14, p, params, p, p, p, kp=p, vel=p) == -1
    assert b"filter parameter" in L.hupr_last_error()


def test_pose_smoothing_validates_on_the_host():
    from hupr_amd import tools
    from hupr_amd.tools import stream as st
    assert tools.PoseSmoothing is st.PoseSmoothing
    assert issubclass(st.SmoothingError, st.StreamError) and issubclass(st.DecodeError, st.StreamError)
    s = st.PoseSmoothing(10)
    assert (s.rate_hz, s.min_cutoff, s.beta, s.d_cutoff, s.min_score) == (10.0, 1.0, 0.01, 1.0, 0.0)
    assert all(isinstance(getattr(s, k), float) for k in s.__slots__)
    st.PoseSmoothing(30.0, min_cutoff=0.5, beta=0.0, d_cutoff=2.0, min_score=-1.0)
    for bad in (dict(rate_hz=0), dict(rate_hz=-10.0), dict(rate_hz=float("nan")), dict(rate_hz=float("inf")), dict(rate_hz="10"),
                dict(rate_hz=None), dict(rate_hz=True), dict(rate_hz=10, min_cutoff=0.0), dict(rate_hz=10, min_cutoff=-1.0),
                dict(rate_hz=10, beta=-1e-3), dict(rate_hz=10, d_cutoff=0), dict(rate_hz=10, d_cutoff=float("nan")),
                dict(rate_hz=10, min_score=float("nan")), dict(rate_hz=10, min_score="0")):
        with pytest.raises(st.SmoothingError):
            st.PoseSmoothing(**bad)


def test_test_decode_is_validated_where_the_config_is_read():
    from hupr_amd.config_tree import load_config
    from hupr_amd.misc.losses import LossComputer
    from hupr_amd.misc.metrics import decode_setting
    cfg = load_config()
    assert not hasattr(cfg.TEST, "decode")                       # the shipped YAML is the reference's
    assert decode_setting(cfg) == "argmax" and LossComputer(cfg, "cpu").decode == "argmax"
    for name in ("argmax", "subpixel"):
        c = copy.deepcopy(cfg)
        c.TEST.decode = name
        assert decode_setting(c) == name and LossComputer(c, "cpu").decode == name
    for bogus in ("dark", "", None, 1, "Subpixel"):
        c = copy.deepcopy(cfg)
        c.TEST.decode = bogus
        with pytest.raises(ValueError):
            LossComputer(c, "cpu")


def test_functional_pose_decode_refuses_bad_arguments_and_cpu_tensors():
    from hupr_amd import functional as F_
    from hupr_amd.runtime import HuprError
    from hupr_amd.tools.stream import PoseSmoothing
    import __graft_entry__ as g
    g.build()
    heat = torch.zeros((2, 8, 8))
    with pytest.raises(ValueError):
        F_.pose_decode(torch.zeros(8), 4.0)
    with pytest.raises(ValueError):
        F_.pose_decode(heat.double(), 4.0)
    with pytest.raises(ValueError):
        F_.pose_decode(heat, 4.0, smoothing=PoseSmoothing(10.0))                 # a filter needs its state
    with pytest.raises(ValueError):
        F_.pose_decode(heat, 4.0, filter_state=torch.zeros((2, 8)))
    with pytest.raises(ValueError):
        F_.pose_decode(heat, 4.0, filter_state=torch.zeros((3, 8)), smoothing=PoseSmoothing(10.0))
    with pytest.raises(HuprError):                                               # no CPU fallback
        F_.pose_decode(heat, 4.0)


def test_session_argument_errors_come_before_the_gpu_check():
    from hupr_amd import tools
    from hupr_amd.config_tree import load_config
    from hupr_amd.runtime import HuprError

    class _Cpu(torch.nn.Module):
        math_mode, numFilters = None, 32

        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

    cfg = load_config()
    with pytest.raises(tools.DecodeError):
        tools.PoseStream(_Cpu(), cfg, decode="dark")
    with pytest.raises(tools.DecodeError):
        tools.PoseStream(_Cpu(), cfg, decode=None)
    with pytest.raises(tools.SmoothingError):
        tools.PoseStream(_Cpu(), cfg, smooth=10.0)
    with pytest.raises(tools.SmoothingError):
        tools.PoseStream(_Cpu(), cfg, decode="subpixel", smooth=(10.0, 1.0, 0.01, 1.0, 0.0))
    with pytest.raises(tools.StreamError):
        tools.PoseStream(_Cpu(), cfg, smooth=tools.PoseSmoothing(0.0))           # raised by PoseSmoothing itself
    with pytest.raises(HuprError):                                               # valid arguments reach the GPU check
        tools.PoseStream(_Cpu(), cfg, decode="subpixel", smooth=tools.PoseSmoothing(10.0))


def test_pose_frame_carries_raw_keypoints_and_velocity():
    from hupr_amd.tools.stream import PoseFrame
    assert PoseFrame.__slots__[-2:] == ("raw_keypoints", "velocity")
    t = [torch.full((1,), float(i)) for i in range(7)]
    pf = PoseFrame(3, *t[:5])
    assert pf.raw_keypoints is pf.keypoints and pf.velocity is None
    c = pf.clone()                                                               # _map passes None through
    assert c.velocity is None and torch.equal(c.raw_keypoints, pf.keypoints) and c.frame == 3
    pf = PoseFrame(4, *t)
    assert pf.raw_keypoints is t[5] and pf.velocity is t[6] and torch.equal(pf.cpu().velocity, t[6])


def test_stream_command_needs_a_rate_to_smooth():
    from hupr_amd.tools import stream as st
    a = st.parse(["--raw", "x"])
    assert a.decode == "argmax" and not a.smooth and a.rate is None
    a = st.parse(["--raw", "x", "--decode", "subpixel", "--smooth", "--rate", "10"])
    assert a.decode == "subpixel" and a.smooth and a.rate == 10.0
    with pytest.raises(SystemExit):
        st.parse(["--raw", "x", "--smooth"])
    with pytest.raises(SystemExit):
        st.parse(["--raw", "x", "--decode", "dark"])


def test_pose_decode_kernel_uses_no_scratch():
    """The listing the build keeps for csrc/pose_decode.hip: its one kernel with 0 spilled registers, 0 bytes of scratch, no LDS."""
    meta = kernel_metadata("pose_decode")
    assert len(meta) == 1 and "hupr_k_pose_decode" in next(iter(meta)), sorted(meta)
    assert "hupr_k_stream_keypoints" not in next(iter(meta))
    m = next(iter(meta.values()))
    assert m["spill"] == 0 and m["sspill"] == 0 and m["scratch"] == 0 and m["lds"] == 0, m
    assert m["threads"] == 64 and m["vgpr"] <= 64, m
