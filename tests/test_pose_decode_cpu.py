"""CPU (-m "not gpu"): the argument checks of the sub-pixel decode / One-Euro filter at every layer (C ABI through ctypes,
``PoseSmoothing``, ``TEST.decode``, ``PoseStream``), the register / scratch metadata of csrc/pose_decode.hip, and the checks every
wrapper makes on ``out=`` / ``stats=`` buffers of the caller's (the decodes, the tracker, arg-max, the presence gate, the FFT chain to
means, the interference filter).  No launch."""
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
    # clone() and cpu() keep the type and every field, those left None and those of a session with presence / interference
    fields = PoseFrame.__slots__ + ("present", "occupancy", "interference")
    full = PoseFrame(6, *t, present=torch.ones(1, dtype=torch.int32), occupancy=torch.full((1, 8), 2.0),
                     interference=torch.full((2, 1, 2), 9, dtype=torch.int32))
    for src in (pf, full, PoseFrame(3, *t[:5])):
        for c in (src.clone(), src.cpu()):
            assert type(c) is PoseFrame and c.frame == src.frame and not hasattr(c, "__dict__")
            for k in fields[1:]:
                a, b = getattr(src, k), getattr(c, k)
                assert (a is None and b is None) or (torch.equal(a, b) and a.dtype == b.dtype), k
    assert full.clone().occupancy is not full.occupancy and full.clone().interference is not None


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


# ---- out= / stats=: buffers the caller owns are checked before any launch ---------------------------------------------------------------
def _out_calls():
    """name -> (call(out), the well-formed ``out`` on CPU tensors) for every wrapper that writes into buffers of the caller's; a bare
    tensor where the function returns one."""
    from hupr_amd import functional as F_, preprocessing as pre
    from hupr_amd.tools import PoseSmoothing, PoseTracking
    i32, f32, lead = torch.int32, torch.float32, (2, 3)
    e = lambda tail, dt: torch.empty(lead + tail, dtype=dt)
    heat, sm, adc = torch.zeros(lead + (8, 8)), PoseSmoothing(10.0), torch.zeros((2, 4, 192, 256, 2), dtype=torch.int16)
    fstate, tstate, present = F_.pose_filter_state(6, "cpu"), F_.pose_track_state(6, "cpu"), torch.ones(2, dtype=i32)
    plain, filtered = (e((), i32), e((), f32), e((2,), f32), None, None), (e((), i32), e((), f32), e((2,), f32), e((2,), f32), e((2,), f32))
    track = filtered + (e((3,), f32), e((2,), f32), e((), i32))
    assoc = track + (e((2, 2), f32), e((2,), f32), e((), i32), e((), i32))
    return {
        "argmax_rows": (lambda out: F_.argmax_rows(heat.view(6, 64), out=out), (torch.empty(6, dtype=i32), torch.empty(6, dtype=f32))),
        "pose_decode": (lambda out: F_.pose_decode(heat, 4.0, out=out), plain),
        "pose_decode filter": (lambda out: F_.pose_decode(heat, 4.0, filter_state=fstate, smoothing=sm, out=out), filtered),
        "pose_decode_integral": (lambda out: F_.pose_decode_integral(heat, 4.0, 2, out=out), plain),
        "pose_decode_integral filter": (lambda out: F_.pose_decode_integral(heat, 4.0, 0, filter_state=fstate, smoothing=sm, out=out), filtered),
        "pose_track": (lambda out: F_.pose_track(heat, 4.0, track_state=tstate, tracking=PoseTracking(10.0), out=out), track),
        "pose_track candidates=2": (lambda out: F_.pose_track(heat, 4.0, track_state=tstate, tracking=PoseTracking(10.0, candidates=2),
                                                              out=out), assoc),
        "pose_track present": (lambda out: F_.pose_track(heat, 4.0, track_state=tstate, tracking=PoseTracking(10.0), present=present,
                                                         out=out), track + (e((1, 2), f32), e((1,), f32), e((), i32), e((), i32))),
        "presence_update": (lambda out: F_.presence_update(torch.zeros((2, 8)), F_.presence_state(2, "cpu"), out=out), torch.empty(2, dtype=i32)),
        "fft_chain_loader_means": (lambda out: pre.fft_chain_loader_means(adc, out=out), torch.empty((2, 16, 64, 64))),
        "fft_chain_loader_means tdm": (lambda out: pre.fft_chain_loader_means(adc, out=out, tdm_compensation=True), torch.empty((2, 16, 64, 64))),
        "adc_interference out": (lambda out: F_.adc_interference(adc, out=out), torch.empty_like(adc)),
        "adc_interference stats": (lambda out: F_.adc_interference(adc, stats=None if out is None else F_.InterferenceStats(*out)),
                                   (torch.empty((2, 2), dtype=i32), torch.empty((2, 12, 2), dtype=i32))),
    }


def _malformed(good):
    """Every way ``good`` (a tuple with Nones, or a bare tensor) can be wrong in one place -> [(what, out)]."""
    bare = isinstance(good, torch.Tensor)
    slots = (good,) if bare else good
    bad = [] if bare else [("one entry short", good[:-1]), ("one entry long", good + (good[0],))]
    for k, t in enumerate(slots):
        put = lambda v, k=k: v if bare else good[:k] + (v,) + good[k + 1:]
        if t is None:
            bad.append(("a tensor where slot %d is None" % k, put(torch.empty((2, 3, 2)))))
            continue
        bad += [("slot %d: shape" % k, put(t.new_empty(tuple(t.shape) + (1,)))), ("slot %d: dtype" % k, put(t.double())),
                ("slot %d: not contiguous" % k, put(t.new_empty(tuple(t.shape) + (2,))[..., 0])),
                ("slot %d: device" % k, put(torch.empty_like(t, device="meta"))), ("slot %d: no tensor" % k, put([0]))]
        if not bare:
            bad.append(("slot %d: None" % k, put(None)))
    return bad


@pytest.mark.parametrize("name", ["argmax_rows", "pose_decode", "pose_decode filter", "pose_decode_integral", "pose_decode_integral filter",
                                  "pose_track", "pose_track candidates=2", "pose_track present", "presence_update", "fft_chain_loader_means",
                                  "fft_chain_loader_means tdm", "adc_interference out", "adc_interference stats"])
def test_a_malformed_out_is_a_value_error_before_any_launch(L, name):
    from hupr_amd.runtime import HuprError
    call, good = _out_calls()[name]
    n0 = L.hupr_launch_count()
    cases = _malformed(good)
    assert len(cases) >= 5
    for what, out in cases:
        if name == "adc_interference stats" and len(out) != 2:
            continue                                                             # InterferenceStats takes its two tensors
        with pytest.raises(ValueError, match=r"\bout\b"):
            call(out)
            pytest.fail("%s: %s went through" % (name, what))
    # the well-formed one reaches the GPU check, like no out at all (presence_update's is torch.cuda.device's own, as before)
    reached = lambda: pytest.raises(ValueError, match="Expected a cuda device") if name == "presence_update" else pytest.raises(HuprError)
    with reached():
        call(good)
    with reached():
        call(None)
    assert L.hupr_launch_count() == n0


def test_stats_must_be_an_interference_stats(L):
    from hupr_amd import functional as F_
    adc = torch.zeros((1, 4, 192, 256, 2), dtype=torch.int16)
    n0 = L.hupr_launch_count()
    for stats in ((torch.empty((1, 2), dtype=torch.int32), torch.empty((1, 12, 2), dtype=torch.int32)), torch.empty((1, 2), dtype=torch.int32), 0):
        with pytest.raises(ValueError, match="InterferenceStats"):
            F_.adc_interference(adc, stats=stats)
    assert L.hupr_launch_count() == n0
