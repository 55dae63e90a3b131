"""CPU: the live stream's window rule and emission schedule against the loader's ``window_indices``, and the session's argument
errors (hupr_amd.tools.stream — host arithmetic only, no GPU)."""
import pytest
import torch

from hupr_amd.datasets.dataset import window_indices
from listing import kernel_metadata

DURATIONS = (1, 2, 3, 5, 8, 20, 600)
GROUPS = (2, 4, 8)


def _run(D, G, lookahead=None):
    """Push D frames, flush -> ([window per emitted pose, in emission order], [emitted per push], number flushed)."""
    from hupr_amd.tools.stream import StreamSchedule
    s = StreamSchedule(G, lookahead)
    windows, centers, per_push = [], [], []
    for n in range(D):
        due = s.push()
        per_push.append(0 if due is None else 1)
        assert s.frames_pushed == n + 1
        if due is not None:
            centers.append(due[0])
            windows.append(due[1])
    tail = s.flush()
    for c, w in tail:
        centers.append(c)
        windows.append(w)
    assert s.frames_emitted == len(windows)
    return windows, centers, per_push, len(tail)


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("D", DURATIONS)
def test_default_lookahead_reproduces_window_indices(D, G):
    """Pushing a D-frame sequence and flushing yields exactly D windows, window_indices(pos, D, G) for every position."""
    from hupr_amd.tools.stream import stream_window_sources
    windows, centers, per_push, flushed = _run(D, G)
    L = G // 2 - 1
    assert centers == list(range(D)) and len(windows) == D
    assert flushed == min(L, D) and per_push == [0] * min(L, D) + [1] * (D - min(L, D))
    for pos in range(D):
        assert windows[pos] == window_indices(pos, D, G), (D, G, pos)
    # the rule itself, with the whole sequence known
    for pos in range(D):
        assert stream_window_sources(pos, D - 1, G) == window_indices(pos, D, G)


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("D", (1, 3, 8, 20))
@pytest.mark.parametrize("seq", (1, 7))
def test_sequences_that_start_at_a_non_zero_index(D, G, seq):
    """A later sequence of a dataset: window_indices works on absolute item indices, the stream counts from its own start."""
    windows, _, _, _ = _run(D, G)
    first = seq * D
    for pos in range(D):
        assert [first + f for f in windows[pos]] == window_indices(first + pos, D, G), (D, G, seq, pos)


@pytest.mark.parametrize("G", GROUPS)
def test_zero_lookahead_answers_every_push(G):
    from hupr_amd.tools.stream import stream_window_sources
    windows, centers, per_push, flushed = _run(20, G, lookahead=0)
    assert per_push == [1] * 20 and flushed == 0 and centers == list(range(20))
    for c, w in enumerate(windows):
        assert w == stream_window_sources(c, c, G)
        assert w[G // 2:] == [c] * (G - G // 2)            # the upper half repeats the newest frame
        assert w[:G // 2] == [max(c - G // 2 + j, 0) for j in range(G // 2)]


@pytest.mark.parametrize("G", GROUPS)
def test_every_lookahead_emits_each_frame_once(G):
    for L in range(G // 2):
        windows, centers, per_push, flushed = _run(11, G, lookahead=L)
        assert centers == list(range(11)) and flushed == L and sum(per_push) == 11 - L
        for c, w in enumerate(windows):
            assert all(0 <= f <= 10 for f in w) and w[G // 2] == c
            # every source is still in a ring of the last G frames when it is read
            newest = min(c + L, 10)
            assert min(w) > newest - G


def test_lookahead_out_of_range_is_a_named_error():
    from hupr_amd.tools import stream as st
    for bad in (-1, 4, 100, 1.5, "2", True):
        with pytest.raises(st.LookaheadError):
            st.check_lookahead(bad, 8)
        with pytest.raises(st.LookaheadError):
            st.StreamSchedule(8, bad)
    with pytest.raises(st.LookaheadError):
        st.check_lookahead(1, 2)
    assert st.check_lookahead(None, 8) == 3 and st.check_lookahead(0, 8) == 0 and st.check_lookahead(3, 8) == 3
    assert issubclass(st.LookaheadError, st.StreamError) and issubclass(st.StreamError, ValueError)


def test_frame_shape_and_dtype_errors_are_named():
    from hupr_amd.tools import stream as st
    ok = torch.zeros((1, 4, 192, 256, 2), dtype=torch.int16)
    st.check_frames(ok, ok.clone(), 1)
    with pytest.raises(st.FrameShapeError):
        st.check_frames(ok, torch.zeros((2, 4, 192, 256, 2), dtype=torch.int16), 1)      # hori / vert mismatch
    with pytest.raises(st.FrameShapeError):
        st.check_frames(ok, ok, 2)                                                       # not the session's lanes
    with pytest.raises(st.FrameShapeError):
        st.check_frames(ok[0], ok[0], 1)
    with pytest.raises(st.FrameDtypeError):
        st.check_frames(ok.float(), ok.float(), 1)
    with pytest.raises(st.FrameDtypeError):
        st.check_frames(ok, ok.to(torch.int32), 1)
    with pytest.raises(st.FrameDtypeError):
        st.check_frames(ok.numpy(), ok.numpy(), 1)


def test_push_after_flush_needs_a_reset():
    from hupr_amd.tools import stream as st
    s = st.StreamSchedule(8)
    for _ in range(5):
        s.push()
    assert [c for c, _ in s.flush()] == [2, 3, 4]
    with pytest.raises(st.StreamEndedError):
        s.push()
    s.reset()
    assert s.frames_pushed == 0 and s.frames_emitted == 0 and s.push() is None


def test_stream_entry_points_check_their_arguments_on_the_host():
    """Null and shape errors come back through hupr_last_error() before any launch; an empty batch is a no-op."""
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    L = runtime.lib()
    assert L.hupr_stream_state_bytes() >= 8
    p = 4096                                               # any non-null address: every call below returns before it launches
    for fn in (L.hupr_mnet_stream_f32, L.hupr_mnet_stream_bf16act):
        assert fn(None, None, None, 3, 0, None, None, None, None, None, None, 0, 8, 4096, None) == 0        # lanes == 0
        assert fn(p, None, p, 3, 0, p, p, p, p, p, p, 1, 8, 4096, None) == -1 and b"null" in L.hupr_last_error()
        assert fn(None, p, p, 3, 0, p, p, p, p, p, p, 1, 8, 4096, None) == -1 and b"staging" in L.hupr_last_error()
        assert fn(p, p, p, 4, 0, p, p, p, p, p, p, 1, 8, 4096, None) == -1 and b"lookahead" in L.hupr_last_error()
        assert fn(p, p, p, -1, 0, p, p, p, p, p, p, 1, 8, 4096, None) == -1
        assert fn(p, p, p, 0, 0, p, p, p, p, p, p, 1, 7, 4096, None) == -1 and b"window" in L.hupr_last_error()
        assert fn(p, p, p, 0, 0, p, p, p, p, p, p, -1, 8, 4096, None) == -1
        assert fn(p, p, p, 0, 0, p, p, p, p, p, p, 1, 8, 0, None) == -1
    assert L.hupr_stream_reset(None, None) == -1 and b"null" in L.hupr_last_error()
    assert L.hupr_stream_advance(None, 0, 0, None) == -1
    assert L.hupr_stream_keypoints_f32(None, None, None, 0, 64, 4.0, None) == 0
    assert L.hupr_stream_keypoints_f32(None, p, p, 14, 64, 4.0, None) == -1


def test_stream_kernels_use_no_scratch():
    """The listing the build keeps for csrc/stream_window.hip: every kernel of the file with 0 spilled registers and 0 bytes of
    scratch, the window kernel in both stores within one wave's 256 registers (two waves per SIMD at least)."""
    meta = kernel_metadata("stream_window")
    for pat, count in (("hupr_k_mnet_stream", 2), ("hupr_k_stream_advance", 1), ("hupr_k_stream_reset", 1), ("hupr_k_stream_keypoints", 1)):
        assert len([n for n in meta if pat in n]) == count, (pat, sorted(meta))
    for n, m in meta.items():
        assert m["spill"] == 0 and m["sspill"] == 0 and m["scratch"] == 0, (n, m)
        assert m["vgpr"] <= 256 and m["lds"] <= 1024, (n, m)


def test_session_is_exported_and_refuses_a_cpu_model():
    from hupr_amd import tools
    from hupr_amd.config_tree import load_config
    from hupr_amd.runtime import HuprError
    assert tools.PoseStream is tools.stream.PoseStream and tools.stream_window_sources(3, 3, 8) == [0, 0, 1, 2, 3, 3, 3, 3]

    class _Cpu(torch.nn.Module):
        math_mode, numFilters = None, 32

        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

    with pytest.raises(HuprError):                      # no CPU fallback
        tools.PoseStream(_Cpu(), load_config())
    with pytest.raises(tools.LookaheadError):           # argument errors come first
        tools.PoseStream(_Cpu(), load_config(), lookahead=9)
