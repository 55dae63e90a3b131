"""GPU (-m gpu): the live stream with ``track=PoseTracking(10.0)`` — the one hupr_pose_track_f32 launch in place of arg-max +
keypoints, eagerly, inside the captured graph and in the flush tail.  Synthetic weights and ADC frames as
tests/test_stream_decode_gpu.py builds them; 12 frames with the default lookahead (3 silent pushes, 2 eager poses, 7 graph replays, 3
flushed poses).  Every comparison is torch.equal."""
import os

import numpy as np
import pytest
import torch

from hupr_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
N = 12
MODE = "bf16"
FIELDS = ("keypoints", "scores", "indices", "heatmap", "gcn_heatmap", "raw_keypoints", "velocity", "covariance", "forecast", "status")
RATE = 10.0


class _Ctx:
    def __init__(self):
        from hupr_amd.config_tree import load_config
        from hupr_amd.tools.engine import TrainEngine
        g = np.load(os.path.join(GOLD, "model_eval.npz"))
        self.cfg = load_config()
        self.engine = TrainEngine(self.cfg, device="cuda")
        self.model = self.engine.model
        self.model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.hupr_state(int(g["model_seed"]), gain=float(g["gain"])).items()})
        self.model.eval()
        self.model.math_mode = MODE
        self.ratio = self.cfg.DATASET.imgSize / self.cfg.DATASET.heatmapSize
        # dev[seq][sensor]: (N, 4, 192, 256, 2) int16
        self.dev = [[torch.from_numpy(np.concatenate([synth.adc_cube_int16(5, seq=q, frame=f, sensor=s) for f in range(N)])).cuda()
                     for s in range(2)] for q in range(2)]
        self.runs = {}

    def tracking(self, **kw):
        from hupr_amd.tools import PoseTracking
        return PoseTracking(RATE, **kw)

    def session(self, kind, lanes=1, graph=True, **kw):
        """kind: "default", "subpixel" (no filter) or "track" (subpixel + tracker)."""
        from hupr_amd.tools import PoseStream
        args = dict(default={}, subpixel=dict(decode="subpixel"), track=dict(decode="subpixel", track=self.tracking()))[kind]
        return PoseStream(self.model, self.cfg, lanes=lanes, graph=graph, **dict(args, **kw))

    def frames(self, lanes, n):
        return (torch.stack([self.dev[q][0][n] for q in range(lanes)]), torch.stack([self.dev[q][1][n] for q in range(lanes)]))

    def play(self, s):
        """Push the N frames, flush -> the N emitted PoseFrames, cloned, in order."""
        out = []
        for n in range(N):
            pf = s.push(*self.frames(s.lanes, n))
            assert (pf is None) == (n < s.lookahead)
            if pf is not None:
                out.append(pf.clone())
        out.extend(s.flush())
        assert [p.frame for p in out] == list(range(N))
        return out

    def run(self, kind, lanes=1, graph=True, **kw):
        key = (kind, lanes, graph) + tuple(sorted(kw.items()))
        if key not in self.runs:
            s = self.session(kind, lanes, graph, **kw)
            self.runs[key] = (s, self.play(s))
            assert bool(s._graphs) == graph
        return self.runs[key]


@pytest.fixture(scope="module")
def ctx():
    c = _Ctx()
    yield c
    c.engine.close()


def _same(a, b, fields=FIELDS, what=None):
    for k in fields:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), (what, a.frame, k)
        if x is not None:
            assert torch.equal(x, y), (what, a.frame, k)


def _offline(ctx, frames, lanes, p):
    """functional.pose_track over the emitted gcn_heatmaps with a state of its own -> [(idx, maxval, raw, kp, vel, cov, fc, status)]."""
    from hupr_amd import functional as F_
    state = F_.pose_track_state(lanes * 14, "cuda")
    return [F_.pose_track(pf.gcn_heatmap, ctx.ratio, refine=True, track_state=state, tracking=p) for pf in frames]


def test_a_tracking_session_emits_tracked_frames_on_an_undisturbed_model_path(ctx):
    from hupr_amd.tools import PoseFrame, TrackedPoseFrame
    _, old = ctx.run("default")
    _, sub = ctx.run("subpixel")
    s, new = ctx.run("track")
    assert s._tstate is not None and s._fstate is None and s.track.horizon_s == 0.0
    assert all(type(pf) is PoseFrame for pf in old + sub) and all(type(pf) is TrackedPoseFrame for pf in new)
    for a, b, c in zip(new, old, sub):
        _same(a, b, ("heatmap", "gcn_heatmap", "indices", "scores"), "tracking vs default")
        _same(a, c, ("raw_keypoints",), "tracking vs subpixel without a filter")
        assert a.covariance.shape == (1, 14, 3) and a.forecast.shape == (1, 14, 2) and a.status.shape == (1, 14)
        assert a.status.dtype == torch.int32 and torch.equal(a.forecast, a.keypoints)        # horizon 0
    seen = new[0].scores > 0
    assert seen.any().item()
    assert torch.equal(new[0].status, torch.where(seen, 3, 4).to(torch.int32))             # STARTED / LOST
    assert torch.equal(new[0].keypoints, new[0].raw_keypoints) and not new[0].velocity.any().item()
    assert any((pf.status == 0).any().item() for pf in new[1:])                             # UPDATED: the filter runs
    assert any(not torch.equal(pf.keypoints, pf.raw_keypoints) for pf in new[1:])


@pytest.mark.parametrize("lanes", [1, 2])
def test_same_tracker_as_offline(ctx, lanes):
    s, frames = ctx.run("track", lanes=lanes)
    for pf, (idx, mx, raw, kp, vel, cov, fc, status) in zip(frames, _offline(ctx, frames, lanes, s.track)):
        assert raw.shape == (lanes, 1, 14, 2) and cov.shape == (lanes, 1, 14, 3) and status.shape == (lanes, 1, 14)
        assert torch.equal(idx.view(lanes, 14), pf.indices) and torch.equal(mx.view(lanes, 14), pf.scores), pf.frame
        assert torch.equal(raw.view(lanes, 14, 2), pf.raw_keypoints), pf.frame
        assert torch.equal(kp.view(lanes, 14, 2), pf.keypoints), pf.frame
        assert torch.equal(vel.view(lanes, 14, 2), pf.velocity), pf.frame
        assert torch.equal(cov.view(lanes, 14, 3), pf.covariance), pf.frame
        assert torch.equal(fc.view(lanes, 14, 2), pf.forecast), pf.frame
        assert torch.equal(status.view(lanes, 14), pf.status), pf.frame
    assert any(pf.velocity.abs().max().item() > 0 for pf in frames)


@pytest.mark.parametrize("lanes", [1, 2])
def test_graph_equals_eager(ctx, lanes):
    _, graph = ctx.run("track", lanes=lanes, graph=True)
    _, eager = ctx.run("track", lanes=lanes, graph=False)
    for a, b in zip(graph, eager):
        _same(a, b, what="graph vs eager, lanes %d" % lanes)


def test_predict_now_forecasts_to_the_newest_frame(ctx):
    _, plain = ctx.run("track")
    s, frames = ctx.run("track", predict_now=True)
    assert s.lookahead == 3 and s.track.horizon_s == 3 / RATE
    p = ctx.tracking(horizon_s=3 / RATE)
    for pf, base, off in zip(frames, plain, _offline(ctx, frames, 1, p)):
        _same(pf, base, tuple(k for k in FIELDS if k != "forecast"), "predict_now touches the forecast only")
        assert torch.equal(off[6].view(1, 14, 2), pf.forecast), pf.frame
    assert any(not torch.equal(pf.forecast, pf.keypoints) for pf in frames)
    # the session's horizon overrides the tracker's own
    s = ctx.session("track", track=ctx.tracking(horizon_s=5.0), predict_now=True)
    assert s.track.horizon_s == 3 / RATE
    # no lookahead, nothing to forecast
    s, frames = ctx.run("track", lookahead=0, predict_now=True)
    assert s.lookahead == 0 and s.track.horizon_s == 0.0
    for pf in frames:
        assert torch.equal(pf.forecast, pf.keypoints), pf.frame


def test_reset_clears_the_tracker_state(ctx):
    s, first = ctx.run("track")
    assert s._tstate.any().item()
    with pytest.raises(ValueError):
        s.push(*ctx.frames(1, 0))                              # flush() ended the sequence
    s.reset()
    assert not s._tstate.any().item() and s.frames_pushed == 0
    second = ctx.play(s)
    for a, b in zip(second, first):
        _same(a, b, what="after reset")


def test_one_launch_fewer_than_the_default_decode(ctx):
    from hupr_amd import runtime as rt
    L = rt.lib()
    counts = {}
    for kind in ("default", "track"):
        s = ctx.session(kind, graph=False)
        for n in range(6):
            s.push(*ctx.frames(1, n))
        c0 = L.hupr_launch_count()
        assert s.push(*ctx.frames(1, 6)) is not None
        counts[kind] = L.hupr_launch_count() - c0
    torch.cuda.synchronize()
    print("launches of a steady eager push: default %d, tracking %d" % (counts["default"], counts["track"]))
    assert counts["track"] == counts["default"] - 1
