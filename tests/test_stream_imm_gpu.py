"""GPU (-m gpu): the live stream with ``track=PoseTracking(10.0, accel_psd_moving=...)`` — the one hupr_pose_track_imm_f32 launch in
the plain tracker's place, eagerly, inside the captured graph and in the flush tail.  Synthetic weights and ADC frames as
tests/test_stream_track_gpu.py builds them; 12 frames with the default lookahead (3 silent pushes, 2 eager poses, 7 graph replays, 3
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
MODELS = dict(accel_psd=5.0, accel_psd_moving=5000.0, switch_prob=0.1, moving_prior=0.25)


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
        """kind: "track" (subpixel + the plain tracker) or "imm" (subpixel + the two-model tracker)."""
        from hupr_amd.tools import PoseStream
        args = dict(track=dict(decode="subpixel", track=self.tracking()), imm=dict(decode="subpixel", track=self.tracking(**MODELS)))[kind]
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


def test_a_two_model_session_emits_the_new_frames_on_an_undisturbed_model_path(ctx):
    from hupr_amd.tools import ManeuveringPoseFrame, TrackedPoseFrame
    _, old = ctx.run("track")
    s, new = ctx.run("imm")
    assert s._tstate.shape == (14, 32) and s._fstate is None and s._cxy is None and s._source is None
    assert all(type(pf) is TrackedPoseFrame for pf in old) and all(type(pf) is ManeuveringPoseFrame for pf in new)
    for a, b in zip(new, old):
        _same(a, b, ("heatmap", "gcn_heatmap", "indices", "scores", "raw_keypoints"), "two models vs the plain tracker")
        assert a.moving.shape == (1, 14) and a.moving.dtype == torch.float32 and a.chosen is None and a.lagged is None
        assert a.covariance.shape == (1, 14, 3) and torch.equal(a.forecast, a.keypoints)     # horizon 0
        assert ((a.moving >= 0) & (a.moving <= 1)).all().item()
        assert not a.moving[a.status == 4].any().item()                                      # 0 where there is no live track
    seen = new[0].scores > 0
    assert seen.any().item()
    assert torch.equal(new[0].status, torch.where(seen, 3, 4).to(torch.int32))             # STARTED / LOST
    assert torch.equal(new[0].moving, torch.where(seen, 0.25, 0.0).to(torch.float32))
    assert torch.equal(new[0].keypoints, new[0].raw_keypoints) and not new[0].velocity.any().item()
    assert any((pf.status == 0).any().item() for pf in new[1:])                             # UPDATED: the filters run
    assert any(not torch.equal(pf.keypoints, pf.raw_keypoints) for pf in new[1:])
    assert any(not torch.equal(a.keypoints, b.keypoints) for a, b in zip(new[1:], old[1:]))  # and they are not the plain one
    assert any(not torch.equal(a.moving, b.moving) for a, b in zip(new[1:], new[2:]))


@pytest.mark.parametrize("lanes", [1, 2])
def test_same_tracker_as_offline(ctx, lanes):
    from hupr_amd import functional as F_
    s, frames = ctx.run("imm", lanes=lanes)
    state = F_.pose_imm_state(lanes * 14, "cuda")
    for pf in frames:
        idx, mx, raw, kp, vel, cov, fc, status, moving = F_.pose_track(pf.gcn_heatmap, ctx.ratio, refine=True, track_state=state,
                                                                       tracking=s.track)
        assert raw.shape == (lanes, 1, 14, 2) and moving.shape == (lanes, 1, 14)
        assert torch.equal(idx.view(lanes, 14), pf.indices) and torch.equal(mx.view(lanes, 14), pf.scores), pf.frame
        assert torch.equal(raw.view(lanes, 14, 2), pf.raw_keypoints), pf.frame
        assert torch.equal(kp.view(lanes, 14, 2), pf.keypoints), pf.frame
        assert torch.equal(vel.view(lanes, 14, 2), pf.velocity), pf.frame
        assert torch.equal(cov.view(lanes, 14, 3), pf.covariance), pf.frame
        assert torch.equal(fc.view(lanes, 14, 2), pf.forecast), pf.frame
        assert torch.equal(status.view(lanes, 14), pf.status), pf.frame
        assert torch.equal(moving.view(lanes, 14), pf.moving), pf.frame
    assert any(pf.velocity.abs().max().item() > 0 for pf in frames)


@pytest.mark.parametrize("lanes", [1, 2])
def test_graph_equals_eager(ctx, lanes):
    _, graph = ctx.run("imm", lanes=lanes, graph=True)
    _, eager = ctx.run("imm", lanes=lanes, graph=False)
    for a, b in zip(graph, eager):
        _same(a, b, FIELDS + ("moving",), what="graph vs eager, lanes %d" % lanes)


def test_reset_clears_the_two_model_state(ctx):
    s, first = ctx.run("imm")
    assert s._tstate.any().item()
    with pytest.raises(ValueError):
        s.push(*ctx.frames(1, 0))                              # flush() ended the sequence
    s.reset()
    assert not s._tstate.any().item() and s.frames_pushed == 0
    second = ctx.play(s)
    for a, b in zip(second, first):
        _same(a, b, FIELDS + ("moving",), what="after reset")


def test_as_many_launches_as_the_plain_tracking_session(ctx):
    from hupr_amd import runtime as rt
    L = rt.lib()
    counts = {}
    for kind in ("track", "imm"):
        s = ctx.session(kind, graph=False)
        for n in range(6):
            s.push(*ctx.frames(1, n))
        c0 = L.hupr_launch_count()
        assert s.push(*ctx.frames(1, 6)) is not None
        counts[kind] = L.hupr_launch_count() - c0
    torch.cuda.synchronize()
    print("launches of a steady eager push: plain tracker %d, two models %d" % (counts["track"], counts["imm"]))
    assert counts["imm"] == counts["track"]


def test_the_smoothers_are_refused_and_the_measurement_record_is_not(ctx):
    from hupr_amd.tools import TrackingError
    with pytest.raises(TrackingError):
        ctx.session("imm", lag=4)
    with pytest.raises(TrackingError):
        ctx.session("imm", history=True)
    s = ctx.session("imm", graph=False)
    with pytest.raises(TrackingError):
        s.smoothed()
    with pytest.raises(TrackingError):
        s.lag_tail()
    # measurements=True composes: the record fills, the poses are those of a session without it, and the fit keeps both PSDs
    _, base = ctx.run("imm")
    s, frames = ctx.run("imm", measurements=True)
    for a, b in zip(frames, base):
        _same(a, b, FIELDS + ("moving",), what="with measurements")
    assert len(s.measurements) == N
    fit = s.fit_tracking(rounds=1)
    assert (fit.tracking.accel_psd, fit.tracking.accel_psd_moving, fit.tracking.switch_prob) == (5.0, 5000.0, 0.1)


def test_a_session_without_the_second_model_is_the_plain_tracking_session(ctx):
    """``accel_psd_moving=None`` beside changed ``switch_prob`` / ``moving_prior``: today's launch, today's frames, bit for bit."""
    from hupr_amd.tools import TrackedPoseFrame
    _, base = ctx.run("track")
    s = ctx.session("track", track=ctx.tracking(switch_prob=0.2, moving_prior=0.9))
    assert s._tstate.shape == (14, 16) and s._moving is None
    frames = ctx.play(s)
    for a, b in zip(frames, base):
        assert type(a) is TrackedPoseFrame
        _same(a, b, what="switch_prob and moving_prior without accel_psd_moving")
