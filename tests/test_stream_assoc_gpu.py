"""GPU (-m gpu): the live stream with ``track=PoseTracking(10.0, candidates=2)`` and with ``gate_on_presence`` — the one
hupr_pose_track_assoc_f32 launch in the tracker's place, eagerly, inside the captured graph and in the flush tail.  Synthetic weights
and ADC frames as tests/test_stream_track_gpu.py builds them: 12 frames with the default lookahead (3 silent pushes, 2 eager poses, 7
graph replays, 3 flushed poses).  Every comparison is torch.equal."""
import os

import numpy as np
import pytest
import torch

from hupr_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
N = 12
MODE = "bf16"
RATE = 10.0
TRACKED = ("keypoints", "scores", "indices", "raw_keypoints", "velocity", "covariance", "forecast", "status")
CANDIDATE = ("candidates", "candidate_scores", "candidate_count", "chosen")
UPDATED, COASTED_MISSING, COASTED_GATED, STARTED, LOST = range(5)


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
        # dev[sensor]: (N, 4, 192, 256, 2) int16
        self.dev = [torch.from_numpy(np.concatenate([synth.adc_cube_int16(5, seq=0, frame=f, sensor=s) for f in range(N)])).cuda()
                    for s in range(2)]

    def session(self, track, **kw):
        from hupr_amd.tools import PoseStream
        return PoseStream(self.model, self.cfg, decode="subpixel", track=track, **kw)

    def play(self, s, frames=None):
        out = []
        for n in range(N):
            hori, vert = (self.dev[0][n:n + 1], self.dev[1][n:n + 1]) if frames is None else frames(n)
            pf = s.push(hori, vert)
            assert (pf is None) == (n < s.lookahead)
            if pf is not None:
                out.append(pf.clone())
        out.extend(s.flush())
        assert [p.frame for p in out] == list(range(N))
        return out


@pytest.fixture(scope="module")
def ctx():
    c = _Ctx()
    yield c
    c.engine.close()


def _offline(ctx, frames, p, present=None):
    """functional.pose_track over the emitted gcn_heatmaps with a state of its own -> its tuples, one per frame."""
    from hupr_amd import functional as F_
    state = F_.pose_track_state(14, "cuda")
    return [F_.pose_track(pf.gcn_heatmap, ctx.ratio, refine=True, track_state=state, tracking=p,
                          present=None if present is None else pf.present.view(1, 1)) for pf in frames]


def _equal_offline(pf, out):
    idx, mx, raw, kp, vel, cov, fc, status, cxy, cscore, ccount, chosen = out
    want = dict(indices=idx, scores=mx, raw_keypoints=raw, keypoints=kp, velocity=vel, covariance=cov, forecast=fc, status=status,
                candidates=cxy, candidate_scores=cscore, candidate_count=ccount, chosen=chosen)
    for k in TRACKED + CANDIDATE:
        got = getattr(pf, k)
        assert got.dtype == want[k].dtype and torch.equal(got, want[k].view(got.shape)), (pf.frame, k)


def test_a_session_with_two_candidates_is_the_eager_tracker_on_its_own_maps(ctx):
    from hupr_amd.tools import PoseTracking, TrackedPoseFrame
    p = PoseTracking(RATE, candidates=2)
    s = ctx.session(p, history=True)
    frames = ctx.play(s)
    assert s._graphs and s.track.associates
    for pf, out in zip(frames, _offline(ctx, frames, p)):
        assert type(pf) is TrackedPoseFrame
        assert pf.candidates.shape == (1, 14, 2, 2) and pf.candidate_scores.shape == (1, 14, 2)
        assert pf.candidate_count.shape == (1, 14) and pf.chosen.shape == (1, 14) and pf.chosen.dtype == torch.int32
        _equal_offline(pf, out)
        assert torch.equal(pf.candidates[:, :, 0], pf.raw_keypoints) and torch.equal(pf.candidate_scores[:, :, 0], pf.scores)
    assert any((pf.status == UPDATED).any().item() for pf in frames[1:])
    # the recorded states are the tracker's layout: smoothed() runs on them as it does on the plain tracker's
    seq = s.smoothed()
    assert len(seq) == N and seq.keypoints.shape == (N, 1, 14, 2) and torch.isfinite(seq.keypoints).all().item()
    # the plain tracker's session decodes the same maps: candidate 0 is its measurement
    plain = ctx.play(ctx.session(PoseTracking(RATE)))
    for a, b in zip(frames, plain):
        assert torch.equal(a.raw_keypoints, b.raw_keypoints) and torch.equal(a.scores, b.scores) and torch.equal(a.indices, b.indices)
        assert b.candidates is None and b.candidate_scores is None and b.candidate_count is None and b.chosen is None


def test_the_route_follows_the_settings(ctx, monkeypatch):
    """candidates = 1 without coupling launches hupr_pose_track_f32, as before; anything else the associating entry — one launch
    either way, so an eager steady push counts the same launches."""
    from hupr_amd import runtime as rt
    from hupr_amd.tools import PoseTracking, PresenceGate
    L = rt.lib()
    calls = {"hupr_pose_track_f32": 0, "hupr_pose_track_assoc_f32": 0}

    def counted(name):
        fn = getattr(L, name)

        def call(*args):
            calls[name] += 1
            return fn(*args)
        return call

    for name in calls:
        monkeypatch.setattr(L, name, counted(name))
    launches = {}
    for kind, kw in (("plain", dict(track=PoseTracking(RATE))), ("two", dict(track=PoseTracking(RATE, candidates=2))),
                     ("coupled", dict(track=PoseTracking(RATE, gate_on_presence=True), presence=PresenceGate()))):
        s = ctx.session(kw.pop("track"), graph=False, **kw)
        for n in range(6):
            s.push(ctx.dev[0][n:n + 1], ctx.dev[1][n:n + 1])
        before, c0 = dict(calls), L.hupr_launch_count()
        assert s.push(ctx.dev[0][6:7], ctx.dev[1][6:7]) is not None
        launches[kind] = L.hupr_launch_count() - c0
        delta = {k: calls[k] - before[k] for k in calls}
        assert delta == ({"hupr_pose_track_f32": 1, "hupr_pose_track_assoc_f32": 0} if kind == "plain"
                         else {"hupr_pose_track_f32": 0, "hupr_pose_track_assoc_f32": 1}), (kind, delta)
    torch.cuda.synchronize()
    print("launches of a steady eager push: %s" % launches)
    assert launches["two"] == launches["plain"] and launches["coupled"] == launches["plain"] + 2     # the detector and the gate


def test_an_empty_scene_takes_the_measurement_away(ctx):
    """Frames 0..4 hold a point target, the gate (confirm 1, hold 0) calls the lane present and tracks start; then the ADC is all zero:
    the gate calls it empty at once, every track updated in frame 4 coasts MISSING for max_coast = 2 frames on its own velocity and
    then reports LOST (one that was coasting already, sooner), whatever the heat-maps show.  Lookahead 0: two eager pushes, then replays.
    """
    from hupr_amd.tools import PoseTracking, PresenceGate
    target = dict(range_bin=60.0, az_bin=-9.0, el_bin=0.0, amp=15.0)
    doppler = (-3, -2, -1, 1, 2, 3)
    live_frames = 5
    cubes = [[torch.from_numpy(synth.point_target_cube([dict(target, doppler_bin=float(doppler[f % 6]))], noise=300.0, seed=10 * f + s)).cuda()
              for s in range(2)] for f in range(live_frames)]
    zero = torch.zeros_like(cubes[0][0])
    p = PoseTracking(RATE, max_coast=2, gate_on_presence=True)
    s = ctx.session(p, lookahead=0, presence=PresenceGate(min_cells=3, confirm=1, hold=0))
    frames = ctx.play(s, lambda n: tuple(cubes[n]) if n < live_frames else (zero, zero))
    assert s._graphs
    present = [int(pf.present[0]) for pf in frames]
    assert present == [1] * live_frames + [0] * (N - live_frames), present
    for pf, out in zip(frames, _offline(ctx, frames, p, present=True)):           # the flag of the emitted frame, replayed or flushed
        _equal_offline(pf, out)
    last = frames[live_frames - 1]
    fresh = (last.status == UPDATED) | (last.status == STARTED)                  # coast 0; a track that coasted already ends sooner
    assert fresh.any().item()
    for k in range(2):
        pf = frames[live_frames + k]
        assert (pf.status[fresh] == COASTED_MISSING).all().item(), k
        assert ((pf.status == COASTED_MISSING) | (pf.status == LOST)).all().item() and (pf.chosen == -1).all().item()
        going = pf.status == COASTED_MISSING
        assert torch.equal(pf.velocity[going], last.velocity[going]), k          # on the track's own velocity
    for pf in frames[live_frames + 2:]:
        assert (pf.status == LOST).all().item() and not pf.velocity.any().item() and torch.equal(pf.keypoints, pf.raw_keypoints)
    assert not s._tstate.any().item()
