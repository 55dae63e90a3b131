"""GPU (-m gpu): the live stream with ``track=PoseTracking(10.0, pair_swap=True)`` — the one hupr_pose_track_pairs_f32 launch in the
tracker's place, eagerly, inside the captured graph and in the flush tail.  Synthetic weights and ADC frames as
tests/test_stream_assoc_gpu.py builds them: 12 frames with the default lookahead (3 silent pushes, 2 eager poses, 7 graph replays, 3
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
RATE = 10.0
FIELDS = ("indices", "scores", "raw_keypoints", "keypoints", "velocity", "covariance", "forecast", "status", "candidates",
          "candidate_scores", "candidate_count", "chosen", "source")           # in the order of functional.pose_track's 13-tuple
PARTNER = (3, 4, 5, 0, 1, 2, 6, 7, 11, 12, 13, 8, 9, 10)


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
        self.dev = [torch.from_numpy(np.concatenate([synth.adc_cube_int16(5, seq=0, frame=f, sensor=s) for f in range(N)])).cuda()
                    for s in range(2)]

    def play(self, track, **kw):
        from hupr_amd.tools import PoseStream
        s = PoseStream(self.model, self.cfg, decode="subpixel", track=track, **kw)
        out = []
        for n in range(N):
            pf = s.push(self.dev[0][n:n + 1], self.dev[1][n:n + 1])
            assert (pf is None) == (n < s.lookahead)
            if pf is not None:
                out.append(pf.clone())
        out.extend(s.flush())
        assert [p.frame for p in out] == list(range(N))
        return s, out


@pytest.fixture(scope="module")
def ctx():
    c = _Ctx()
    yield c
    c.engine.close()


@pytest.mark.parametrize("graph", (False, True), ids=["eager", "graph"])
def test_a_session_with_pair_swap_is_the_eager_tracker_on_its_own_maps(ctx, graph):
    from hupr_amd import functional as F_
    from hupr_amd.tools import PairedPoseFrame, PoseTracking, TrackedPoseFrame
    p = PoseTracking(RATE, pair_swap=True, candidates=2)
    s, frames = ctx.play(p, graph=graph, history=True)
    assert bool(s._graphs) == graph and s.track.associates and s.track.pairs == PARTNER
    state = F_.pose_track_state(14, "cuda")
    for pf in frames:
        assert type(pf) is PairedPoseFrame and pf.source.shape == (1, 14) and pf.source.dtype == torch.int32
        out = F_.pose_track(pf.gcn_heatmap, ctx.ratio, refine=True, track_state=state, tracking=s.track)
        assert len(out) == 13
        for k, want in zip(FIELDS, out):
            got = getattr(pf, k)
            assert got.dtype == want.dtype and torch.equal(got, want.view(got.shape)), (pf.frame, k)
        assert ((pf.source >= 0) == (pf.chosen >= 0)).all().item()
    assert torch.equal(s._tstate, state)
    assert any((pf.source >= 0).any().item() for pf in frames)
    seq = s.smoothed()                                                           # the state layout is the tracker's: smoothed() runs on it
    assert len(seq) == N and torch.isfinite(seq.keypoints).all().item()
    # heat-maps, scores and arg-max are those of a session without the option
    _, plain = ctx.play(PoseTracking(RATE), graph=graph)
    for a, b in zip(frames, plain):
        assert torch.equal(a.gcn_heatmap, b.gcn_heatmap) and torch.equal(a.heatmap, b.heatmap)
        assert torch.equal(a.raw_keypoints, b.raw_keypoints) and torch.equal(a.scores, b.scores) and torch.equal(a.indices, b.indices)
        assert type(b) is TrackedPoseFrame and b.source is None and b.chosen is None
