"""GPU (-m gpu): the live stream with ``decode="subpixel"`` and ``smooth=PoseSmoothing(10.0)`` — the one hupr_pose_decode_f32 launch
in place of arg-max + keypoints, eagerly, inside the captured graph and in the flush tail.  Synthetic weights and ADC frames as
tests/test_stream_gpu.py builds them; 12 frames with the default lookahead (3 silent pushes, 2 eager poses, 7 graph replays, 3
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
FIELDS = ("keypoints", "scores", "indices", "heatmap", "gcn_heatmap", "raw_keypoints", "velocity")


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

    def smoothing(self):
        from hupr_amd.tools import PoseSmoothing
        return PoseSmoothing(10.0)

    def session(self, new, lanes=1, graph=True):
        from hupr_amd.tools import PoseStream
        kw = dict(decode="subpixel", smooth=self.smoothing()) if new else {}
        return PoseStream(self.model, self.cfg, lanes=lanes, graph=graph, **kw)

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

    def run(self, new, lanes=1, graph=True):
        key = (new, lanes, graph)
        if key not in self.runs:
            s = self.session(new, lanes, graph)
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


def test_default_session_is_what_it_was(ctx):
    """No new argument: the two launches of before, raw_keypoints is keypoints, no velocity."""
    s, frames = ctx.run(False)
    assert not s._fused and s._fstate is None
    pf = s._frame(0, (frames[0].heatmap, frames[0].gcn_heatmap))
    assert pf.raw_keypoints is pf.keypoints and pf.velocity is None
    for pf in frames:
        assert pf.velocity is None and torch.equal(pf.raw_keypoints, pf.keypoints)
        assert torch.equal(pf.keypoints, torch.stack([pf.indices % 64, pf.indices // 64], dim=2).float() * ctx.ratio * (pf.scores > 0)[..., None])


def test_model_path_is_undisturbed(ctx):
    _, old = ctx.run(False)
    s, new = ctx.run(True)
    assert s._fused and s._fstate is not None
    for a, b in zip(new, old):
        _same(a, b, ("heatmap", "gcn_heatmap", "indices", "scores"), "subpixel + smoothing vs default")
        assert (a.raw_keypoints - b.keypoints).abs().max().item() <= 0.5 * ctx.ratio
    assert any(not torch.equal(a.raw_keypoints, b.keypoints) for a, b in zip(new, old))
    assert any(not torch.equal(a.raw_keypoints, a.keypoints) for a in new[1:])           # the filter does something
    assert torch.equal(new[0].raw_keypoints, new[0].keypoints)                           # its first sample is the raw one


@pytest.mark.parametrize("lanes", [1, 2])
def test_same_decode_as_offline(ctx, lanes):
    """functional.pose_decode on each emitted gcn_heatmap, with a filter state of its own, gives the session's keypoints."""
    from hupr_amd import functional as F_
    _, frames = ctx.run(True, lanes=lanes)
    state = F_.pose_filter_state(lanes * 14, "cuda")
    sm = ctx.smoothing()
    for pf in frames:
        idx, mx, raw, kp, vel = F_.pose_decode(pf.gcn_heatmap, ctx.ratio, refine=True, filter_state=state, smoothing=sm)
        assert raw.shape == (lanes, 1, 14, 2)
        assert torch.equal(idx.view(lanes, 14), pf.indices) and torch.equal(mx.view(lanes, 14), pf.scores), pf.frame
        assert torch.equal(raw.view(lanes, 14, 2), pf.raw_keypoints), pf.frame
        assert torch.equal(kp.view(lanes, 14, 2), pf.keypoints), pf.frame
        assert torch.equal(vel.view(lanes, 14, 2), pf.velocity), pf.frame
    assert any(pf.velocity.abs().max().item() > 0 for pf in frames)


@pytest.mark.parametrize("lanes", [1, 2])
def test_graph_equals_eager(ctx, lanes):
    _, graph = ctx.run(True, lanes=lanes, graph=True)
    _, eager = ctx.run(True, lanes=lanes, graph=False)
    for a, b in zip(graph, eager):
        _same(a, b, what="graph vs eager, lanes %d" % lanes)


def test_reset_clears_the_filter_state(ctx):
    s, first = ctx.run(True)
    assert s._fstate.any().item()
    with pytest.raises(ValueError):
        s.push(*ctx.frames(1, 0))                              # flush() ended the sequence
    s.reset()
    assert not s._fstate.any().item() and s.frames_pushed == 0
    second = ctx.play(s)
    for a, b in zip(second, first):
        _same(a, b, what="after reset")


def test_one_launch_fewer_than_the_default_decode(ctx):
    from hupr_amd import runtime as rt
    L = rt.lib()
    counts = {}
    for new in (False, True):
        s = ctx.session(new, graph=False)
        for n in range(6):
            s.push(*ctx.frames(1, n))
        c0 = L.hupr_launch_count()
        assert s.push(*ctx.frames(1, 6)) is not None
        counts[new] = L.hupr_launch_count() - c0
    torch.cuda.synchronize()
    print("launches of a steady eager push: default %d, subpixel + smoothing %d" % (counts[False], counts[True]))
    assert counts[True] == counts[False] - 1
