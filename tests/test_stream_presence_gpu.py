"""GPU (-m gpu): the live stream with ``presence=PresenceGate(...)`` — the CA-CFAR launch on the centre frame's ring planes and the
gate launch behind it, eagerly (the first two emitting pushes), inside the captured graph and in the flush tail.  Synthetic weights as
tests/test_stream_track_gpu.py builds them; 12 frames per lane: noise, then a point target that moves through the Doppler slots, then
noise again.  Every comparison is torch.equal."""
import os

import numpy as np
import pytest
import torch

import cfar_ref as ref
from hupr_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
N = 12
MODE = "bf16"
OLD_FIELDS = ("keypoints", "scores", "indices", "heatmap", "gcn_heatmap", "raw_keypoints", "velocity")
TARGET_FRAMES = (range(3, 8), range(1, 5))           # per lane: the frames that hold the mover
GATE = dict(min_cells=3, confirm=2, hold=2)
DOPPLER = (-3, -2, -1, 1, 2, 3)


def _frame(lane, f, sensor):
    if f in TARGET_FRAMES[lane]:
        t = dict(range_bin=60.0 - 2 * lane, az_bin=-9.0 + 5 * lane, el_bin=0.0, amp=15.0, doppler_bin=float(DOPPLER[(f + lane) % 6]))
        return synth.point_target_cube([t], noise=300.0, seed=100 * lane + 10 * f + sensor)
    return synth.adc_cube_int16(9, seq=lane, frame=f, sensor=sensor)


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
        # dev[lane][sensor]: (N, 4, 192, 256, 2) int16
        self.dev = [[torch.from_numpy(np.concatenate([_frame(q, f, s) for f in range(N)])).cuda() for s in range(2)] for q in range(2)]
        self.runs = {}
        self._offline = {}

    def gate(self, **kw):
        from hupr_amd.tools import PresenceGate
        return PresenceGate(**dict(GATE, **kw))

    def frames(self, lanes, n):
        return (torch.stack([self.dev[q][0][n] for q in range(lanes)]), torch.stack([self.dev[q][1][n] for q in range(lanes)]))

    def play(self, s):
        out = []
        for n in range(N):
            pf = s.push(*self.frames(s.lanes, n))
            assert (pf is None) == (n < s.lookahead)
            if pf is not None:
                out.append(pf.clone())
        out.extend(s.flush())
        assert [p.frame for p in out] == list(range(N))
        return out

    def run(self, lanes, lookahead, graph=True, presence=True, **kw):
        from hupr_amd.tools import PoseStream
        key = (lanes, lookahead, graph, presence) + tuple(sorted(kw))
        if key not in self.runs:
            s = PoseStream(self.model, self.cfg, lanes=lanes, lookahead=lookahead, graph=graph, presence=self.gate() if presence else None, **kw)
            self.runs[key] = (s, self.play(s))
            assert bool(s._graphs) == graph
        return self.runs[key]

    def offline(self, lane):
        """functional.cfar_ra on the lane's N horizontal frames through the offline chain -> (N, 8) summary."""
        from hupr_amd import functional as F_, preprocessing
        if lane not in self._offline:
            g = self.gate()
            planes = preprocessing.fft_chain_loader_means(self.dev[lane][0])
            self._offline[lane] = F_.cfar_ra(planes, g.pfa, g.guard, g.train, want_mask=False).summary
        return self._offline[lane]


@pytest.fixture(scope="module")
def ctx():
    c = _Ctx()
    yield c
    c.engine.close()


def _want_present(ctx, lane):
    counts = ctx.offline(lane)[:, 0].cpu().numpy()
    return ref.ref_gate(counts, GATE["min_cells"], GATE["confirm"], GATE["hold"])[0]


def test_the_sequence_is_what_the_test_needs(ctx):
    """The offline detector sees the mover in exactly the target frames, in the slot of its Doppler bin, and the reference gate rises
    and falls inside the sequence."""
    for lane in range(2):
        occ = ctx.offline(lane).cpu().numpy()
        hit = occ[:, 0] >= GATE["min_cells"]
        assert hit.tolist() == [f in TARGET_FRAMES[lane] for f in range(N)]
        for f in TARGET_FRAMES[lane]:
            assert occ[f, 2] == DOPPLER[(f + lane) % 6] + 4 and np.sign(occ[f, 7]) == np.sign(DOPPLER[(f + lane) % 6])
        first, last = TARGET_FRAMES[lane][0], TARGET_FRAMES[lane][-1]
        want = [int(first + GATE["confirm"] - 1 <= f <= last + GATE["hold"]) for f in range(N)]
        assert _want_present(ctx, lane).tolist() == want and want[-1] == 0


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("lookahead", [0, 3])
def test_occupancy_is_the_offline_detector_and_present_follows_the_gate(ctx, lanes, lookahead):
    s, frames = ctx.run(lanes, lookahead)
    assert s._graphs and s._gstate is not None
    for pf in frames:
        assert pf.occupancy.shape == (lanes, 8) and pf.occupancy.dtype == torch.float32
        assert pf.present.shape == (lanes,) and pf.present.dtype == torch.int32
        for lane in range(lanes):
            assert torch.equal(pf.occupancy[lane], ctx.offline(lane)[pf.frame]), (pf.frame, lane)
    for lane in range(lanes):
        assert [int(pf.present[lane]) for pf in frames] == _want_present(ctx, lane).tolist()
    assert s._gstate.cpu()[:, 3].tolist() == [N] * lanes


def test_eager_pushes_give_the_bits_of_the_replay(ctx):
    _, replay = ctx.run(1, 3)
    s, eager = ctx.run(1, 3, graph=False)
    assert not s._graphs
    for a, b in zip(eager, replay):
        assert torch.equal(a.occupancy, b.occupancy) and torch.equal(a.present, b.present)


def test_reset_clears_the_gate(ctx):
    s, frames = ctx.run(2, 0)
    s.reset()
    assert not s._gstate.any().item()
    again = ctx.play(s)
    for a, b in zip(again, frames):
        assert torch.equal(a.occupancy, b.occupancy) and torch.equal(a.present, b.present)
    # without the reset the gate would have gone on from its last state: one hit then confirms at once
    assert [int(pf.present[0]) for pf in again] == _want_present(ctx, 0).tolist()


def test_the_gate_reports_only(ctx):
    """A session without ``presence`` emits the same bits in every field it always had, and None in the two new ones."""
    _, with_gate = ctx.run(1, 3)
    s, without = ctx.run(1, 3, presence=False)
    assert s._gstate is None and s._occ is None
    for a, b in zip(with_gate, without):
        assert b.present is None and b.occupancy is None and a.present is not None
        for k in OLD_FIELDS:
            x, y = getattr(a, k), getattr(b, k)
            assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), (a.frame, k)


def test_presence_composes_with_the_tracker_and_its_history(ctx):
    from hupr_amd.tools import PoseTracking, TrackedPoseFrame
    from hupr_amd.tools import PoseStream
    s = PoseStream(ctx.model, ctx.cfg, lanes=1, lookahead=3, presence=ctx.gate(), decode="subpixel", track=PoseTracking(10.0),
                   history=True, tdm_compensation=False)
    frames = ctx.play(s)
    _, plain = ctx.run(1, 3)
    assert all(type(pf) is TrackedPoseFrame for pf in frames) and len(s.smoothed()) == N
    for a, b in zip(frames, plain):
        assert torch.equal(a.occupancy, b.occupancy) and torch.equal(a.present, b.present) and a.covariance is not None
        assert torch.equal(a.cpu().present, b.present.cpu())


def test_stream_command_adds_the_two_keys_and_nothing_else(ctx, tmp_path, monkeypatch):
    """python -m hupr_amd.tools.stream --presence on a tiny raw capture: every record gains present and occupancy, the detector's
    summary of that frame; the other keys are those of a run without the flag, value for value."""
    import json
    from hupr_amd import functional as F_, preprocessing
    from hupr_amd.tools import stream as st
    root = synth.write_tiny_dataset(str(tmp_path / "tinyraw"), cubes=False, raw=True, phases=("val",))
    seq = synth.TINY["valName"][0]
    os.makedirs(tmp_path / "logs" / "streamtest")
    torch.save({"epoch": 3, "model_state_dict": ctx.model.state_dict(), "optimizer_state_dict": {}, "accuracy": 0.0},
               str(tmp_path / "logs" / "streamtest" / "model_best.pth"))
    monkeypatch.chdir(tmp_path)
    raw = os.path.join(root, "single_%d" % seq)
    common = ["--dir", "streamtest", "--raw", raw, "--math", MODE]
    plain = st.main(common + ["--out", str(tmp_path / "plain.json")])
    gated = st.main(common + ["--out", str(tmp_path / "gated.json"), "--presence", "--pfa", "1e-3", "--min-cells", "1", "--confirm", "2",
                              "--hold", "0"])
    assert json.load(open(tmp_path / "gated.json")) == gated and len(gated) == len(plain) == synth.TINY["duration"]
    frames = preprocessing.dca1000_frames(torch.from_numpy(np.fromfile(os.path.join(raw, "hori", "adc_data.bin"), dtype=np.int16)).cuda())
    occ = F_.cfar_ra(preprocessing.fft_chain_loader_means(frames), 1e-3, 2, 4, want_mask=False).summary.cpu().numpy()
    want = ref.ref_gate(occ[:, 0], 1, 2, 0)[0]
    for k, (a, b) in enumerate(zip(gated, plain)):
        assert set(a) == set(b) | {"present", "occupancy"} and "present" not in b
        assert {key: a[key] for key in b} == b
        assert a["occupancy"] == [float(v) for v in occ[k]] and a["present"] == int(want[k])
