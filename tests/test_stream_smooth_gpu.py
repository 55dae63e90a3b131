"""GPU (-m gpu): the Rauch-Tung-Striebel smoother behind the live stream and behind Runner.eval.
``PoseStream(track=..., history=True)`` on the 12 synthetic frames of tests/test_stream_track_gpu.py (3 silent pushes, 2 eager poses, 7
graph replays, 3 flushed poses): ``smoothed()`` against a ``SequenceSmoother`` fed the emitted maps, and the frames of a session with
``history=False`` against a session built without the argument — every comparison torch.equal.  ``Runner.eval`` through main.py on 8
frames of the synthetic data set: ``TEST.temporal: rts`` prints its MPJPE and Jitter lines and writes one record per frame; without
the key, and with ``off``, the printed lines and the JSON are those of an untouched config."""
import json
import os
import re

import numpy as np
import pytest
import torch
import yaml

from hupr_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
N = 12
RATE = 10.0
FIELDS = ("keypoints", "scores", "indices", "heatmap", "gcn_heatmap", "raw_keypoints", "velocity", "covariance", "forecast", "status")
SEQ = ("keypoints", "velocity", "covariance", "flag", "filtered", "raw", "status", "scores")


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
        self.model.math_mode = "bf16"
        self.ratio = self.cfg.DATASET.imgSize / self.cfg.DATASET.heatmapSize
        self.dev = [torch.from_numpy(np.concatenate([synth.adc_cube_int16(5, seq=0, frame=f, sensor=s) for f in range(N)])).cuda()
                    for s in range(2)]

    def session(self, **kw):
        from hupr_amd.tools import PoseStream, PoseTracking
        return PoseStream(self.model, self.cfg, decode="subpixel", track=PoseTracking(RATE), **kw)

    def play(self, s):
        out = []
        for n in range(N):
            pf = s.push(self.dev[0][n:n + 1], self.dev[1][n:n + 1])
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


def test_a_session_with_a_history_smooths_what_it_emitted(ctx):
    from hupr_amd.tools import SequenceSmoother, SmoothedSequence, TrackingError
    plain = ctx.session()
    as_today = ctx.play(plain)
    off = ctx.play(ctx.session(history=False))
    s = ctx.session(history=True)
    frames = ctx.play(s)
    assert bool(s._graphs) and plain._history is None
    for a, b, c in zip(as_today, off, frames):
        for k in FIELDS:
            assert torch.equal(getattr(a, k), getattr(b, k)), ("history=False", a.frame, k)
            assert torch.equal(getattr(a, k), getattr(c, k)), ("history=True", a.frame, k)
    with pytest.raises(TrackingError):
        plain.smoothed()
    seq = s.smoothed()
    assert isinstance(seq, SmoothedSequence) and len(seq) == N
    assert seq.keypoints.shape == (N, 1, 14, 2) and seq.covariance.shape == (N, 1, 14, 3) and seq.flag.shape == (N, 1, 14)
    # the history holds what the session emitted
    for k, pf in enumerate(frames):
        assert torch.equal(seq.filtered[k], pf.keypoints) and torch.equal(seq.raw[k], pf.raw_keypoints), k
        assert torch.equal(seq.status[k], pf.status) and torch.equal(seq.scores[k], pf.scores), k
    # the offline route over the same maps
    sm = SequenceSmoother(s.track, 14, "cuda")
    for pf in frames:
        sm.track(pf.gcn_heatmap, ctx.ratio, refine=True)
    want = sm.smooth()
    for k in SEQ:
        assert torch.equal(getattr(seq, k).reshape(getattr(want, k).shape), getattr(want, k)), k
    flag = seq.flag.cpu().numpy()
    assert (flag == 0).any() and (flag[-1] != 0).all()                           # SMOOTHED frames exist; the last frame never is one
    live = seq.status[:-1] != 4
    assert not torch.equal(seq.keypoints[:-1][live], seq.filtered[:-1][live])     # and the smoother moves them
    # reset() clears the history; the next sequence smooths to the same bits
    s.reset()
    with pytest.raises(ValueError):
        s.smoothed()
    ctx.play(s)
    again = s.smoothed()
    for k in SEQ:
        assert torch.equal(getattr(again, k), getattr(seq, k)), ("after reset", k)


def test_the_history_grows_by_doubling():
    from hupr_amd import functional as F_
    from hupr_amd.tools import PoseTracking, TrackHistory
    h = TrackHistory((3,), "cuda", capacity=2)
    state = F_.pose_track_state(3, "cuda")
    rng = np.random.RandomState(0)
    maps = torch.from_numpy(rng.uniform(0.0, 1.0, (5, 3, 64, 64)).astype(np.float32)).cuda()
    p = PoseTracking(RATE)
    kept = []
    for t in range(5):
        o = F_.pose_track(maps[t], 4.0, track_state=state, tracking=p)
        h.append(state, o[7], o[3], o[2], o[1])
        kept.append((state.clone(), o[7], o[3]))
    assert len(h) == 5 and h._capacity == 8
    seq = h.smooth(p)
    want = F_.pose_smooth_rts(torch.stack([k[0] for k in kept]), torch.stack([k[1] for k in kept]), torch.stack([k[2] for k in kept]), p)
    for got, w in zip((seq.keypoints, seq.velocity, seq.covariance, seq.flag), want):
        assert torch.equal(got, w)


def test_stream_command_with_rts_adds_the_smoothed_pose_to_every_record(ctx, tmp_path, monkeypatch):
    """python -m hupr_amd.tools.stream --track --rate 10 --rts on a tiny raw capture with a saved checkpoint."""
    from hupr_amd.tools import stream as st
    root = synth.write_tiny_dataset(str(tmp_path / "tinyraw"), cubes=False, raw=True)
    seq = synth.TINY["valName"][0]
    os.makedirs(tmp_path / "logs" / "streamtest")
    torch.save({"epoch": 3, "model_state_dict": ctx.model.state_dict(), "optimizer_state_dict": {}, "accuracy": 0.0},
               str(tmp_path / "logs" / "streamtest" / "model_best.pth"))
    monkeypatch.chdir(tmp_path)
    out = tmp_path / "poses.json"
    st.main(["--dir", "streamtest", "--raw", os.path.join(root, "single_%d" % seq), "--math", "bf16", "--out", str(out),
             "--decode", "subpixel", "--track", "--rate", "10", "--rts"])
    records = json.load(open(out))
    n = synth.TINY["duration"]
    assert [r["frame"] for r in records] == list(range(n))
    for r in records:
        assert set(r) == {"frame", "keypoints", "velocity", "covariance", "forecast", "status",
                          "smoothed", "smoothed_velocity", "smoothed_covariance", "smoothed_flag"}
        assert np.array(r["smoothed"]).shape == (14, 2) and np.array(r["smoothed_velocity"]).shape == (14, 2)
        assert np.array(r["smoothed_covariance"]).shape == (14, 3) and len(r["smoothed_flag"]) == 14
        for j, f in enumerate(r["smoothed_flag"]):
            assert (f == 2) == (r["status"][j] == 4)                              # PASSTHROUGH where the tracker says LOST
            if f in (1, 2):                                                     # END / PASSTHROUGH: the filter's own keypoint
                assert r["smoothed"][j] == r["keypoints"][j][:2]
    assert all(f in (1, 2) for f in records[-1]["smoothed_flag"])
    assert any(f == 0 for r in records for f in r["smoothed_flag"])


# ---- Runner.eval ----------------------------------------------------------------------------------------------------------------------------
FRAMES = 8


def _eval(tmp_path, monkeypatch, capsys, name, **test_keys):
    """main.py --eval on FRAMES synthetic frames with ``test_keys`` added to TEST -> (stdout lines, records of test_results.json)."""
    from hupr_amd import main as hmain
    from hupr_amd.config_tree import CONFIG_DIR
    cfgd = yaml.safe_load(open(os.path.join(CONFIG_DIR, "mscsa_prgcn.yaml")))
    cfgd["DATASET"]["dataDir"] = "synthetic"
    cfgd["TEST"]["batchSize"] = 4
    cfgd["TEST"].update(test_keys)
    for d in ("config", "logs", "visualization"):
        (tmp_path / d).mkdir(exist_ok=True)
    yaml.safe_dump(cfgd, open(tmp_path / "config" / (name + ".yaml"), "w"))
    monkeypatch.chdir(tmp_path)
    capsys.readouterr()
    hmain.main(["--config", name + ".yaml", "--dir", name, "--synthetic_length", str(FRAMES), "--eval"])
    out = capsys.readouterr().out
    print(out)
    return out.splitlines(), json.load(open(tmp_path / "logs" / name / "test_results.json"))


def test_eval_with_temporal_rts_scores_the_smoothed_keypoints(tmp_path, monkeypatch, capsys):
    lines, recs = _eval(tmp_path, monkeypatch, capsys, "rts", temporal="rts", tracking={"accel_psd": 100.0})
    assert len(recs) == FRAMES and [r["image_id"] for r in recs] == list(range(FRAMES))
    assert all(len(r["keypoints"]) == 42 and np.isfinite(r["keypoints"]).all() for r in recs)
    ap = next(i for i, l in enumerate(lines) if l.startswith("AP:"))
    tail = lines[ap + 1:]
    mp = [l for l in tail if l.startswith("MPJPE ")]
    assert [l.split(":")[0] for l in mp] == ["MPJPE raw", "MPJPE filtered", "MPJPE smoothed"]
    for l in mp:
        m = re.fullmatch(r"MPJPE \w+: (\S+) px \(n = (\d+)\)", l)
        assert m and np.isfinite(float(m.group(1))) and int(m.group(2)) == FRAMES, l
    jt = [l for l in tail if l.startswith("Jitter ")]
    assert [l.split(":")[0] for l in jt] == ["Jitter raw", "Jitter filtered", "Jitter smoothed", "Jitter truth"]
    for l in jt:
        m = re.fullmatch(r"Jitter \w+: (\S+) px", l)
        assert m and np.isfinite(float(m.group(1))), l
    assert tail.index(jt[0]) > tail.index(mp[-1])


def test_eval_without_the_key_is_todays(tmp_path, monkeypatch, capsys):
    plain_lines, plain = _eval(tmp_path, monkeypatch, capsys, "plain")
    off_lines, off = _eval(tmp_path, monkeypatch, capsys, "off", temporal="off", temporalRate=10.0)
    assert len(plain) == FRAMES and plain == off
    strip = lambda ls: [l for l in ls if "logs/" not in l]                      # the line that names the run's directory
    assert strip(plain_lines) == strip(off_lines)
    assert not any(l.startswith(("MPJPE", "Jitter")) for l in plain_lines)
    kp = np.array([r["keypoints"] for r in plain]).reshape(FRAMES, 14, 3)
    assert (kp[..., :2] % 4 == 0).all() and (kp[..., 2] == 1).all()              # the arg-max decode: whole heat-map pixels x 4
