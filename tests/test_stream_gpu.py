"""GPU (-m gpu): the live stream (hupr_amd.tools.stream, csrc/stream_window.hip) against the existing offline route.

Everything in front of the 3-D encoders is a pure function of one sensor-frame, so a session that transforms only the new frame and
runs the MNet over a ring of mean planes must reproduce ``engine.preprocess`` on the gathered ADC window + ``engine.infer`` bit for
bit: every comparison with that route here is ``torch.equal``.  Weights: synth.hupr_state with the gain of the model goldens (1.4,
de-flattened heads) and perturbed BatchNorm buffers; ADC frames: synth.adc_cube_int16."""
import json
import os

import numpy as np
import pytest
import torch

from hupr_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
D = 20                       # frames per test sequence: clamped head, steady state, ring wrap-around (G = 8), flush tail


def _planes_reference(L, bf16, planes, w, b):
    """hupr_mnet_fwd_means_* on gathered planes (n_bg, 16, pixels) -> (n_bg, pixels, 32)."""
    from hupr_amd import runtime as rt
    n_bg, _, pixels = planes.shape
    out = torch.empty((n_bg, pixels, 32), dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    fn = L.hupr_mnet_fwd_means_bf16act if bf16 else L.hupr_mnet_fwd_means_f32
    rt.check(fn(rt.ptr(planes), rt.ptr(w), rt.ptr(b), rt.ptr(out), None, n_bg, pixels, rt.stream()))
    return out


@pytest.mark.parametrize("lookahead", [3, 0, 1])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16act"])
def test_stream_window_kernel_equals_mnet_on_gathered_planes(bf16, lanes, lookahead):
    """hupr_mnet_stream_* + hupr_stream_advance over a 20-frame stream (and its flush tail) == hupr_mnet_fwd_means_* on the planes
    index_select gathers by the window rule: every frame, both sensors, both stores."""
    from hupr_amd import runtime as rt
    from hupr_amd.tools.stream import stream_window_sources
    L = rt.lib()
    G, pixels = 8, 64 * 64
    gen = torch.Generator(device="cuda").manual_seed(11 + lanes)
    planes = torch.randn((2, lanes, D, 16, pixels), device="cuda", generator=gen)
    ws = [torch.randn((32, 2, 2, 1, 1), device="cuda", generator=gen) * 0.5 for _ in range(2)]
    bs = [torch.randn((32,), device="cuda", generator=gen) * 0.5 for _ in range(2)]
    staging = torch.empty((2, lanes, 16, pixels), device="cuda")
    ring = torch.full((2, lanes, G, 16, pixels), float("nan"), device="cuda")          # a slot read before it is filed would show
    state = torch.full((int(L.hupr_stream_state_bytes()),), 0x5A, dtype=torch.uint8, device="cuda")
    act = torch.bfloat16 if bf16 else torch.float32
    outs = [torch.empty((lanes, G, pixels, 32), dtype=act, device="cuda") for _ in range(2)]
    fn = L.hupr_mnet_stream_bf16act if bf16 else L.hupr_mnet_stream_f32
    rt.check(L.hupr_stream_reset(rt.ptr(state), rt.stream()))

    def step(flush):
        rt.check(fn(None if flush else rt.ptr(staging), rt.ptr(ring), rt.ptr(state), lookahead, int(flush), rt.ptr(ws[0]),
                    rt.ptr(bs[0]), rt.ptr(ws[1]), rt.ptr(bs[1]), rt.ptr(outs[0]), rt.ptr(outs[1]), lanes, G, pixels, rt.stream()))
        rt.check(L.hupr_stream_advance(rt.ptr(state), lookahead, int(flush), rt.stream()))

    def check(center, newest):
        idx = torch.tensor(stream_window_sources(center, newest, G), device="cuda")
        for s in range(2):
            gathered = planes[s].index_select(1, idx).reshape(lanes * G, 16, pixels).contiguous()
            want = _planes_reference(L, bf16, gathered, ws[s], bs[s]).view(lanes, G, pixels, 32)
            assert torch.equal(outs[s], want), (center, newest, s)

    checked = 0
    for n in range(D):
        staging.copy_(planes[:, :, n])
        step(False)
        if n >= lookahead:
            check(n - lookahead, n)
            checked += 1
    for c in range(D - lookahead, D):
        step(True)
        check(c, D - 1)
        checked += 1
    assert checked == D
    counters = state.cpu().numpy().view(np.int32)
    assert counters[0] == D and counters[1] == D
    rt.check(L.hupr_stream_reset(rt.ptr(state), rt.stream()))
    assert not state.cpu().numpy().any()


# ---- the session against the offline route -----------------------------------------------------------------------------------------
class _Ctx:
    """One engine (its model carries the synthetic weights), the 2 x 20 frames of two sequences on host and device, and the offline
    route's results per (mode, lane sequence, window)."""

    def __init__(self):
        from hupr_amd.config_tree import load_config
        from hupr_amd.tools.engine import TrainEngine
        g = np.load(os.path.join(GOLD, "model_eval.npz"))
        self.cfg = load_config()
        self.engine = TrainEngine(self.cfg, device="cuda")
        self.model = self.engine.model
        self.state = {k: torch.from_numpy(np.array(v)) for k, v in synth.hupr_state(int(g["model_seed"]), gain=float(g["gain"])).items()}
        self.model.load_state_dict(self.state)
        self.model.eval()
        self.G = self.cfg.DATASET.numGroupFrames
        self.K, self.H = self.cfg.DATASET.numKeypoints, self.cfg.DATASET.heatmapSize
        self.ratio = self.cfg.DATASET.imgSize / self.cfg.DATASET.heatmapSize
        # host[seq][sensor]: (D, 4, 192, 256, 2) int16
        self.host = [[torch.from_numpy(np.concatenate([synth.adc_cube_int16(5, seq=q, frame=f, sensor=s) for f in range(D)]))
                      for s in range(2)] for q in range(2)]
        self.dev = [[t.cuda() for t in seq] for seq in self.host]
        self.offline_cache = {}

    def offline(self, mode, seqs, window):
        """The existing route on one window: engine.preprocess on the gathered ADC frames, engine.infer, arg-max, get_max_preds."""
        key = (mode, tuple(seqs), tuple(window))
        if key not in self.offline_cache:
            self.offline_cache[key] = self.offline_uncached(mode, seqs, window)
        return self.offline_cache[key]

    def offline_uncached(self, mode, seqs, window):
        from hupr_amd import functional as F_
        from hupr_amd.misc.metrics import get_max_preds
        self.model.math_mode = mode
        idx = torch.tensor(window, device="cuda")
        hori = torch.cat([self.dev[q][0].index_select(0, idx) for q in seqs])
        vert = torch.cat([self.dev[q][1].index_select(0, idx) for q in seqs])
        h, v = self.engine.preprocess(hori, vert)
        p1, p2 = self.engine.infer(h, v)
        am, mx = F_.argmax_rows(p2.reshape(-1, self.H * self.H))
        kp, _ = get_max_preds(p2.reshape(-1, self.K, self.H, self.H))
        return p1, p2, am.view(len(seqs), self.K), mx.view(len(seqs), self.K), kp * self.ratio

    def session(self, mode, **kw):
        from hupr_amd.tools import PoseStream
        self.model.math_mode = mode
        return PoseStream(self.model, self.cfg, **kw)

    def frames(self, seqs, n, host):
        src = self.host if host else self.dev
        return (torch.stack([src[q][0][n] for q in seqs]), torch.stack([src[q][1][n] for q in seqs]))

    def assert_frame(self, pf, want, what):
        p1, p2, am, mx, kp = want
        assert torch.equal(pf.heatmap, p1), what
        assert torch.equal(pf.gcn_heatmap, p2), what
        assert torch.equal(pf.indices, am) and torch.equal(pf.scores, mx), what
        got = pf.keypoints.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == kp.shape and np.array_equal(got, kp), what


@pytest.fixture(scope="module")
def ctx():
    c = _Ctx()
    yield c
    c.engine.close()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_control_existing_route_is_run_to_run_identical(ctx, mode):
    """The yardstick of the comparisons below: the offline route twice on one window gives the same bits."""
    window = [0, 0, 1, 2, 3, 4, 5, 6]
    a = ctx.offline_uncached(mode, (0,), window)
    b = ctx.offline_uncached(mode, (0,), window)
    for x, y in zip(a[:4], b[:4]):
        spread = (x.float() - y.float()).abs().max().item()
        print("control %s: run-to-run max-abs spread %.3e" % (mode, spread))
        assert torch.equal(x, y)
    assert np.array_equal(a[4], b[4])
    # heads are not flat: the arg-max positions differ between joints
    assert len(set(a[2].cpu().numpy().reshape(-1).tolist())) > 1


@pytest.mark.parametrize("lookahead", [None, 0], ids=["default", "zero"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_session_equals_offline_route(ctx, mode, graph, lookahead):
    """Every emitted PoseFrame of a 20-frame sequence (both heat-maps, arg-max indices, scores, keypoints) == the existing route on
    window_indices(pos, 20, G) — for lookahead 0 on stream_window_sources(c, c, G).  Host frames through the pinned staging."""
    from hupr_amd.datasets.dataset import window_indices
    from hupr_amd.tools.stream import stream_window_sources
    s = ctx.session(mode, graph=graph, lookahead=lookahead)
    L = s.lookahead
    assert L == (3 if lookahead is None else 0)
    emitted = []
    for n in range(D):
        pf = s.push(*ctx.frames((0,), n, host=True))
        assert s.frames_pushed == n + 1
        if n < L:
            assert pf is None
            continue
        c = n - L
        assert pf.frame == c
        window = window_indices(c, D, ctx.G) if lookahead is None else stream_window_sources(c, c, ctx.G)
        if lookahead is None and c + L < D:
            assert window == stream_window_sources(c, n, ctx.G)
        ctx.assert_frame(pf, ctx.offline(mode, (0,), window), (mode, graph, L, c))
        emitted.append(c)
    tail = s.flush()
    assert len(tail) == L
    for pf in tail:
        ctx.assert_frame(pf, ctx.offline(mode, (0,), window_indices(pf.frame, D, ctx.G)), (mode, graph, L, pf.frame, "flush"))
        emitted.append(pf.frame)
    assert emitted == list(range(D)) and s.frames_emitted == D
    assert bool(s._graphs) == graph


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_two_lanes_advance_in_lock_step(ctx, mode):
    """lanes = 2 (device frames, graph) and two single-lane sessions on the same frames.
    (a) The two-lane session == the existing route run on the two windows as one batch of 2, and each single-lane session == the
        existing route on its window as a batch of 1: torch.equal, every frame.
    (b) Two lanes against the two single-lane sessions: the EXISTING route is not bit-equal between a batch of 2 and two batches of
        1 (other launch routes: single-sample attention batching, K-sliced convolutions, split-K — other summation orders), so
        neither are the sessions.  The test measures the existing route's batch-of-2 minus batch-of-1 difference on every window
        and asserts that the sessions show exactly that difference, element for element, on both heat-maps, the scores, the
        arg-max positions and the keypoints — no tolerance.  Measured on an MI355X over the 12 frames x 2 lanes: f32 heat-maps
        differ by at most 3.6e-07 (0 of 336 arg-max positions differ), bf16 by at most 8.7e-04 (1 of 336); both figures are printed."""
    from hupr_amd.datasets.dataset import window_indices
    two = ctx.session(mode, lanes=2, graph=True)
    ones = [ctx.session(mode, lanes=1, graph=False) for _ in range(2)]
    worst, moved, joints = 0.0, 0, 0
    n_frames = 12

    def compare(pf, singles):
        nonlocal worst, moved, joints
        window = window_indices(pf.frame, n_frames, ctx.G)
        off2 = ctx.offline(mode, (0, 1), window)
        ctx.assert_frame(pf, off2, (mode, pf.frame, "batch of 2"))
        for lane, one in enumerate(singles):
            assert one.frame == pf.frame
            off1 = ctx.offline(mode, (lane,), window)
            ctx.assert_frame(one, off1, (mode, pf.frame, lane))
            what = (mode, pf.frame, lane, "two lanes - single lane == existing batch of 2 - batch of 1")
            for got2, got1, ref2, ref1 in ((pf.heatmap, one.heatmap, off2[0], off1[0]), (pf.gcn_heatmap, one.gcn_heatmap, off2[1], off1[1]),
                                           (pf.scores, one.scores, off2[3], off1[3])):
                assert torch.equal(got2[lane] - got1[0], ref2[lane] - ref1[0]), what
                worst = max(worst, (ref2[lane] - ref1[0]).abs().max().item())
            assert torch.equal(pf.indices[lane] - one.indices[0], off2[2][lane] - off1[2][0]), what
            assert np.array_equal(pf.keypoints[lane].cpu().numpy() - one.keypoints[0].cpu().numpy(), off2[4][lane] - off1[4][0]), what
            moved += int((off2[2][lane] != off1[2][0]).sum().item())
            joints += ctx.K

    for n in range(n_frames):
        pf = two.push(*ctx.frames((0, 1), n, host=False))
        singles = [ones[q].push(*ctx.frames((q,), n, host=False)) for q in range(2)]
        if pf is None:
            assert singles == [None, None]
            continue
        compare(pf, singles)
    tails = [o.flush() for o in ones]
    for k, pf in enumerate(two.flush()):
        compare(pf, [tails[0][k], tails[1][k]])
    assert joints == n_frames * 2 * ctx.K
    print("existing route, batch of 2 vs two batches of 1 (%s): max-abs heat-map / score difference %.3e, %d of %d arg-max positions differ"
          % (mode, worst, moved, joints))


def test_reset_reproduces_the_sequence(ctx):
    s = ctx.session("bf16", graph=True)

    def run():
        got = []
        for n in range(10):
            pf = s.push(*ctx.frames((0,), n, host=True))
            if pf is not None:
                got.append(pf.cpu())
        got.extend(pf.cpu() for pf in s.flush())
        return got

    first = run()
    with pytest.raises(ValueError):
        s.push(*ctx.frames((0,), 0, host=True))           # flush() ended the sequence
    s.reset()
    assert s.frames_pushed == 0 and s.frames_emitted == 0
    second = run()
    assert [p.frame for p in first] == [p.frame for p in second] == list(range(10))
    for a, b in zip(first, second):
        for k in ("keypoints", "scores", "indices", "heatmap", "gcn_heatmap"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (a.frame, k)
    # another sequence after a reset is that sequence, not a mixture with what the ring held
    s.reset()
    from hupr_amd.datasets.dataset import window_indices
    for n in range(6):
        pf = s.push(*ctx.frames((1,), n, host=True))
        if pf is not None:
            ctx.assert_frame(pf, ctx.offline("bf16", (1,), window_indices(pf.frame, D, ctx.G)), ("after reset", pf.frame))


def test_weight_change_between_pushes_reaches_the_graph(ctx):
    """param.mul_ + invalidate_packed between two pushes: the next graph push == a fresh eager session on the changed weights."""
    from hupr_amd import functional as F_
    s = ctx.session("bf16", graph=True)
    try:
        for n in range(8):
            s.push(*ctx.frames((0,), n, host=True))
        assert s._graphs                                        # steady state runs from the graph by now
        s.push(*ctx.frames((0,), 8, host=True))
        from hupr_amd.datasets.dataset import window_indices
        old_weights = ctx.offline_uncached("bf16", (0,), window_indices(6, D, ctx.G))      # frame 6 before the change
        with torch.no_grad():
            for p in ctx.model.parameters():
                p.mul_(0.9)
        F_.invalidate_packed()
        after = s.push(*ctx.frames((0,), 9, host=True))
        fresh = ctx.session("bf16", graph=False)
        for n in range(10):
            want = fresh.push(*ctx.frames((0,), n, host=True))
        assert want.frame == after.frame == 6
        for k in ("keypoints", "scores", "indices", "heatmap", "gcn_heatmap"):
            assert torch.equal(getattr(after, k), getattr(want, k)), k
        assert not torch.equal(after.gcn_heatmap, old_weights[1])      # the change is visible at all: the same frame on the old weights
    finally:
        ctx.model.load_state_dict(ctx.state)
        F_.invalidate_packed()
        ctx.offline_cache.clear()


def test_steady_state_is_one_graph_replay_and_no_eager_launch(ctx, monkeypatch):
    from hupr_amd import runtime as rt
    L = rt.lib()
    s = ctx.session("bf16", graph=True)
    for n in range(8):
        s.push(*ctx.frames((0,), n, host=True))
    assert list(s._graphs) == ["host"]
    replays = []
    real = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(self), real(self))[1])
    for n in range(8, D):
        c0 = L.hupr_launch_count()
        pf = s.push(*ctx.frames((0,), n, host=True))
        assert L.hupr_launch_count() == c0, "an eager library launch in a steady-state push"
        assert len(replays) == n - 7 and replays[-1] is s._graphs["host"][0]
        assert pf.frame == n - 3
    torch.cuda.synchronize()


def test_stream_command_matches_the_raw_capture_dataset(ctx, tmp_path, monkeypatch):
    """python -m hupr_amd.tools.stream on a tiny raw capture with a saved checkpoint: the keypoints written == HuPRRawADC items ->
    engine.infer -> get_max_preds x imgHeatmapRatio, frame for frame."""
    import copy
    from hupr_amd.datasets import getDataset
    from hupr_amd.misc.metrics import get_max_preds
    from hupr_amd.tools import stream as st

    class _Args:
        sampling_ratio = 1

    root = synth.write_tiny_dataset(str(tmp_path / "tinyraw"), cubes=False, raw=True)
    seq = synth.TINY["valName"][0]
    os.makedirs(tmp_path / "logs" / "streamtest")
    torch.save({"epoch": 3, "model_state_dict": ctx.model.state_dict(), "optimizer_state_dict": {}, "accuracy": 0.0},
               str(tmp_path / "logs" / "streamtest" / "model_best.pth"))
    monkeypatch.chdir(tmp_path)
    out = tmp_path / "poses.json"
    st.main(["--dir", "streamtest", "--raw", os.path.join(root, "single_%d" % seq), "--math", "f32", "--out", str(out)])
    records = json.load(open(out))
    n = synth.TINY["duration"]
    assert [r["frame"] for r in records] == list(range(n))

    cfg = copy.deepcopy(ctx.cfg)
    cfg.DATASET.dataDir = cfg.DATASET.rawDir = str(root)
    cfg.DATASET.duration = n
    cfg.DATASET.trainName, cfg.DATASET.valName, cfg.DATASET.testName = (synth.TINY[k] for k in ("trainName", "valName", "testName"))
    ds = getDataset("val", cfg, _Args(), random=False)
    assert len(ds) == n
    ctx.model.math_mode = "f32"
    for i in range(n):
        it = ds[i]
        _, p2 = ctx.engine.infer(it["VRDAEmap_hori"][None], it["VRDAEmap_vert"][None])
        kp, mx = get_max_preds(p2.reshape(-1, ctx.K, ctx.H, ctx.H))
        got = np.asarray(records[i]["keypoints"])
        assert got.shape == (ctx.K, 3)
        assert np.array_equal(got[:, :2].astype(np.float32), (kp * ctx.ratio)[0]), i
        assert np.array_equal(got[:, 2].astype(np.float32), mx[0, :, 0]), i
