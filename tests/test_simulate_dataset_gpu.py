"""GPU (-m gpu): a simulated data set of the tiny shape (hupr_amd.simulate.write_simulated_dataset) read back by the raw-capture
dataset with no change to it, and one of its sequences through the live stream's presence gate.

The gate's verdict is known before the device is asked.  Receiver noise of 2 ADC units per component, ``PresenceGate(pfa=1e-5, guard=2,
train=4, min_cells=3, confirm=2, hold=2)``, data-set seed 11, sequence single_7: through the fp64 restatements (tests/radar_scene_ref.py,
tests/tdm_ref.py's loader, tests/cfar_ref.py) on the CPU, with numpy noise of the same level, the six frames with the body hold 178, 175,
96, 58, 95 and 82 detections and the empty room none, against ``min_cells`` 3.  Here the same restatement of the detector runs on the
device chain's planes and must give that verdict again; the stream must follow it."""
import os

import numpy as np
import pytest
import torch

import cfar_ref
from hupr_amd import simulate as sim
from hupr_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SEED, NOISE = 11, 2.0
GATE = dict(pfa=1e-5, guard=2, train=4, min_cells=3, confirm=2, hold=2)
DUR = synth.TINY["duration"]
NAMES = {"train": synth.TINY["trainName"], "val": synth.TINY["valName"]}


class _Args:
    sampling_ratio = 1


def _cfg(root):
    import copy
    from hupr_amd.config_tree import load_config
    cfg = copy.deepcopy(load_config())
    cfg.DATASET.dataDir = cfg.DATASET.rawDir = str(root)
    cfg.DATASET.duration = DUR
    cfg.DATASET.trainName, cfg.DATASET.valName, cfg.DATASET.testName = (synth.TINY[k] for k in ("trainName", "valName", "testName"))
    return cfg


def _sequence(seq, model, empty=False):
    s = sim.sequence_seed(SEED, seq)
    body = sim.walking_body(DUR, model.frame_rate_hz, s)
    return sim.simulate_sequence(model, body.with_amp(0.0) if empty else body, noise_std=NOISE, seed=s)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    model = sim.RadarModel()
    root = sim.write_simulated_dataset(str(tmp_path_factory.mktemp("sim")), NAMES, DUR, SEED, model=model, noise_std=NOISE)
    return root, model


def test_the_raw_capture_dataset_reads_the_simulated_tree(tree):
    from hupr_amd import preprocessing
    from hupr_amd.datasets import HuPRRawADC, getDataset, window_indices
    root, model = tree
    cubes = {}
    for seq in NAMES["train"] + NAMES["val"]:
        cubes[seq] = _sequence(seq, model)
        for sensor, want in zip(("hori", "vert"), cubes[seq]):
            raw = np.fromfile(os.path.join(root, "single_%d" % seq, sensor, "adc_data.bin"), dtype=np.int16)
            got = preprocessing.dca1000_frames(torch.from_numpy(raw).cuda())
            assert got.shape == (DUR, 4, 192, 256, 2) and torch.equal(got, want)              # bit for bit
            assert int(want.abs().max()) > 50                                                  # a body, not only noise
    ds = getDataset("train", _cfg(root), _Args(), random=False)
    assert isinstance(ds, HuPRRawADC) and len(ds) == 2 * DUR
    for idx in (0, 4, 7, 11):
        it = ds[idx]
        seq = NAMES["train"][idx // DUR]
        frames = [i - (idx // DUR) * DUR for i in window_indices(idx, DUR, 8)]
        for si, sensor in enumerate(("hori", "vert")):
            assert torch.equal(it["VRDAEmap_" + sensor], preprocessing.fft_chain_loader(cubes[seq][si][frames]))
        assert it["imageId"] == idx % DUR + 100000 * seq
        want = sim.project_joints(sim.walking_body(DUR, model.frame_rate_hz, sim.sequence_seed(SEED, seq)).joints3d[idx % DUR])
        assert np.array_equal(it["jointsFloat"].numpy(), want) and tuple(it["jointsGroup"].shape) == (14, 2)


def _counts(cube_hori):
    """The fp64 restatement of the detector on the device chain's mean planes -> detections per frame."""
    from hupr_amd import preprocessing
    planes = preprocessing.fft_chain_loader_means(cube_hori).cpu().numpy()
    return cfar_ref.ref_cfar(planes, GATE["pfa"], GATE["guard"], GATE["train"])["summary"][:, 0]


def test_the_presence_gate_sees_the_body_and_not_the_empty_room(tree):
    from hupr_amd.config_tree import load_config
    from hupr_amd.tools import PoseStream, PresenceGate
    from hupr_amd.tools.engine import TrainEngine
    _, model = tree
    seq = NAMES["val"][0]
    g = np.load(os.path.join(GOLD, "model_eval.npz"))
    cfg = load_config()
    engine = TrainEngine(cfg, device="cuda")
    try:
        net = engine.model
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.hupr_state(int(g["model_seed"]), gain=float(g["gain"])).items()})
        net.eval()
        net.math_mode = "bf16"
        verdicts = {}
        for empty in (False, True):
            hori, vert = _sequence(seq, model, empty=empty)
            counts = _counts(hori)
            want = cfar_ref.ref_gate(counts, GATE["min_cells"], GATE["confirm"], GATE["hold"])[0]
            print("%s: detections per frame %s, gate %s" % ("empty room" if empty else "body", counts.tolist(), want.tolist()))
            s = PoseStream(net, cfg, lanes=1, lookahead=0, presence=PresenceGate(**GATE))
            out = [s.push(hori[n:n + 1], vert[n:n + 1]).clone() for n in range(DUR)]
            assert [int(pf.present[0]) for pf in out] == want.tolist()
            assert [float(pf.occupancy[0, 0]) for pf in out] == counts.tolist()
            verdicts[empty] = (counts, want.tolist())
        # the verdict the CPU gave: every frame with the body is a hit, so the gate is up from its second frame on; the empty room never
        assert (verdicts[False][0] >= 10 * GATE["min_cells"]).all() and verdicts[False][1] == [0] + [1] * (DUR - 1)
        assert (verdicts[True][0] < GATE["min_cells"]).all() and verdicts[True][1] == [0] * DUR
    finally:
        engine.close()
