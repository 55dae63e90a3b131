"""GPU (-m gpu): ``TEST.presence`` in Runner.eval on the miniature dataset of synth.write_tiny_dataset — stored cubes and raw captures.
With the key the evaluation prints the ``Presence:`` line; without it the output is what it was."""
import os
import re

import pytest
import yaml

from hupr_amd import synth

pytestmark = pytest.mark.gpu
LINE = re.compile(r"^Presence: (\d\.\d{3}|nan) of (\d+) labelled frames present, median (\S+) detections$", re.M)


def _eval(tmp_path, monkeypatch, capsys, name, raw, presence):
    from hupr_amd import main as hmain
    from hupr_amd.config_tree import CONFIG_DIR
    root = tmp_path / ("tinyraw" if raw else "tiny")
    if not root.exists():
        synth.write_tiny_dataset(str(root), cubes=not raw, raw=raw, phases=("test",))
    cfgd = yaml.safe_load(open(os.path.join(CONFIG_DIR, "mscsa_prgcn.yaml")))
    cfgd["DATASET"].update(dataDir=str(root), duration=synth.TINY["duration"], trainName=synth.TINY["trainName"],
                           valName=synth.TINY["valName"], testName=synth.TINY["testName"])
    if raw:
        cfgd["DATASET"]["rawDir"] = str(root)
    cfgd["TEST"]["batchSize"] = 4                      # 6 frames: a full batch and a ragged one
    if presence is not None:
        cfgd["TEST"]["presence"] = presence
    for d in ("config", "logs", "visualization"):
        (tmp_path / d).mkdir(exist_ok=True)
    yaml.safe_dump(cfgd, open(tmp_path / "config" / (name + ".yaml"), "w"))
    monkeypatch.chdir(tmp_path)
    capsys.readouterr()
    hmain.main(["--config", name + ".yaml", "--dir", name, "--eval"])
    return capsys.readouterr().out


def test_stored_cubes_print_the_presence_line_and_nothing_else_changes(tmp_path, monkeypatch, capsys):
    plain = _eval(tmp_path, monkeypatch, capsys, "plain", False, None)
    off = _eval(tmp_path, monkeypatch, capsys, "off", False, False)
    on = _eval(tmp_path, monkeypatch, capsys, "on", False, {"pfa": 1e-3, "min_cells": 1, "confirm": 1, "hold": 0})
    assert "Presence" not in plain and "Presence" not in off and "AP: " in plain
    ap = lambda s: [l for l in s.splitlines() if l.startswith("AP: ")]
    rest = lambda s: [l.split(":")[0] for l in s.splitlines() if not l.startswith("Presence:")]
    assert len(ap(plain)) == 1 and ap(off) == ap(plain) and ap(on) == ap(plain)      # the scores are what they were
    assert rest(off) == rest(plain) and rest(on) == rest(plain)                      # and so is every other line, by its head
    m = LINE.findall(on)
    assert len(m) == 1 and int(m[0][1]) == synth.TINY["duration"] * len(synth.TINY["testName"])
    # unit noise at pfa = 1e-3: some tens of false alarms in every frame, so this permissive gate calls every frame present
    assert float(m[0][0]) == 1.0 and float(m[0][2]) >= 1


def test_raw_captures_print_the_presence_line(tmp_path, monkeypatch, capsys):
    out = _eval(tmp_path, monkeypatch, capsys, "raw", True, True)
    m = LINE.findall(out)
    assert len(m) == 1 and int(m[0][1]) == synth.TINY["duration"] * len(synth.TINY["testName"])
    assert 0.0 <= float(m[0][0]) <= 1.0


def test_a_bad_key_is_refused_where_the_config_is_read(tmp_path, monkeypatch, capsys):
    with pytest.raises(ValueError, match="TEST.presence"):
        _eval(tmp_path, monkeypatch, capsys, "bad", False, {"guard": 5, "train": 4})
