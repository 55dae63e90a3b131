"""CPU (-m "not gpu"): TRAINING.emaDecay — the three C-ABI entries of the weight average are declared, exported and bound and refuse
bad arguments on the host, the key's values map to off / a decay, and WeightEMA's host bookkeeping (allocation, state dict, load)
works on CPU tensors without a launch."""
import ctypes
import os
import re
import types

import pytest
import torch

from hupr_amd.tools.distributed import GradientBuckets
from hupr_amd.tools.ema import WeightEMA, ema_decay_setting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMA_ENTRIES = ("hupr_ema_tick_f32", "hupr_ema_update_f32", "hupr_swap_f32")
ABSENT = object()
A, B, S = 0x10000, 0x20000, 0x30000           # never dereferenced: every call below is refused before a launch


def _cfg(decay=ABSENT):
    training = types.SimpleNamespace(optimizer="adam")
    if decay is not ABSENT:
        training.emaDecay = decay
    return types.SimpleNamespace(TRAINING=training)


def test_ema_entry_points_are_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hupr.h")).read(), flags=re.S)
    lib = ctypes.CDLL(runtime.LIB_PATH)
    for name in EMA_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
        assert name in runtime.SIGNATURES, name
    v, f, n = ctypes.c_void_p, ctypes.c_float, ctypes.c_long
    assert runtime.SIGNATURES["hupr_ema_tick_f32"] == (ctypes.c_int, [v, f, v, v])
    assert runtime.SIGNATURES["hupr_ema_update_f32"] == (ctypes.c_int, [v, v, n, v, v])
    assert runtime.SIGNATURES["hupr_swap_f32"] == (ctypes.c_int, [v, v, n, v])


def test_ema_entries_refuse_bad_arguments_without_a_gpu():
    """Argument errors are found on the host, before any launch: -1 and a message that names the entry."""
    from hupr_amd import runtime as rt
    L = rt.lib()
    before = L.hupr_launch_count()

    def refused(name, *args):
        assert getattr(L, name)(*args, None) == -1, (name, args)
        assert name.encode() in L.hupr_last_error(), (name, args, L.hupr_last_error())

    refused("hupr_ema_tick_f32", None, 0.999, None)
    refused("hupr_ema_tick_f32", None, 0.999, A)
    for decay in (0.0, 1.0, 1.5, -0.1, float("nan")):
        refused("hupr_ema_tick_f32", S, decay, None)
        refused("hupr_ema_tick_f32", S, decay, A)
    for ema, p, n, state in [(None, B, 16, S), (A, None, 16, S), (A, B, 16, None), (A, B, 0, S), (A, B, -4, S)]:
        refused("hupr_ema_update_f32", ema, p, n, state)
    for a, b, n in [(None, B, 16), (A, None, 16), (A, B, 0), (A, B, -4)]:
        refused("hupr_swap_f32", a, b, n)
    for a, b, n in [(A, A, 16), (A, A + 4, 16), (A + 60, A, 16), (A, A + 4 * 15, 16), (A + 4, A, 1 << 20)]:      # overlapping ranges
        refused("hupr_swap_f32", a, b, n)
    assert L.hupr_launch_count() == before


def test_ema_decay_setting_values():
    for decay, want in [(ABSENT, None), (-1, None), (-1.0, None), (0.999, 0.999), (0.5, 0.5)]:
        got = ema_decay_setting(_cfg(decay))
        assert got == want and (want is None or type(got) is float), (decay, got)


@pytest.mark.parametrize("bad", [0, 1, 2, -0.5, float("nan"), "0.9", True, None, 0.0, 1.0, False, float("inf")])
def test_ema_decay_setting_refuses_other_values(bad):
    with pytest.raises(ValueError, match="TRAINING.emaDecay"):
        ema_decay_setting(_cfg(bad))


def test_shipped_yaml_does_not_carry_the_key():
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    assert not hasattr(cfg.TRAINING, "emaDecay")
    assert ema_decay_setting(cfg) is None


def _net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.BatchNorm1d(16), torch.nn.Linear(16, 4), torch.nn.Linear(4, 2))


def test_weight_ema_host_bookkeeping_on_cpu_tensors():
    net = _net()
    gb = GradientBuckets(net, bucket_bytes=256, tail_bytes=0)
    pairs, layout = gb.flat_pairs(), gb.layout()
    assert len(pairs) >= 2
    ema = WeightEMA(pairs, layout, 0.999, module=net)
    assert ema.decay == 0.999 and not ema.swapped
    assert len(ema.flat) == len(pairs)
    for e, (p, _) in zip(ema.flat, pairs):
        assert e.dtype == torch.float32 and e.shape == p.shape and torch.equal(e, p) and e.data_ptr() != p.data_ptr()
    assert ema.stats() == {"updates": 0, "weight": 0.0}

    # a complete state dict of the network: parameters from the average, buffers cloned from the model
    for i, e in enumerate(ema.flat):
        e.copy_(torch.arange(e.numel(), dtype=torch.float32) + 1000.0 * (i + 1))
    net[1].running_mean.fill_(0.25)
    net[1].num_batches_tracked.fill_(5)
    ref, sd = net.state_dict(), ema.state_dict(net)
    assert list(sd) == list(ref)
    for k in ref:
        assert sd[k].shape == ref[k].shape and sd[k].dtype == ref[k].dtype, k
        assert sd[k].data_ptr() != ref[k].data_ptr(), k
    names = dict(net.named_parameters())
    for k in ref:
        if k in names:
            assert not torch.equal(sd[k], ref[k]), k
        else:
            assert torch.equal(sd[k], ref[k]), k
    for i, entries in enumerate(layout):
        for p, off, n in entries:
            key = [k for k, q in names.items() if q is p][0]
            assert torch.equal(sd[key].reshape(-1), ema.flat[i][off:off + n]), key
    twin = _net()
    twin.load_state_dict(sd, strict=True)
    assert twin[1].num_batches_tracked.item() == 5 and twin[1].running_mean[0].item() == 0.25

    # ... which a second instance restores exactly, with the update count
    ema2 = WeightEMA(pairs, layout, 0.999, module=net)
    ema2.load_state_dict(sd, updates=7)
    for a, b in zip(ema.flat, ema2.flat):
        assert torch.equal(a, b)
    assert ema2.stats() == {"updates": 7, "weight": 0.0}
    for (p, _), e in zip(pairs, ema.flat):
        assert not torch.equal(p, e)                                 # the parameters were not touched by any of this

    ema.swapped = True
    for call in (lambda: ema.state_dict(net), lambda: ema.load_state_dict(sd, 1), ema.reset, ema.update):
        with pytest.raises(RuntimeError, match="swapped"):
            call()
    ema.swapped = False
    ema.reset()
    for e, (p, _) in zip(ema.flat, pairs):
        assert torch.equal(e, p)
    assert ema.stats()["updates"] == 0


def test_weight_ema_needs_names_a_full_layout_and_a_valid_decay():
    net = _net()
    gb = GradientBuckets(net, bucket_bytes=256, tail_bytes=0)
    pairs, layout = gb.flat_pairs(), gb.layout()
    for bad in (0.0, 1.0, -0.5, 2.0, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            WeightEMA(pairs, layout, bad)
    with pytest.raises(ValueError, match="layout"):
        WeightEMA(pairs, None, 0.9)
    ema = WeightEMA(pairs, layout, 0.9)
    with pytest.raises(RuntimeError, match="names"):
        ema.load_state_dict(net.state_dict(), 0)
    # a parameter outside the buckets (frozen when they were made): the averaged state dict would not be complete
    net2 = _net()
    net2[3].bias.requires_grad_(False)
    gb2 = GradientBuckets(net2, bucket_bytes=256, tail_bytes=0)
    with pytest.raises(RuntimeError, match="3.bias"):
        WeightEMA(gb2.flat_pairs(), gb2.layout(), 0.9).state_dict(net2)


def test_checkpoint_keys_follow_the_setting():
    """_checkpoint_dict: the reference's four keys without an average, two more with one."""
    from hupr_amd.tools.base import BaseRunner
    net = _net()
    gb = GradientBuckets(net, bucket_bytes=256, tail_bytes=0)
    r = BaseRunner.__new__(BaseRunner)
    r.model, r.optimizer = net, torch.optim.SGD(net.parameters(), lr=0.1)
    r.logger = types.SimpleNamespace(showBestAP=lambda: 0.0)
    assert list(r._checkpoint_dict(3)) == ["epoch", "model_state_dict", "optimizer_state_dict", "accuracy"]
    r.engine = types.SimpleNamespace(ema=None)
    assert list(r._checkpoint_dict(3)) == ["epoch", "model_state_dict", "optimizer_state_dict", "accuracy"]
    r.engine.ema = WeightEMA(gb.flat_pairs(), gb.layout(), 0.9, module=net)
    ck = r._checkpoint_dict(3)
    assert list(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "accuracy", "ema_state_dict", "ema_updates"]
    assert ck["ema_updates"] == 0 and list(ck["ema_state_dict"]) == list(net.state_dict())
