"""CPU (-m "not gpu"): TRAINING.optimizer = sgd — the optimiser choice of the reference (tools/base.py:44-47), FusedSGD's
checkpoint interchange with torch.optim.SGD over flat buckets, and the two C-ABI entry points of the fused SGD step."""
import os
import re
import types

import pytest
import torch

from hupr_amd.tools.optim import FusedAdam, FusedSGD, make_optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SGD_ENTRIES = ("hupr_sgd_step_f32", "hupr_sgd_step_dev_f32")


def _cfg(name):
    return types.SimpleNamespace(TRAINING=types.SimpleNamespace(optimizer=name))


def _group(opt):
    return {k: v for k, v in opt.param_groups[0].items() if k != "params"}


def test_make_optimizer_follows_training_optimizer():
    net = torch.nn.Linear(4, 3)
    sgd = make_optimizer(_cfg("sgd"), net.parameters(), 2e-3)
    assert type(sgd) is FusedSGD
    ref = torch.optim.SGD(net.parameters(), lr=2e-3, momentum=0.9, weight_decay=1e-4)
    assert _group(sgd) == _group(ref)
    adam = make_optimizer(_cfg("adam"), net.parameters(), 2e-3)
    assert type(adam) is FusedAdam
    assert _group(adam) == dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, amsgrad=False, maximize=False,
                                foreach=None, capturable=False, differentiable=False, fused=None)
    with pytest.raises(ValueError, match="'sgd' or 'adam'"):
        make_optimizer(_cfg("rmsprop"), net.parameters(), 2e-3)


@pytest.mark.parametrize("kw", [dict(momentum=0.0), dict(dampening=0.1), dict(nesterov=True), dict(maximize=True)])
def test_fused_sgd_refuses_unsupported_settings(kw):
    net = torch.nn.Linear(4, 3)
    with pytest.raises(ValueError, match="dampening=0, nesterov=False, maximize=False"):
        FusedSGD(net.parameters(), lr=1e-3, weight_decay=1e-4, **kw)


def test_fused_sgd_refuses_an_unsupported_torch_sgd_checkpoint():
    net = torch.nn.Linear(4, 3)
    opt = FusedSGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    sd = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, nesterov=True).state_dict()
    with pytest.raises(ValueError, match="nesterov=False"):
        opt.load_state_dict(sd)
    assert opt.param_groups[0]["nesterov"] is False


def test_fused_sgd_checkpoint_interchanges_with_torch_sgd():
    """Mirror of the FusedAdam interchange test: the flat-bucket momentum buffers round-trip through torch.optim.SGD's
    per-parameter state_dict layout ({"momentum_buffer": tensor}; reference tools/base.py:76-81 saves it, :113 restores it)."""
    from hupr_amd.tools.distributed import GradientBuckets
    torch.manual_seed(13)

    def make():
        return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 4), torch.nn.Linear(4, 2))
    net = make()
    gb = GradientBuckets(net, bucket_bytes=256, tail_bytes=0)
    assert len(gb.buckets) >= 2
    opt = FusedSGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    opt.attach_flat_buckets(gb.flat_pairs(), gb.layout())
    assert opt.state_dict()["state"] == {}                      # nothing before the first step, like torch
    for st in opt._flat_state:                                  # as if 3 steps had run
        st["step"] = 3
        st["momentum_buffer"].normal_()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(6)) and sd["param_groups"][0]["params"] == list(range(6))
    assert all(set(s) == {"momentum_buffer"} for s in sd["state"].values())
    # (a) a torch.optim.SGD over the same parameters accepts it and sees the right slices
    tsgd = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    tsgd.load_state_dict(sd)
    for i, entries in enumerate(gb.layout()):
        for p, off, n in entries:
            assert torch.equal(tsgd.state[p]["momentum_buffer"].reshape(-1), opt._flat_state[i]["momentum_buffer"][off:off + n])
    # (b) a fresh FusedSGD restores the flat buffers from torch's state_dict, bit for bit
    net2 = make()
    gb2 = GradientBuckets(net2, bucket_bytes=256, tail_bytes=0)
    opt2 = FusedSGD(net2.parameters(), lr=5e-4, momentum=0.9, weight_decay=1e-4)
    opt2.attach_flat_buckets(gb2.flat_pairs(), gb2.layout())
    opt2.load_state_dict(tsgd.state_dict())
    assert opt2.param_groups[0]["lr"] == 1e-3 and len(opt2.state) == 0
    for a, b in zip(opt._flat_state, opt2._flat_state):
        assert b["step"] >= 1 and torch.equal(a["momentum_buffer"], b["momentum_buffer"])
    # (c) a parameter without a saved entry keeps a zero slice
    tsd = tsgd.state_dict()
    del tsd["state"][5]
    opt3 = FusedSGD(net2.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    opt3.attach_flat_buckets(gb2.flat_pairs(), gb2.layout())
    opt3._flat_state[-1]["momentum_buffer"].fill_(7.0)
    opt3.load_state_dict(tsd)
    p5 = list(net2.parameters())[5]
    for i, entries in enumerate(gb2.layout()):
        for p, off, n in entries:
            got = opt3._flat_state[i]["momentum_buffer"][off:off + n]
            if p is p5:
                assert torch.equal(got, torch.zeros(n))
            else:
                assert torch.equal(got, opt._flat_state[i]["momentum_buffer"][off:off + n])
    # (d) an Adam checkpoint (flat-bucket FusedAdam or torch.optim.Adam) is refused and named
    adam = FusedAdam(net.parameters(), lr=1e-3, weight_decay=1e-4)
    adam.attach_flat_buckets(gb.flat_pairs(), gb.layout())
    for st in adam._flat_state:
        st["step"] = 2
    opt4 = FusedSGD(net2.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    opt4.attach_flat_buckets(gb2.flat_pairs(), gb2.layout())
    with pytest.raises(ValueError, match="Adam"):
        opt4.load_state_dict(adam.state_dict())
    assert all(st["step"] == 0 for st in opt4._flat_state)


def _torch14_sgd_state(params, seed=17):
    """optimizer_state_dict as the reference's torch 1.4 (environment.yml) saves optim.SGD(momentum=0.9, weight_decay=1e-4):
    param_groups hold only lr, momentum, dampening, weight_decay, nesterov and params; one momentum buffer per parameter."""
    g = torch.Generator().manual_seed(seed)
    return {"state": {i: {"momentum_buffer": torch.randn(p.shape, generator=g)} for i, p in enumerate(params)},
            "param_groups": [{"lr": 3e-4, "momentum": 0.9, "dampening": 0, "weight_decay": 1e-4, "nesterov": False,
                              "params": list(range(len(params)))}]}


def test_fused_sgd_resumes_a_torch14_reference_checkpoint():
    """A reference SGD run's checkpoint (torch 1.4 group keys) loads with flat buckets and without: the later group keys are
    filled in as torch.optim.SGD.__setstate__ does, the buffers land bit for bit, and the caller's dict is left as it was."""
    from hupr_amd.tools.distributed import GradientBuckets

    def make():
        torch.manual_seed(19)
        return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 4), torch.nn.Linear(4, 2))
    old = _torch14_sgd_state(list(make().parameters()))
    old_keys = set(old["param_groups"][0])
    tsgd = torch.optim.SGD(make().parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    tsgd.load_state_dict(old)                            # torch itself accepts it
    # (a) flat buckets, as TrainEngine runs it
    net = make()
    gb = GradientBuckets(net, bucket_bytes=256, tail_bytes=0)
    assert len(gb.buckets) >= 2
    opt = FusedSGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    opt.attach_flat_buckets(gb.flat_pairs(), gb.layout())
    opt.load_state_dict(old)
    index = {id(p): i for i, p in enumerate(net.parameters())}
    for i, entries in enumerate(gb.layout()):
        assert opt._flat_state[i]["step"] == 1
        for p, off, n in entries:
            assert torch.equal(opt._flat_state[i]["momentum_buffer"][off:off + n],
                               old["state"][index[id(p)]]["momentum_buffer"].reshape(-1))
    assert set(opt.param_groups[0]) == set(tsgd.param_groups[0]) and opt.param_groups[0]["lr"] == 3e-4
    assert {k: v for k, v in _group(opt).items() if k in old_keys} == {k: v for k, v in old["param_groups"][0].items()
                                                                       if k != "params"}
    sd = opt.state_dict()                                # and writes it back in torch's layout
    for i, entry in old["state"].items():
        assert torch.equal(sd["state"][i]["momentum_buffer"], entry["momentum_buffer"])
    # (b) the per-parameter path
    net2 = make()
    opt2 = FusedSGD(net2.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    opt2.load_state_dict(old)
    for i, p in enumerate(net2.parameters()):
        assert torch.equal(opt2.state[p]["momentum_buffer"], old["state"][i]["momentum_buffer"])
    assert set(opt2.param_groups[0]) == set(tsgd.param_groups[0])
    assert set(old["param_groups"][0]) == old_keys
    # a torch 1.4 checkpoint of an unsupported SGD is still refused with the supported settings named
    bad = dict(old, param_groups=[dict(old["param_groups"][0], nesterov=True)])
    with pytest.raises(ValueError, match="nesterov=False"):
        FusedSGD(make().parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4).load_state_dict(bad)


def test_sgd_entry_points_are_declared_and_bound():
    from hupr_amd import runtime
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hupr.h")).read(), flags=re.S)
    for name in SGD_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in runtime.SIGNATURES, name
