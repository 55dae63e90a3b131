"""CPU (-m "not gpu"): TRAINING.gradClip — the five C-ABI entries of the gradient guard are declared, exported and bound, the
key's values map to off / a max norm / guard only, and the guard refuses an optimiser without flat buckets."""
import ctypes
import os
import re
import types

import pytest
import torch
import yaml

from hupr_amd.tools.optim import FusedAdam, FusedSGD, make_optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD_ENTRIES = ("hupr_grad_sumsq_partials", "hupr_grad_sumsq_f32", "hupr_grad_guard_f32", "hupr_adam_step_guard_f32",
                 "hupr_sgd_step_guard_f32")
ABSENT = object()


def _cfg(clip=ABSENT, name="adam"):
    training = types.SimpleNamespace(optimizer=name)
    if clip is not ABSENT:
        training.gradClip = clip
    return types.SimpleNamespace(TRAINING=training)


def test_guard_entry_points_are_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hupr.h")).read(), flags=re.S)
    lib = ctypes.CDLL(runtime.LIB_PATH)
    for name in GUARD_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
        assert name in runtime.SIGNATURES, name
    # the guarded steps are the _dev entries plus one pointer (the guard) behind dev_state
    for opt in ("adam", "sgd"):
        dev = runtime.SIGNATURES["hupr_%s_step_dev_f32" % opt][1]
        grd = runtime.SIGNATURES["hupr_%s_step_guard_f32" % opt][1]
        at = max(i for i, a in enumerate(dev[:-1]) if a is ctypes.c_void_p)        # dev_state
        assert grd == dev[:at + 1] + [ctypes.c_void_p] + dev[at + 1:]
    n = runtime.lib().hupr_grad_sumsq_partials()
    assert n >= 64 and n % 64 == 0


def test_guard_entries_refuse_null_pointers_without_a_gpu():
    """Argument errors are found on the host, before any launch: -1 and a message that names the entry."""
    from hupr_amd import runtime as rt
    L = rt.lib()
    before = L.hupr_launch_count()
    assert L.hupr_grad_sumsq_f32(None, 16, None, None) == -1 and b"hupr_grad_sumsq_f32" in L.hupr_last_error()
    assert L.hupr_grad_guard_f32(None, 4, 1.0, 1.0, None, None, None) == -1 and b"hupr_grad_guard_f32" in L.hupr_last_error()
    assert L.hupr_adam_step_guard_f32(None, None, None, None, 16, None, None, 0.9, 0.999, 1e-8, 1e-4, 1.0, None) == -1
    assert b"hupr_adam_step_guard_f32" in L.hupr_last_error()
    assert L.hupr_sgd_step_guard_f32(None, None, None, 16, None, None, 0.9, 1e-4, 1.0, None) == -1
    assert b"hupr_sgd_step_guard_f32" in L.hupr_last_error()
    assert L.hupr_launch_count() == before


@pytest.mark.parametrize("name, cls", [("adam", FusedAdam), ("sgd", FusedSGD)])
def test_make_optimizer_reads_grad_clip(name, cls):
    net = torch.nn.Linear(4, 3)
    for clip, want in [(ABSENT, None), (-1, None), (-1.0, None), (1.0, 1.0), (5, 5.0), (float("inf"), float("inf"))]:
        opt = make_optimizer(_cfg(clip, name), net.parameters(), 1e-3)
        assert type(opt) is cls and opt.grad_clip == want, (clip, opt.grad_clip)
        assert want is None or type(opt.grad_clip) is float
        assert opt._guard is None                              # enabled by the engine, once the buckets are attached


def test_yaml_inf_means_guard_only():
    cfgd = yaml.safe_load("TRAINING:\n  optimizer: adam\n  gradClip: .inf\n")
    from hupr_amd.config_tree import obj
    opt = make_optimizer(obj(cfgd), torch.nn.Linear(4, 3).parameters(), 1e-3)
    assert opt.grad_clip == float("inf")


@pytest.mark.parametrize("bad", [0, 0.0, -2, -0.5, float("nan"), float("-inf"), "1.0", True, None])
def test_make_optimizer_refuses_other_grad_clip_values(bad):
    with pytest.raises(ValueError, match="TRAINING.gradClip"):
        make_optimizer(_cfg(bad), torch.nn.Linear(4, 3).parameters(), 1e-3)


def test_shipped_yaml_does_not_carry_the_key():
    """The YAML's parsed content is pinned against the reference: the key is opt-in, the default configuration trains as before."""
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    assert not hasattr(cfg.TRAINING, "gradClip")
    assert make_optimizer(cfg, torch.nn.Linear(4, 3).parameters(), 1e-3).grad_clip is None


@pytest.mark.parametrize("cls", [FusedAdam, FusedSGD])
def test_enable_grad_guard_needs_flat_buckets(cls):
    opt = cls(torch.nn.Linear(4, 3).parameters(), lr=1e-3, weight_decay=1e-4)
    with pytest.raises(RuntimeError, match="flat gradient buckets"):
        opt.enable_grad_guard(1.0)
    assert opt.guard_stats() is None


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan")])
def test_enable_grad_guard_refuses_a_non_positive_max_norm(bad):
    from hupr_amd.tools.distributed import GradientBuckets
    net = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 4))
    gb = GradientBuckets(net, bucket_bytes=256, tail_bytes=0)
    opt = FusedSGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    opt.attach_flat_buckets(gb.flat_pairs(), gb.layout())
    with pytest.raises(ValueError, match="max_norm"):
        opt.enable_grad_guard(bad)
    assert opt._guard is None and opt._dev_state is None


def test_enable_grad_guard_allocates_once_and_keeps_checkpoint_interchange():
    """Host-side bookkeeping (no launch): one partial vector slice per bucket, a zeroed 4-float guard, {lr, step} in tensor form
    carrying the restored step count; state_dict() reads the count from there."""
    from hupr_amd import runtime as rt
    from hupr_amd.tools.distributed import GradientBuckets
    net = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 4), torch.nn.Linear(4, 2))
    gb = GradientBuckets(net, bucket_bytes=256, tail_bytes=0)
    assert len(gb.buckets) >= 2
    opt = FusedAdam(net.parameters(), lr=2e-3, weight_decay=1e-4)
    opt.attach_flat_buckets(gb.flat_pairs(), gb.layout())
    for st in opt._flat_state:
        st["step"] = 7
    opt.enable_grad_guard(float("inf"))
    k = rt.lib().hupr_grad_sumsq_partials()
    assert opt._guard_partials.dtype == torch.float64 and opt._guard_partials.numel() == k * len(gb.buckets)
    assert opt._guard.tolist() == [0.0, 0.0, 0.0, 0.0] and opt._dev_state.tolist() == [pytest.approx(2e-3), 7.0]
    assert opt.guard_stats() == {"norm": 0.0, "coef": 0.0, "skipped": 0}
    partials, guard, state = opt._guard_partials, opt._guard, opt._dev_state
    opt.enable_grad_guard(2.0)                                   # again: same buffers (a captured graph keeps their addresses)
    assert opt._guard_partials is partials and opt._guard is guard and opt._dev_state is state and opt._guard_max_norm == 2.0
    opt._dev_state[1] = 9.0                                      # as the guard kernel advances it
    sd = opt.state_dict()
    assert all(float(s["step"]) == 9.0 for s in sd["state"].values())
    opt2 = FusedAdam(net.parameters(), lr=1e-3, weight_decay=1e-4)
    opt2.attach_flat_buckets(gb.flat_pairs(), gb.layout())
    opt2.enable_grad_guard(1.0)
    opt2.load_state_dict(sd)
    assert opt2._dev_state.tolist() == [pytest.approx(2e-3), 9.0] and opt2._host_step(0) == 9
