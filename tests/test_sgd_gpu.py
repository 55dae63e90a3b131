"""GPU (-m gpu): TRAINING.optimizer = sgd — the fused SGD-momentum step (hupr_sgd_step_f32 / hupr_sgd_step_dev_f32) against
torch.optim.SGD and a float64 restatement, then the engine, graph capture, checkpoint resume, the collective and main.py with it.

The reference's optimiser: optim.SGD(lr, momentum=0.9, weight_decay=1e-4) (tools/base.py:44-45), dampening 0, no Nesterov."""
import copy
import json
import os

import pytest
import torch
import yaml

from hupr_amd import synth

pytestmark = pytest.mark.gpu
LR, MOM, WD = 1e-2, 0.9, 1e-4


def close(got, ref, tol, what=""):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-30
    assert err <= tol * scale, "%s: max err %.3e vs scale %.3e (rel %.3e)" % (what, err, scale, err / scale)


def _rnd(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _sgd(p, g, buf, lr, first, gscale=1.0):
    from hupr_amd import runtime as rt
    rt.check(rt.lib().hupr_sgd_step_f32(rt.ptr(p), rt.ptr(g), rt.ptr(buf), p.numel(), lr, MOM, WD, int(first), gscale,
                                        rt.stream()))


# ---- the kernel through the C ABI ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 10007, (1 << 20) + 3])
def test_sgd_step_matches_torch_and_fp64(n):
    """5 steps with a new gradient each step: parameters and momentum buffers agree with torch.optim.SGD on the GPU and with
    a float64 restatement of d = g + wd p, buf = d (step 1) | m buf + d, p -= lr buf."""
    p0 = _rnd(n, 1)
    pd, buf = p0.cuda(), torch.empty(n, device="cuda")
    pt = p0.cuda().requires_grad_(True)
    opt = torch.optim.SGD([pt], lr=LR, momentum=MOM, weight_decay=WD)
    p64, b64 = p0.double(), None
    for step in range(1, 6):
        g = _rnd(n, 100 + step)
        pt.grad = g.cuda()
        opt.step()
        _sgd(pd, g.cuda(), buf, LR, step == 1)
        d64 = g.double() + WD * p64
        b64 = d64 if b64 is None else MOM * b64 + d64
        p64 = p64 - LR * b64
    torch.cuda.synchronize()
    close(pd, pt, 1e-6, "p vs torch")
    close(buf, opt.state[pt]["momentum_buffer"], 1e-6, "buf vs torch")
    close(pd, p64, 1e-6, "p vs fp64")
    close(buf, b64, 1e-6, "buf vs fp64")


@pytest.mark.parametrize("shifted", ["all", "buf"])
@pytest.mark.parametrize("n", [5, 10007, (1 << 20) + 3])
def test_unaligned_launch_equals_aligned_launch(n, shifted):
    """The same data at element offset 1 of larger buffers (the scalar path: not every stream is 16-byte aligned) gives exactly
    the aligned (float4) launch's results; the canary elements around the slice stay untouched."""
    canary = -12345.5
    p0, b0 = _rnd(n, 3), _rnd(n, 4)
    grads = [_rnd(n, 10 + s).cuda() for s in range(3)]
    pa, ba = p0.cuda(), b0.cuda()
    big = {k: torch.full((n + 8,), canary, device="cuda") for k in ("p", "g", "buf")}
    off = {k: 1 if shifted == "all" or k == shifted else 0 for k in big}
    view = {k: big[k][off[k]:off[k] + n] for k in big}
    view["p"].copy_(p0)
    view["buf"].copy_(b0)
    assert view["buf"].data_ptr() % 16 == 4 and (shifted == "buf" or view["p"].data_ptr() % 16 == 4)
    for s, g in enumerate(grads):
        _sgd(pa, g, ba, LR, s == 0)
        view["g"].copy_(g)
        _sgd(view["p"], view["g"], view["buf"], LR, s == 0)
    torch.cuda.synchronize()
    assert torch.equal(view["p"], pa) and torch.equal(view["buf"], ba)
    for k, t in big.items():
        outside = torch.cat([t[:off[k]], t[off[k] + n:]])
        assert bool((outside == canary).all()), k


def test_device_lr_entry_equals_host_lr_entry():
    """hupr_sgd_step_dev_f32 reads {lr, step} from device memory (the layout hupr_adam_step_dev_f32 uses; step 1 is the first
    step): bit for bit the host-argument entry over 4 steps, with the learning rate halved after step 2."""
    from hupr_amd import runtime as rt
    n = 10007
    ph, pd = _rnd(n, 5).cuda(), _rnd(n, 5).cuda()
    bh, bd = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    lr = LR
    state = torch.zeros(2, device="cuda")
    for step in range(1, 5):
        if step == 3:
            lr = LR / 2
        g = _rnd(n, 20 + step).cuda()
        _sgd(ph, g, bh, lr, step == 1)
        state.copy_(torch.tensor([lr, float(step)]))
        rt.check(rt.lib().hupr_sgd_step_dev_f32(rt.ptr(pd), rt.ptr(g), rt.ptr(bd), n, rt.ptr(state), MOM, WD, 1.0, rt.stream()))
    torch.cuda.synchronize()
    assert torch.equal(ph, pd) and torch.equal(bh, bd)


def test_gradient_scale_equals_prescaled_gradient():
    n = 10007
    p1, p2 = _rnd(n, 6).cuda(), _rnd(n, 6).cuda()
    b1, b2 = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    for step in range(1, 4):
        g = _rnd(n, 30 + step).cuda()
        _sgd(p1, g, b1, LR, step == 1, gscale=0.5)
        _sgd(p2, g * 0.5, b2, LR, step == 1)
    torch.cuda.synchronize()
    assert torch.equal(p1, p2) and torch.equal(b1, b2)


def test_sgd_entries_refuse_bad_arguments_before_any_launch():
    from hupr_amd import runtime as rt
    L = rt.lib()
    t = torch.zeros(16, device="cuda")
    a = rt.ptr(t)
    before = L.hupr_launch_count()
    host = [(None, a, a, 16), (a, None, a, 16), (a, a, None, 16), (a, a, a, 0), (a, a, a, -4)]
    for p, g, b, n in host:
        assert L.hupr_sgd_step_f32(p, g, b, n, LR, MOM, WD, 1, 1.0, rt.stream()) == -1
        assert b"hupr_sgd_step_f32" in L.hupr_last_error()
    for p, g, b, n, st in [args + (a,) for args in host] + [(a, a, a, 16, None)]:
        assert L.hupr_sgd_step_dev_f32(p, g, b, n, st, MOM, WD, 1.0, rt.stream()) == -1
        assert b"hupr_sgd_step_dev_f32" in L.hupr_last_error()
    assert L.hupr_launch_count() == before
    assert bool((t == 0).all())


def test_per_parameter_path_matches_torch_sgd():
    """Without flat buckets: one launch per parameter tensor; a parameter whose gradient is None is skipped (no state, no
    change), as torch.optim.SGD skips it; parameters and state_dict follow torch.optim.SGD step for step."""
    from hupr_amd.tools.optim import FusedSGD
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.Linear(17, 5)).cuda()
    ref = copy.deepcopy(net)
    frozen0 = net[1].bias.detach().clone()
    opt = FusedSGD(net.parameters(), lr=LR, momentum=MOM, weight_decay=WD)
    topt = torch.optim.SGD(ref.parameters(), lr=LR, momentum=MOM, weight_decay=WD)
    for _ in range(4):
        x = torch.randn(8, 33, device="cuda")
        for m, o in ((net, opt), (ref, topt)):
            o.zero_grad(set_to_none=True)
            m(x).square().sum().backward()
            m[1].bias.grad = None
            o.step()
    torch.cuda.synchronize()
    for a, b in zip(net.parameters(), ref.parameters()):
        close(a, b, 1e-6, "parameters")
    assert torch.equal(net[1].bias, frozen0) and net[1].bias not in opt.state
    sd, tsd = opt.state_dict(), topt.state_dict()
    assert sorted(sd["state"]) == sorted(tsd["state"]) == [0, 1, 2]
    for i in sd["state"]:
        close(sd["state"][i]["momentum_buffer"], tsd["state"][i]["momentum_buffer"], 1e-6, "buffer %d" % i)


# ---- the engine with TRAINING.optimizer = sgd (bf16, B = 4 synthetic cubes) -------------------------------------------
def _setup(B=4, seed=51):
    from hupr_amd.config_tree import load_config
    cfg = load_config()
    cfg.TRAINING.optimizer = "sgd"
    dev = torch.device("cuda", 0)
    G = cfg.DATASET.numGroupFrames
    adc_h = torch.from_numpy(synth.adc_cube_int16(seed, sensor=0, nframes=B * G)).to(dev)
    adc_v = torch.from_numpy(synth.adc_cube_int16(seed, sensor=1, nframes=B * G)).to(dev)
    joints = torch.from_numpy(synth.keypoints(B, seed + 1)).to(dev)
    return cfg, dev, adc_h, adc_v, joints


def _flat(eng):
    return torch.cat([p.detach().flatten() for p in eng.model.parameters()])


@pytest.fixture
def bf16():
    from hupr_amd import functional as F_
    F_.set_math("bf16")
    yield F_
    F_.set_math("f32")


def test_engine_first_sgd_step(bf16):
    """One step: every bucket's buffer is grad * gscale + 1e-4 p_before, the parameters p_before - lr buf."""
    from hupr_amd.tools.engine import TrainEngine
    from hupr_amd.tools.optim import FusedSGD
    cfg, dev, adc_h, adc_v, joints = _setup(seed=91)
    eng = TrainEngine(cfg, device=dev, seed=0)
    opt = eng.optimizer
    assert type(opt) is FusedSGD and opt.param_groups[0]["momentum"] == MOM and opt.param_groups[0]["weight_decay"] == WD
    lr = opt.param_groups[0]["lr"]
    before = [p.clone() for p, _ in opt._flat]
    eng.train_step_from_adc(adc_h, adc_v, joints)
    torch.cuda.synchronize()
    for (p, g), st, p0 in zip(opt._flat, opt._flat_state, before):
        buf = st["momentum_buffer"]
        assert st["step"] == 1
        close(buf, g.double() * opt.grad_scale + WD * p0.double(), 1e-6, "buffer")
        close(p, p0.double() - lr * buf.double(), 1e-6, "parameters")
        assert not torch.equal(p, p0)


def test_engine_sgd_loss_falls(bf16):
    """Ten SGD steps on one fixed batch at lr = 1e-2 (the YAML's 1e-4 moves the loss too little in ten steps)."""
    from hupr_amd.tools.engine import TrainEngine
    cfg, dev, adc_h, adc_v, joints = _setup(seed=93)
    eng = TrainEngine(cfg, device=dev, seed=0, lr=1e-2)
    losses = [float(eng.train_step_from_adc(adc_h, adc_v, joints)[0]) for _ in range(10)]
    assert losses[-1] < losses[0], losses
    assert bool(torch.isfinite(_flat(eng)).all())


def test_engine_sgd_graph_replay_equals_eager_steps(bf16):
    """5 eager steps == 2 eager + capture (1 warm-up) + 2 replays, bit for bit, with the learning rate halved after step 3
    (sync_lr on the graph side).  SGD has no bias correction: nothing is evaluated differently on the device."""
    from hupr_amd.tools.engine import TrainEngine
    cfg, dev, adc_h, adc_v, joints = _setup(seed=95)

    def halve(eng):
        for group in eng.optimizer.param_groups:
            group["lr"] *= 0.5
    e1 = TrainEngine(cfg, device=dev, seed=0)
    for s in range(5):
        if s == 3:
            halve(e1)
        e1.train_step_from_adc(adc_h, adc_v, joints)
    e2 = TrainEngine(cfg, device=dev, seed=0)
    for _ in range(2):
        e2.train_step_from_adc(adc_h, adc_v, joints)
    e2.capture(adc_h, adc_v, joints, warmup=1)
    halve(e2)
    e2.sync_lr()
    for _ in range(2):
        e2.train_step_from_adc(adc_h, adc_v, joints)
    torch.cuda.synchronize()
    assert e2.optimizer._host_step(0) == 5
    assert torch.equal(_flat(e1), _flat(e2))


def test_engine_sgd_checkpoint_resume_is_bit_exact(tmp_path, bf16):
    """2 steps -> save -> a fresh engine (another seed) loads -> step 3 lands on the bits of the uninterrupted run, also from the
    checkpoint with torch 1.4 group keys; the saved state has torch.optim.SGD's layout and drives torch.optim.SGD."""
    from hupr_amd.tools.engine import TrainEngine
    cfg, dev, adc_h, adc_v, joints = _setup(seed=97)
    e1 = TrainEngine(cfg, device=dev, seed=0)
    for _ in range(2):
        e1.train_step_from_adc(adc_h, adc_v, joints)
    ck = {"model_state_dict": e1.model.state_dict(), "optimizer_state_dict": e1.optimizer.state_dict()}
    torch.save(ck, tmp_path / "checkpoint.pth")
    e1.train_step_from_adc(adc_h, adc_v, joints)
    n_params = sum(1 for _ in e1.model.parameters())
    ck = torch.load(tmp_path / "checkpoint.pth", map_location="cuda")
    st = ck["optimizer_state_dict"]["state"]
    assert len(st) == n_params and all(set(s) == {"momentum_buffer"} and s["momentum_buffer"].abs().sum() > 0 for s in st.values())
    e2 = TrainEngine(cfg, device=dev, seed=123)              # different init on purpose
    e2.model.load_state_dict(ck["model_state_dict"])
    e2.optimizer.load_state_dict(ck["optimizer_state_dict"])
    bf16.invalidate_packed()
    e2.train_step_from_adc(adc_h, adc_v, joints)
    torch.cuda.synchronize()
    assert torch.equal(_flat(e1), _flat(e2))
    # the same checkpoint with a torch 1.4 reference run's group keys (lr, momentum, dampening, weight_decay, nesterov) resumes
    # to the same bits
    osd = ck["optimizer_state_dict"]
    old_keys = ("lr", "momentum", "dampening", "weight_decay", "nesterov", "params")
    osd14 = {"state": osd["state"], "param_groups": [{k: g[k] for k in old_keys} for g in osd["param_groups"]]}
    e3 = TrainEngine(cfg, device=dev, seed=321)
    e3.model.load_state_dict(ck["model_state_dict"])
    e3.optimizer.load_state_dict(osd14)
    bf16.invalidate_packed()
    e3.train_step_from_adc(adc_h, adc_v, joints)
    torch.cuda.synchronize()
    assert torch.equal(_flat(e1), _flat(e3))
    tsgd = torch.optim.SGD(e2.model.parameters(), lr=cfg.TRAINING.lr, momentum=MOM, weight_decay=WD)
    tsgd.load_state_dict(ck["optimizer_state_dict"])
    assert len(tsgd.state) == n_params


def test_engine_sgd_rccl_exchange_single_rank_is_bit_transparent(monkeypatch, bf16):
    """HUPR_FORCE_ALLREDUCE=1 (every bucket through hupr_allreduce_bucket on a single-rank communicator): 3 SGD steps ==
    3 steps without any collective, bit for bit."""
    from hupr_amd.tools.engine import TrainEngine
    saved = bf16.TWO_STREAMS
    try:
        bf16.TWO_STREAMS = False
        cfg, dev, adc_h, adc_v, joints = _setup(seed=99)
        monkeypatch.delenv("HUPR_FORCE_ALLREDUCE", raising=False)
        e0 = TrainEngine(cfg, device=dev, seed=0)
        assert not e0.buckets.active
        monkeypatch.setenv("HUPR_FORCE_ALLREDUCE", "1")
        e1 = TrainEngine(cfg, device=dev, seed=0)
        assert e1.buckets.active and e1.buckets.transport.name.startswith("rccl"), e1.buckets.transport.name
        for _ in range(3):
            l0, _ = e0.train_step_from_adc(adc_h, adc_v, joints)
            l1, _ = e1.train_step_from_adc(adc_h, adc_v, joints)
        torch.cuda.synchronize()
        assert float(l0) == float(l1)
        assert torch.equal(_flat(e0), _flat(e1))
        for a, b in zip(e0.optimizer._flat_state, e1.optimizer._flat_state):
            assert torch.equal(a["momentum_buffer"], b["momentum_buffer"])
        e1.buckets.transport.close()
    finally:
        bf16.TWO_STREAMS = saved


def test_main_train_then_eval_with_sgd(tmp_path, monkeypatch):
    """main.py with TRAINING.optimizer: sgd — the checkpoint holds torch.optim.SGD's state, a second training run resumes
    from it, and --eval reloads the weights."""
    from hupr_amd import main as hmain
    from hupr_amd.config_tree import CONFIG_DIR
    cfgd = yaml.safe_load(open(os.path.join(CONFIG_DIR, "mscsa_prgcn.yaml")))
    cfgd["DATASET"]["dataDir"] = "synthetic"
    cfgd["TRAINING"]["batchSize"] = 2
    cfgd["TRAINING"]["epochs"] = 1
    cfgd["TRAINING"]["optimizer"] = "sgd"
    cfgd["TEST"]["batchSize"] = 2
    (tmp_path / "config").mkdir()
    yaml.safe_dump(cfgd, open(tmp_path / "config" / "tiny.yaml", "w"))
    (tmp_path / "logs").mkdir()
    (tmp_path / "visualization").mkdir()
    monkeypatch.chdir(tmp_path)
    hmain.main(["--config", "tiny.yaml", "--dir", "run0", "--synthetic_length", "4", "--max_steps", "2"])
    run = tmp_path / "logs" / "run0"
    ck = torch.load(run / "checkpoint.pth")
    osd = ck["optimizer_state_dict"]
    assert osd["param_groups"][0]["momentum"] == 0.9 and osd["param_groups"][0]["weight_decay"] == 1e-4
    assert len(osd["state"]) == len(osd["param_groups"][0]["params"])
    assert all(set(s) == {"momentum_buffer"} for s in osd["state"].values())
    hmain.main(["--config", "tiny.yaml", "--dir", "run0", "--synthetic_length", "4", "--max_steps", "1"])   # resumes
    osd2 = torch.load(run / "checkpoint.pth")["optimizer_state_dict"]
    assert len(osd2["state"]) == len(osd["state"]) and all(set(s) == {"momentum_buffer"} for s in osd2["state"].values())
    hmain.main(["--config", "tiny.yaml", "--dir", "run0", "--synthetic_length", "4", "--eval"])
    assert len(json.load(open(run / "test_results.json"))) == 4
