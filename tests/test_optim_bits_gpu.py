"""GPU (-m gpu): the optimiser family bit for bit against a recorded run — Adam and SGD in their three forms, the gradient guard
(hupr_grad_sumsq_f32, hupr_grad_guard_f32) and the weight average (hupr_ema_tick_f32, hupr_ema_update_f32, hupr_swap_f32), driven
through the C ABI only and compared as SHA-256 digests of the output bytes with tests/golden/optim_bits.json.

The fixture is this module's own record (``python tests/test_optim_bits_gpu.py --record`` on the GPU), taken before the kernels
were gathered into csrc/optim.hip.  A digest that moves means a kernel changed which thread touches which element or an order of
operations: fix the kernel, do not record again.  The inputs come from a seeded CPU generator and are uploaded.  Every digest is
taken over the whole allocation, canaries around the array included, so a store beside an array moves it too.

Sizes: 1 (the scalar head alone), 7 (head and tail, no float4 round), 4099 (one partial round of the unrolled loops), 2^20 + 3,
and 2^23 + 2^21 + 5, which lies beyond every grid cap of the family (Adam and SGD 2.1 M elements, the square sum's unrolled loop
4.2 M, the average's 2048 workgroups 8.4 M), so every grid-stride loop goes round more than once.  Offsets: every array at element
0, 1 and 3 of a 256-byte-aligned allocation, and one set of different offsets (the 4-byte launches of the average and the swap,
SGD's path without float4)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "optim_bits.json")

pytestmark = pytest.mark.gpu
SIZES = [1, 7, 4099, (1 << 20) + 3, (1 << 23) + (1 << 21) + 5]
OFFSETS = [(0, 0, 0, 0), (1, 1, 1, 1), (3, 3, 3, 3), (0, 1, 3, 2)]       # per entry: its arrays in argument order
PAD = 8
CANARY = -12345.5
INF = float("inf")
LR, B1, B2, EPS, WD, MOM, GSCALE, DECAY = 1e-3, 0.9, 0.999, 1e-8, 1e-4, 0.9, 1.0 / 3.0, 0.999


def _lib():
    from hupr_amd import runtime as rt
    return rt, rt.lib()


_POOLS = None


def pools():
    """Two seeded CPU normal vectors (start values; gradients, step k reads [k, k + n)) and their uploads, made once."""
    global _POOLS
    if _POOLS is None:
        gen = torch.Generator().manual_seed(20261019)
        a = torch.randn(SIZES[-1] + PAD, generator=gen)
        b = torch.randn(SIZES[-1] + PAD, generator=gen)
        _POOLS = (a.cuda(), b.cuda(), b.numpy())
    return _POOLS


def _place(n, off, src=None):
    """n elements at element offset ``off`` of a 256-byte-aligned allocation filled with the canary -> (allocation, view)."""
    big = torch.full((n + PAD,), CANARY, device="cuda")
    assert big.data_ptr() % 256 == 0
    view = big[off:off + n]
    if src is None:
        view.zero_()
    else:
        view.copy_(src)
    return big, view


def _digest(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy())
    return h.hexdigest()


def _half_norm(g):
    """A max_norm below the step's gradient norm, so that the guard clips: half of gscale * |g|, from the CPU copy in fp64."""
    return float(np.float32(0.5 * GSCALE * np.sqrt(np.sum(np.square(g.astype(np.float64))))))


def _optimizer(kind, form, n, offs):
    """Three consecutive steps from zero state.  host: the step count / first flag as arguments; dev: {lr, step} on the device;
    guard: step 1 unclipped (max_norm = inf), step 2 clipped, step 3 with one inf among the gradients (nothing moves)."""
    rt, L = _lib()
    s = rt.stream()
    A, B, Bcpu = pools()
    K = L.hupr_grad_sumsq_partials()
    assert K == 1024
    P, p = _place(n, offs[0], A[:n])
    _, g = _place(n, offs[1])
    bufs = [_place(n, offs[2 + i]) for i in range(2 if kind == "adam" else 1)]
    st = [rt.ptr(v) for _, v in bufs]
    dev = torch.tensor([LR, 0.0], device="cuda")
    guard = torch.zeros(4, device="cuda")
    partials = torch.zeros(K, dtype=torch.float64, device="cuda")
    steps, decisions = [], []
    for k in (1, 2, 3):
        g.copy_(B[k:k + n])
        if form == "guard":
            max_norm = INF if k == 1 else _half_norm(Bcpu[2:2 + n])
            if k == 3:
                g[n // 2] = INF
            rt.check(L.hupr_grad_sumsq_f32(rt.ptr(g), n, rt.ptr(partials), s))
            rt.check(L.hupr_grad_guard_f32(rt.ptr(partials), K, GSCALE, max_norm, rt.ptr(dev), rt.ptr(guard), s))
            if kind == "adam":
                rt.check(L.hupr_adam_step_guard_f32(rt.ptr(p), rt.ptr(g), *st, n, rt.ptr(dev), rt.ptr(guard), B1, B2, EPS, WD, GSCALE, s))
            else:
                rt.check(L.hupr_sgd_step_guard_f32(rt.ptr(p), rt.ptr(g), *st, n, rt.ptr(dev), rt.ptr(guard), MOM, WD, GSCALE, s))
        elif form == "dev":
            dev[1] += 1
            if kind == "adam":
                rt.check(L.hupr_adam_step_dev_f32(rt.ptr(p), rt.ptr(g), *st, n, rt.ptr(dev), B1, B2, EPS, WD, GSCALE, s))
            else:
                rt.check(L.hupr_sgd_step_dev_f32(rt.ptr(p), rt.ptr(g), *st, n, rt.ptr(dev), MOM, WD, GSCALE, s))
        elif kind == "adam":
            rt.check(L.hupr_adam_step_f32(rt.ptr(p), rt.ptr(g), *st, n, LR, B1, B2, EPS, WD, k, GSCALE, s))
        else:
            rt.check(L.hupr_sgd_step_f32(rt.ptr(p), rt.ptr(g), *st, n, LR, MOM, WD, int(k == 1), GSCALE, s))
        steps.append(_digest(P, *[b for b, _ in bufs]))
        if form == "guard":
            decisions.append(_digest(partials, guard, dev))
            coef, norm, skipped, finite = guard.tolist()
            if k == 1:
                assert (coef, skipped, finite) == (1.0, 0.0, 1.0) and 0 < norm < INF and dev[1].item() == 1.0
            elif k == 2:
                assert 0 < coef < 1 and (skipped, finite) == (0.0, 1.0) and dev[1].item() == 2.0
            else:
                assert (coef, norm, skipped, finite) == (0.0, INF, 1.0, 0.0) and dev[1].item() == 2.0
                assert steps[2] == steps[1]                          # the skipped step stored nothing
    assert len(set(steps)) == (2 if form == "guard" else 3)
    name = "%s_%s" % (kind, form)
    return {name: steps, name + ".decision": decisions} if form == "guard" else {name: steps}


def _average(n, offs):
    """Three ticks and updates (the second behind a guard that skipped the step), then the swap of the average and the parameters."""
    rt, L = _lib()
    s = rt.stream()
    A, B, _ = pools()
    E, e = _place(n, offs[0], A[:n])
    Pb, p = _place(n, offs[1])
    state = torch.zeros(2, device="cuda")
    skipped = torch.tensor([0.0, INF, 1.0, 0.0], device="cuda")
    updates, ticks = [], []
    for k in (1, 2, 3):
        p.copy_(B[k:k + n])
        rt.check(L.hupr_ema_tick_f32(rt.ptr(state), DECAY, rt.ptr(skipped) if k == 2 else None, s))
        rt.check(L.hupr_ema_update_f32(rt.ptr(e), rt.ptr(p), n, rt.ptr(state), s))
        updates.append(_digest(E))
        ticks.append(_digest(state))
        assert state[0].item() == (1.0 if k < 3 else 2.0) and (state[1].item() == 0.0) == (k == 2)
    assert updates[1] == updates[0] != updates[2]
    rt.check(L.hupr_swap_f32(rt.ptr(e), rt.ptr(p), n, s))
    return {"ema_update": updates, "ema_tick": ticks, "swap": [_digest(E, Pb)]}


def case_id(n, offs):
    return "n=%d off=%s" % (n, "-".join(map(str, offs)))


def digests(n, offs):
    out = {}
    for kind in ("adam", "sgd"):
        for form in ("host", "dev", "guard"):
            out.update(_optimizer(kind, form, n, offs))
    out.update(_average(n, offs))
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("offs", OFFSETS, ids=lambda o: "-".join(map(str, o)))
@pytest.mark.parametrize("n", SIZES)
def test_bits_equal_the_recorded_run(n, offs, recorded):
    want = recorded["digests"][case_id(n, offs)]
    got = digests(n, offs)
    moved = [k for k in want if got.get(k) != want[k]]
    print("%s: %d digest lists, moved: %s" % (case_id(n, offs), len(got), moved or "none"))
    assert sorted(got) == sorted(want) and not moved, (case_id(n, offs), moved)


def _hipcc_version():
    import shutil
    import subprocess
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    try:
        lines = subprocess.run([exe, "--version"], capture_output=True, text=True).stdout.splitlines()
    except OSError:
        return None
    return next((ln for ln in lines if "version" in ln.lower()), None)


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_optim_bits_gpu.py --record      (writes %s)" % FIXTURE)
    record = {"hipcc": _hipcc_version(), "partials": _lib()[1].hupr_grad_sumsq_partials(),
              "digests": {case_id(n, offs): digests(n, offs) for n in SIZES for offs in OFFSETS}}
    with open(FIXTURE, "w") as f:
        json.dump(record, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d cases to %s" % (len(record["digests"]), FIXTURE))
