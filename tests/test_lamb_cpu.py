"""CPU (-m "not gpu"): TRAINING.optimizer = lamb — the optimiser choice and TRAINING.lambWeightDecay, the chunk table the LAMB
kernels walk (a pure host function), FusedLAMB's checkpoints over flat buckets and the C-ABI entries."""
import os
import re
import types

import pytest
import torch

from hupr_amd.tools.optim import FusedAdam, FusedLAMB, FusedSGD, lamb_chunk_table, make_optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMB_ENTRIES = ("hupr_lamb_chunk", "hupr_lamb_table_check", "hupr_lamb_stage1_f32", "hupr_lamb_ratio_f32", "hupr_lamb_stage2_f32")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime


def _cfg(name, **training):
    return types.SimpleNamespace(TRAINING=types.SimpleNamespace(optimizer=name, **training))


def _group(opt):
    return {k: v for k, v in opt.param_groups[0].items() if k != "params"}


# ---- make_optimizer ---------------------------------------------------------------------------------------------------------
def test_make_optimizer_builds_lamb():
    net = torch.nn.Linear(4, 3)
    opt = make_optimizer(_cfg("lamb"), net.parameters(), 2e-3)
    assert type(opt) is FusedLAMB
    assert _group(opt) == dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, trust_ratio=True)
    assert opt._state_keys == ("exp_avg", "exp_avg_sq") and opt.grad_clip is None
    assert make_optimizer(_cfg("lamb", gradClip=2.0), net.parameters(), 2e-3).grad_clip == 2.0


@pytest.mark.parametrize("given, expected", [(0, 0.0), (0.05, 0.05), (1, 1.0)])
def test_lamb_weight_decay_is_parsed(given, expected):
    net = torch.nn.Linear(4, 3)
    opt = make_optimizer(_cfg("lamb", lambWeightDecay=given), net.parameters(), 1e-3)
    wd = opt.param_groups[0]["weight_decay"]
    assert wd == expected and type(wd) is float


@pytest.mark.parametrize("bad", [-1, float("nan"), "0.01", float("inf"), True, None])
def test_lamb_weight_decay_is_refused(bad):
    with pytest.raises(ValueError, match="lambWeightDecay"):
        make_optimizer(_cfg("lamb", lambWeightDecay=bad), torch.nn.Linear(4, 3).parameters(), 1e-3)


@pytest.mark.parametrize("other", ["adam", "sgd"])
def test_lamb_weight_decay_with_another_optimiser_is_refused(other):
    with pytest.raises(ValueError, match="lambWeightDecay"):
        make_optimizer(_cfg(other, lambWeightDecay=0.01), torch.nn.Linear(4, 3).parameters(), 1e-3)
    assert type(make_optimizer(_cfg(other), torch.nn.Linear(4, 3).parameters(), 1e-3)) in (FusedAdam, FusedSGD)


def test_unknown_optimiser_error_names_all_three():
    with pytest.raises(ValueError, match="'sgd' or 'adam'") as e:
        make_optimizer(_cfg("rmsprop"), torch.nn.Linear(4, 3).parameters(), 1e-3)
    assert "lamb" in str(e.value) and "rmsprop" in str(e.value)


# ---- the chunk table --------------------------------------------------------------------------------------------------------
def _parse(table):
    S, K, C, n = table[:4]
    segs = [tuple(table[4 + 5 * s:9 + 5 * s]) for s in range(S)]
    chunks = [tuple(table[4 + 5 * S + 2 * k:6 + 5 * S + 2 * k]) for k in range(K)]
    assert len(table) == 4 + 5 * S + 2 * K
    return C, n, segs, chunks


def _segments(lengths, adapted):
    out, at = [], 0
    for n, a in zip(lengths, adapted):
        out.append((at, n, a))
        at += n
    return out


@pytest.mark.parametrize("C", [4, 7, 256, 2048])
def test_chunk_table_tiles_every_segment_once_and_in_order(C):
    lengths = [1, 3, C - 1, C, C + 1, 2 * C, 2 * C + 3]
    adapted = [True, False, True, False, True, False, True]
    chunk, n, segs, chunks = _parse(lamb_chunk_table(_segments(lengths, adapted), C))
    assert chunk == C and n == sum(lengths) and len(segs) == len(lengths)
    covered, at, k = [], 0, 0
    for s, (start, length, first, count, flag) in enumerate(segs):
        assert (start, length, first, flag) == (at, lengths[s], k, int(adapted[s])) and count == -(-length // C)
        for j in range(count):                                   # the segment's chunks are consecutive, in order, from its start
            seg, rel = chunks[first + j]
            assert seg == s and rel == j * C
            lo, hi = start + rel, start + min(rel + C, length)   # no chunk crosses the segment's end
            assert start <= lo < hi <= start + length and hi - lo <= C
            covered += list(range(lo, hi))
        at += length
        k += count
    assert k == len(chunks) and covered == list(range(n))        # every element exactly once, in order


def test_chunk_starts_are_relative_to_their_segment():
    """A segment moved inside its bucket (another tensor in front of it) keeps its chunk entries; only the absolute start moves."""
    C = 8
    alone = _parse(lamb_chunk_table([(0, 2 * C + 3, True)], C))
    moved = _parse(lamb_chunk_table([(0, 5, False), (5, 2 * C + 3, True)], C))
    assert alone[2][0] == (0, 2 * C + 3, 0, 3, 1) and moved[2][1] == (5, 2 * C + 3, 1, 3, 1)
    assert [rel for _, rel in alone[3]] == [rel for seg, rel in moved[3] if seg == 1] == [0, C, 2 * C]


def test_chunk_table_refuses_segments_that_do_not_tile():
    for segs in ([], [(1, 4, True)], [(0, 4, True), (5, 2, True)], [(0, 4, True), (3, 2, True)], [(0, 0, True)]):
        with pytest.raises(ValueError, match="lamb_chunk_table"):
            lamb_chunk_table(segs, 4)
    with pytest.raises(ValueError, match="chunk"):
        lamb_chunk_table([(0, 4, True)], 0)


def test_adapted_flags_follow_ndim(built):
    """Over real buckets: weights (ndim 2) are adapted, biases (ndim 1) are not, and the host check of the library accepts every
    table FusedLAMB builds."""
    from hupr_amd.tools.distributed import GradientBuckets
    net = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 4), torch.nn.Linear(4, 2))
    gb = GradientBuckets(net, bucket_bytes=256, tail_bytes=0)
    opt = FusedLAMB(net.parameters(), lr=1e-3)
    opt.attach_flat_buckets(gb.flat_pairs(), gb.layout())
    C = built.lib().hupr_lamb_chunk()
    assert C > 0 and C % 4 == 0
    seen = 0
    for st, entries, (p, _) in zip(opt._flat_state, gb.layout(), gb.flat_pairs()):
        table = st["lamb"]["host"]
        chunk, n, segs, _ = _parse(table.tolist())
        assert chunk == C and n == p.numel() and len(segs) == len(entries) == st["lamb"]["segments"]
        for (q, off, numel), (start, length, _, _, flag) in zip(entries, segs):
            assert (start, length, flag) == (off, numel, int(q.ndim > 1))
            seen += 1
        assert built.lib().hupr_lamb_table_check(table.data_ptr(), table.numel(), n) == 0
        assert torch.equal(st["lamb"]["dev"], table)
    assert seen == 6 and opt._dev_state is not None              # {lr, step} are in device memory from the attachment on


# ---- checkpoints ------------------------------------------------------------------------------------------------------------
def _net():
    return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 4), torch.nn.Linear(4, 2))


def _lamb_over_buckets(net, lr=1e-3):
    from hupr_amd.tools.distributed import GradientBuckets
    gb = GradientBuckets(net, bucket_bytes=256, tail_bytes=0)
    assert len(gb.buckets) >= 2
    opt = FusedLAMB(net.parameters(), lr=lr, weight_decay=0.02)
    opt.attach_flat_buckets(gb.flat_pairs(), gb.layout())
    return gb, opt


def test_lamb_state_dict_round_trip_is_bit_exact(built):
    torch.manual_seed(13)
    gb, opt = _lamb_over_buckets(_net())
    assert opt.state_dict()["state"] == {}                      # nothing before the first step
    opt._dev_state[1] = 3.0                                     # as if 3 steps had run
    for st in opt._flat_state:
        st["exp_avg"].normal_()
        st["exp_avg_sq"].uniform_()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(6)) and sd["param_groups"][0]["params"] == list(range(6))
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} and float(s["step"]) == 3.0 for s in sd["state"].values())
    assert sd["param_groups"][0]["trust_ratio"] is True and sd["param_groups"][0]["eps"] == 1e-6
    assert sd["param_groups"][0]["weight_decay"] == 0.02
    gb2, opt2 = _lamb_over_buckets(_net(), lr=5e-4)
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["lr"] == 1e-3 and len(opt2.state) == 0
    assert opt2._dev_state.tolist() == [pytest.approx(1e-3), 3.0]
    for a, b in zip(opt._flat_state, opt2._flat_state):
        assert b["step"] == 3
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))
    sd2 = opt2.state_dict()
    for i in sd["state"]:
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sd["state"][i][k], sd2["state"][i][k])


def test_lamb_refuses_an_sgd_checkpoint_by_name(built):
    net = _net()
    gb, opt = _lamb_over_buckets(net)
    sgd = FusedSGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    sgd.attach_flat_buckets(gb.flat_pairs(), gb.layout())
    for st in sgd._flat_state:
        st["step"] = 2
    with pytest.raises(ValueError, match="SGD"):
        opt.load_state_dict(sgd.state_dict())
    assert all(st["step"] == 0 for st in opt._flat_state) and opt.param_groups[0]["trust_ratio"] is True


def test_lamb_refuses_an_adam_checkpoint_by_name(built):
    net = _net()
    gb, opt = _lamb_over_buckets(net)
    adam = FusedAdam(net.parameters(), lr=1e-3, weight_decay=1e-4)
    adam.attach_flat_buckets(gb.flat_pairs(), gb.layout())
    for st in adam._flat_state:
        st["step"] = 2
    for sd in (adam.state_dict(), torch.optim.Adam(net.parameters(), lr=1e-3).state_dict()):
        with pytest.raises(ValueError, match="Adam"):
            opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert all(st["step"] == 0 for st in opt._flat_state) and g["eps"] == 1e-6 and g["weight_decay"] == 0.02


def test_lamb_step_without_buckets_raises():
    net = torch.nn.Linear(4, 3)
    opt = FusedLAMB(net.parameters(), lr=1e-3)
    net(torch.ones(2, 4)).sum().backward()
    with pytest.raises(RuntimeError, match="attach_flat_buckets"):
        opt.step()
    with pytest.raises(RuntimeError, match="layout"):
        opt.attach_flat_buckets([(torch.zeros(4), torch.zeros(4))])


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_lamb_entry_points_are_declared_and_bound(built):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hupr.h")).read(), flags=re.S)
    lib = built.lib()
    for name in LAMB_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in built.SIGNATURES and hasattr(lib, name), name


def test_table_check_refuses_bad_tables_on_the_host(built):
    """hupr_lamb_table_check runs on the host only: a gap, an overlap, a run past n, another chunk size, a truncated table."""
    L = built.lib()
    C = L.hupr_lamb_chunk()
    good = lamb_chunk_table([(0, 5, True), (5, C + 1, False)], C)

    def check(table, n):
        t = torch.tensor(table, dtype=torch.int64)
        return L.hupr_lamb_table_check(t.data_ptr(), t.numel(), n)
    assert check(good, C + 6) == 0
    gap, overlap, past = list(good), list(good), list(good)
    gap[4 + 5] = 6
    overlap[4 + 5] = 4
    past[4 + 5 + 1] = C + 2
    for bad, word in ((gap, b"gap"), (overlap, b"overlap"), (past, b"past n")):
        assert check(bad, C + 6) == -1
        assert b"hupr_lamb_table_check" in L.hupr_last_error() and word in L.hupr_last_error(), L.hupr_last_error()
    assert check(good, C + 7) == -1 and check(good[:-1], C + 6) == -1
    assert check(lamb_chunk_table([(0, 5, True), (5, C + 1, False)], C // 2), C + 6) == -1
    assert L.hupr_lamb_table_check(None, 10, 4) == -1


# ---- the Runner's line ------------------------------------------------------------------------------------------------------
def test_trust_ratio_line_names_the_extremes_of_the_adapted_tensors():
    from hupr_amd.tools.run import trust_ratio_line
    params = {"a.weight": torch.zeros(2, 2), "a.bias": torch.zeros(2), "b.weight": torch.zeros(3, 2), "c.weight": torch.zeros(1, 1, 3)}
    stats = {"a.weight": (1.0, 2.0, 0.5), "a.bias": (1.0, 9.0, 1.0), "b.weight": (4.0, 1.0, 4.0), "c.weight": (1.0, 0.5, 2.0)}
    line = trust_ratio_line(7, stats, params)
    assert "epoch 7" in line and "3 adapted tensors" in line and "a.bias" not in line
    assert "min 0.5 (a.weight)" in line and "median 2 " in line and "max 4 (b.weight)" in line
    assert "no adapted tensor" in trust_ratio_line(0, {"a.bias": (1.0, 1.0, 1.0)}, params)
