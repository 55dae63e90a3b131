"""CPU (no GPU needed): the routing of the temporal merges (hupr_tmerge_stream_supported, hupr_tmerge_wgrad_stream_supported and the
workgroup count behind hupr_tmerge_wgrad_stream_ws_bytes: host code only) sends every case of the fp64 table
(test_tmerge_fp64_gpu.py), the merge cases of test_ops_gpu.py and the three model-scale levels to the kernels they name — a change that
silently moves level 1 back to the generic engine fails here; the table reaches every instantiation, both reduce kernels, every kind
of persistent loop and every reason for the generic engine; the refused calls are refused by host checks alone; and the fp64 gate of
the table rejects the results of subtly wrong kernels (a frame dropped, exchanged or read from a stale ring slot, a K step or a tile
missing, reversed taps, dy truncated instead of rounded) while it accepts an fp32 accumulation in another order and its bf16 store."""
import pytest
import torch

import test_ops_gpu as O
import test_tmerge_fp64_gpu as T


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


# ---- routes ------------------------------------------------------------------------------------------------------------------------
def reasons(L, c):
    """Which of G, HW, C keeps a generic case off the streaming kernel of its operation: the attribute whose repair alone would let it
    stream, or one that no choice of the others can make up for; "storage" where only the fp32 storage does."""
    sup = L.hupr_tmerge_wgrad_stream_supported if c.op == "wgrad" else L.hupr_tmerge_stream_supported
    HW = c.H * c.W
    if sup(c.G, HW, c.C, c.C):
        return {"storage"} if c.store != "bf16" else set()
    Gs, HWs, Cs = (8, 4, 2, 1), (128, 256), (64, 128, 256)
    out = set()
    if any(sup(g, HW, c.C, c.C) for g in Gs) or not any(sup(c.G, hw, C, C) for hw in HWs for C in Cs):
        out.add("G")
    if any(sup(c.G, hw, c.C, c.C) for hw in HWs) or not any(sup(g, HW, C, C) for g in Gs for C in Cs):
        out.add("HW")
    if any(sup(c.G, HW, C, C) for C in Cs) or not any(sup(g, hw, c.C, c.C) for g in Gs for hw in HWs):
        out.add("C")
    return out


@pytest.mark.parametrize("c", T.CASES, ids=[T.case_id(c) for c in T.CASES])
def test_fp64_case_table_routes(c, L):
    assert T.route_of(L, c) == T.expected_route(c)
    if c.route == "generic":
        assert c.grid is None and c.why in reasons(L, c), (c.why, reasons(L, c))
    else:
        assert c.why is None and c.store == "bf16" and (c.H * c.W) % 128 == 0
        if c.op == "wgrad":                  # the table's literal grid is the launcher's plan: Co / 64 blocks x min(tiles, 256 / NB) slots
            assert c.grid == (c.C // 64, min(T.tiles_of(c), 256 // (c.C // 64)))
        else:
            assert c.grid is None and c.C == 64


def loop_kinds(tiles, cap):
    """How the persistent loop over `tiles` looks on a grid capped at `cap` workgroups (slots)."""
    if tiles < cap:
        return "fewer tiles than the cap: one each"
    if tiles == cap:
        return "one tile for each of the cap"
    return "several each, evenly" if tiles % cap == 0 else "several each, unevenly"


def test_the_table_reaches_every_instantiation_and_loop_kind():
    stream = [c for c in T.CASES if c.route == "stream"]
    for op in ("fwd", "dgrad"):
        assert {c.G for c in stream if c.op == op} == {8, 4, 2}
        for G in (8, 4, 2):
            tiles = {T.tiles_of(c) for c in stream if c.op == op and c.G == G}
            assert tiles >= {1, 2, 3, 257, 264, 512}, (op, G)
            assert {loop_kinds(t, 256) for t in tiles} >= {"fewer tiles than the cap: one each", "several each, evenly",
                                                           "several each, unevenly"}, (op, G)
        t2 = {T.tiles_of(c) for c in stream if c.op == op and c.G == 2}
        assert 520 in t2 and 256 in t2                      # two and three tiles per workgroup in one launch; tiles == grid
        assert len({loop_kinds(T.tiles_of(c), 256) for c in stream if c.op == op}) == 4
        # G = 2: a tile is two stages, shorter than the three-stage prologue of the forward ring
        assert any(c.G == 2 and T.tiles_of(c) == 1 for c in stream if c.op == op)
        assert any(c.H != c.W and c.H * c.W > 128 for c in stream if c.op == op)
    wg = [c for c in stream if c.op == "wgrad"]
    # hupr_k_tmerge_wgrad_stream<F> with SUB = C / 64 virtual frames per frame: every pair with F = G SUB in {8, 4, 2}
    assert {(c.G * c.C // 64, c.C // 64) for c in wg} == {(F, SUB) for F in (8, 4, 2) for SUB in (1, 2, 4) if F >= SUB}
    assert len({loop_kinds(T.tiles_of(c), 256 // c.grid[0]) for c in wg}) == 4
    for NB in (1, 2, 4):
        assert any(T.tiles_of(c) % c.grid[1] != 0 for c in wg if c.grid[0] == NB), NB
    # hupr_k_tmerge_wgrad_reduce4 (C = 64) over 1, 3, 17 and 256 partials; the general reduce with NB = 2 and 4 below and above 16 slots
    for G in (8, 4, 2):
        assert {c.grid[1] for c in wg if c.C == 64 and c.G == G} >= {1, 3, 17, 256}
    for NB in (2, 4):
        slots = {c.grid[1] for c in wg if c.grid[0] == NB}
        assert min(slots) < 16 < max(slots) and max(slots) == 256 // NB
    generic = [c for c in T.CASES if c.route == "generic"]
    assert {c.why for c in generic} == {"G", "HW", "C", "storage"}
    for op in T.OPS:
        mine = [c for c in generic if c.op == op]
        assert {(c.G, c.H, c.C) for c in mine} >= {(6, 16, 64), (8, 8, 64), (1, 16, 64), (3, 16, 128), (8, 16, 128)}, op
        assert any(c.store == "f32" and (c.G, c.H, c.W, c.C) == (4, 16, 16, 64) for c in mine), op


def _params(test):
    (mark,) = [m for m in test.pytestmark if m.name == "parametrize"]
    return mark.args[0], mark.args[1]


def test_existing_merge_tests_and_model_levels_still_stream(L):
    """The merge cases of test_ops_gpu.py and the three encoder levels at the bench batch keep their streaming kernels."""
    names, params = _params(O.test_streaming_temporal_merge_matches_the_generic_kernel)
    assert names == "B,H" and len(params) >= 3
    for B, H in params:
        assert L.hupr_tmerge_stream_supported(8, H * H, 64, 64) and L.hupr_tmerge_wgrad_stream_supported(8, H * H, 64, 64), (B, H)
        assert L.hupr_tmerge_wgrad_stream_ws_bytes(B, 8, H * H, 64, 64) == min(B * H * H // 128, 256) * 64 * 64 * 8 * 4
    names, params = _params(O.test_streaming_merge_weight_gradient_on_wider_maps)
    assert names == "B,G,H,C" and len(params) >= 5
    for B, G, H, C in params:
        assert L.hupr_tmerge_wgrad_stream_supported(G, H * H, C, C), (B, G, H, C)          # (else that test would skip)
        NB = C // 64
        assert L.hupr_tmerge_wgrad_stream_ws_bytes(B, G, H * H, C, C) == NB * min(B * H * H // 128, 256 // NB) * 64 * 64 * G * NB * 4
    # model scale, B = 32: level 1 on all three streaming kernels, levels 2 and 3 on the streaming weight gradient
    assert L.hupr_tmerge_stream_supported(8, 64 * 64, 64, 64)
    for G, H, C, NB, slots in ((8, 64, 64, 1, 256), (4, 32, 128, 2, 128), (2, 16, 256, 4, 64)):
        assert L.hupr_tmerge_wgrad_stream_supported(G, H * H, C, C), (G, H, C)
        assert L.hupr_tmerge_wgrad_stream_ws_bytes(32, G, H * H, C, C) == NB * slots * 64 * 64 * 8 * 4, (G, H, C)
    # the forward and the input gradient of levels 2 and 3 are the generic engine's (C != 64)
    assert not L.hupr_tmerge_stream_supported(4, 32 * 32, 128, 128) and not L.hupr_tmerge_stream_supported(2, 16 * 16, 256, 256)


def test_supported_answers_at_the_edges(L):
    for G in range(0, 12):
        assert bool(L.hupr_tmerge_stream_supported(G, 256, 64, 64)) == (G in (8, 4, 2)), G
        for C in (64, 128, 192, 256, 320):
            assert bool(L.hupr_tmerge_wgrad_stream_supported(G, 256, C, C)) == (C <= 256 and G * C // 64 in (8, 4, 2)), (G, C)
    for HW in (64, 127, 128, 192, 256, 4096 + 64):
        assert bool(L.hupr_tmerge_stream_supported(8, HW, 64, 64)) == (HW % 128 == 0), HW
        assert bool(L.hupr_tmerge_wgrad_stream_supported(4, HW, 128, 128)) == (HW % 128 == 0), HW
    for Ci, Co in ((64, 128), (128, 64), (32, 32), (96, 96), (512, 512)):
        assert not L.hupr_tmerge_stream_supported(8, 256, Ci, Co) and not L.hupr_tmerge_wgrad_stream_supported(1, 256, Ci, Co), (Ci, Co)
    assert L.hupr_tmerge_wgrad_stream_ws_bytes(0, 8, 256, 64, 64) == 0 and L.hupr_tmerge_wgrad_stream_ws_bytes(4, 6, 256, 64, 64) == 0


@pytest.mark.parametrize("r", T.REFUSED, ids=[r[0] for r in T.REFUSED])
def test_refused_calls_are_refused_by_host_checks(r, L):
    """On made-up addresses and without a device: the error comes back before anything is launched or dereferenced."""
    base = 1 << 24
    n0 = L.hupr_launch_count()
    rc = T.refused_call(L, r, base, 2 * base, 3 * base, 4 * base, 5 * base, None)
    assert rc in (T.HUPR_ERR_ARG, T.HUPR_ERR_WORKSPACE), (r[0], rc, L.hupr_last_error())
    assert L.hupr_launch_count() == n0


# ---- gate sensitivity, on CPU fp64 data ----------------------------------------------------------------------------------------------
SHAPE = (2, 8, 16, 16, 64)                    # 4 tiles of 128 voxels, two per sample


def stored(op, t):
    """What a kernel would leave in memory of the sums t: one rounding to fp32, for dx one more to bf16."""
    return t.float().to(torch.bfloat16) if op == "dgrad" else t.float()


def _ok(op, t, ref, A):
    return T.within(stored(op, t), ref, A, T.GATE_C[op], op == "dgrad")


def _rejects(op, bad, ref, A, what, frac=0.8):
    """bad: faulty fp64 sums; stored as the kernel stores them they must fail the gate at >= frac of the outputs the fault touches and
    nowhere else."""
    ok = _ok(op, bad, ref, A)
    touched = bad != ref
    n = int(touched.sum())
    caught = int((~ok & touched).sum())
    assert n > 0, what
    assert caught >= frac * n and caught >= 1, (what, caught, n)
    assert not bool((~ok & ~touched).any()), what


def truncated(t):
    """fp32 -> bf16 by dropping the low 16 bits, as fp64."""
    return (t.float().view(torch.int32) & -65536).view(torch.float32).double()


@pytest.fixture(scope="module")
def data():
    B, G, H, W, C = SHAPE
    x, w, dy = T.make_operands(*SHAPE)
    d = {"x": x.double(), "wq": T.q(w), "dy": dy, "dyq": T.q(dy)}
    d["fwd"] = T.fwd_ref(d["x"], d["wq"])
    d["dgrad"] = T.dgrad_ref(d["dyq"], d["wq"])
    d["wgrad"] = T.wgrad_ref(d["x"], d["dyq"])
    return d


def test_gate_accepts_faithful_results(data):
    """The fp64 sums rounded once (and, for dx, once more to bf16) pass everywhere."""
    for op in T.OPS:
        ref, A = data[op]
        assert bool(_ok(op, ref, ref, A).all()), op


def test_gate_rejects_a_dropped_or_exchanged_frame(data):
    x, wq, dyq = data["x"], data["wq"], data["dyq"]
    xz = x.clone()
    xz[:, 3] = 0
    _rejects("fwd", T.fwd_ref(xz, wq)[0], *data["fwd"], "fwd: frame 3 never multiplied")
    xs = x.clone()
    xs[:, 2], xs[:, 5] = x[:, 5], x[:, 2]
    _rejects("fwd", T.fwd_ref(xs, wq)[0], *data["fwd"], "fwd: frames 2 and 5 exchanged")
    for op, dim in (("dgrad", 1), ("wgrad", 2)):
        ref, A = data[op]
        bad = ref.clone()
        bad.select(dim, 3).zero_()
        _rejects(op, bad, ref, A, op + ": frame 3 left zero")
        bad = ref.clone()
        bad.select(dim, 2).copy_(ref.select(dim, 5))
        bad.select(dim, 5).copy_(ref.select(dim, 2))
        _rejects(op, bad, ref, A, op + ": frames 2 and 5 exchanged")
        _rejects(op, ref.flip(dim), ref, A, op + ": taps reversed")


def test_gate_rejects_a_stage_read_from_a_stale_ring_slot(data):
    """The forward ring without one dma(n + kTmStages - 1) re-issue: the stage multiplied is the one that sat in the slot four stages
    earlier — frame 6 of a tile replaced by its frame 2; and across a tile border, frame 1 replaced by frame 5 of the workgroup's
    previous tile.  The weight gradient's ring (two dy stages + G frames per tile): x frame 4 replaced by x frame 0."""
    x, wq, dyq = data["x"], data["wq"], data["dyq"]
    xs = x.clone()
    xs[0, 6, 128:256] = x[0, 2, 128:256]
    _rejects("fwd", T.fwd_ref(xs, wq)[0], *data["fwd"], "fwd: stale slot inside a tile")
    xs = x.clone()
    xs[1, 1, 0:128] = x[0, 5, 128:256]
    _rejects("fwd", T.fwd_ref(xs, wq)[0], *data["fwd"], "fwd: stale slot across a tile border")
    xs = x.clone()
    xs[1, 4, 128:256] = x[1, 0, 128:256]
    _rejects("wgrad", T.wgrad_ref(xs, dyq)[0], *data["wgrad"], "wgrad: stale slot")


def test_gate_rejects_a_missing_k_step_or_tile(data):
    x, wq, dyq = data["x"], data["wq"], data["dyq"]
    # one 16-voxel K step of one tile missing from one wave's 32 x 32 block of every frame
    part = torch.zeros_like(dyq)
    part[1, 160:176] = dyq[1, 160:176]
    ref, A = data["wgrad"]
    bad = ref.clone()
    bad[:32, 32:] -= T.wgrad_ref(x, part)[0][:32, 32:]
    _rejects("wgrad", bad, ref, A, "wgrad: one K step")
    # one tile never accumulated
    part = torch.zeros_like(dyq)
    part[0, 128:256] = dyq[0, 128:256]
    _rejects("wgrad", ref - T.wgrad_ref(x, part)[0], ref, A, "wgrad: one tile")
    # one tile of the output left zero (a workgroup's last tile not reached)
    ref, A = data["fwd"]
    bad = ref.clone()
    bad[1, 128:256] = 0
    _rejects("fwd", bad, ref, A, "fwd: one tile zero")
    ref, A = data["dgrad"]
    bad = ref.clone()
    bad[1, :, 128:256] = 0
    _rejects("dgrad", bad, ref, A, "dgrad: one tile zero")
    bad = ref.clone()
    bad[1, 5, 128:256] = 0
    _rejects("dgrad", bad, ref, A, "dgrad: one frame of one tile zero")


def test_gate_rejects_dy_truncated_to_bf16(data):
    """dy cut to bf16 instead of rounded to nearest even: every product is off by up to 2^-7 of itself, two bf16 steps of dy.  The
    fp32 dW shows that nearly everywhere.  Behind the bf16 store of dx the fault is of the size of the store's own rounding (about
    2^-9 of a typical result): together they exceed 2^-8 |ref| at about half of the elements, and the gate fails there."""
    x, wq, dy = data["x"], data["wq"], data["dy"]
    dyt = truncated(dy)
    assert bool((dyt != data["dyq"]).float().mean() > 0.4)
    _rejects("wgrad", T.wgrad_ref(x, dyt)[0], *data["wgrad"], "wgrad: dy truncated")
    _rejects("dgrad", T.dgrad_ref(dyt, wq)[0], *data["dgrad"], "dgrad: dy truncated", frac=0.3)


def fp32_reversed(op, x, wq, dyq):
    """The same products accumulated in fp32 with every contracted axis reversed."""
    x, wq, dyq = x.float(), wq.float(), dyq.float()
    if op == "fwd":
        return torch.einsum("bgvc,ocg->bvo", x.flip(1, 3), wq.flip(2, 1))
    if op == "dgrad":
        return torch.einsum("bvo,ocg->bgvc", dyq.flip(2), wq.flip(0))
    return torch.einsum("bvo,bgvc->ocg", dyq.flip(0, 1), x.flip(0, 2))


def test_gate_accepts_fp32_accumulation_in_reversed_order(data):
    for op in T.OPS:
        ref, A = data[op]
        got = fp32_reversed(op, data["x"], data["wq"], data["dyq"])
        assert got.dtype == torch.float32
        assert bool(_ok(op, got, ref, A).all()), op
        if op != "dgrad":
            assert bool((got.double() != ref).any())           # (it is another result than the reference's)


CPU_CASES = [c for c in T.CASES if c.B * c.G * c.H * c.W * c.C <= 1 << 22]
assert len(CPU_CASES) >= 40


@pytest.mark.parametrize("c", CPU_CASES, ids=[T.case_id(c) for c in CPU_CASES])
def test_reversed_fp32_accumulation_stays_inside_the_committed_gate(c):
    """With the c values committed in the GPU file, an honest fp32 accumulation of each table shape small enough for the CPU stays
    inside the gate (bf16 store included for a bf16 dx)."""
    x, w, dy = T.make_operands(c.B, c.G, c.H, c.W, c.C)
    wq, dyq = T.q(w), T.q(dy)
    ref, A = {"fwd": lambda: T.fwd_ref(x, wq), "dgrad": lambda: T.dgrad_ref(dyq, wq), "wgrad": lambda: T.wgrad_ref(x, dyq)}[c.op]()
    got = fp32_reversed(c.op, x, wq, dyq)
    bf = c.op == "dgrad" and c.store == "bf16"
    out = got.to(torch.bfloat16) if bf else got
    ok = T.within(out, ref, A, T.GATE_C[c.op], bf)
    assert bool(ok.all()), (T.case_id(c), T.measured(out, ref, A, bf), T.GATE_C[c.op])
