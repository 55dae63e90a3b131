"""CPU (no GPU needed): the routing of the network's last stage (functional.gcn_route, functional.head_route: host code only) sends every
GCNLayerFn case of the fp64 table (test_head_fp64_gpu.py), the cases of test_ops_gpu.test_gcn_layer and the model's own shapes to the
kernels they name — a change that silently moves B = 32 off the product kernels, or B = 1 off the sliced forward, fails here; the
table reaches both instantiations and every prefetch branch of the product kernels, both ld branches of the adjacency forward, a
wrapping grid-stride loop of every kernel that has one and the four kinds of workgroup of the head's weight gradient, and names every
entry point of csrc/head.hip and csrc/gcn_products.hip; the refused calls are refused by host checks alone; and the fp64 gates of the
table reject the results of subtly wrong kernels (W or the adjacency transposed, a K slice or a chunk dropped, the masked sample
counted, the ReLU mask taken from dy, bias indexed [k][f], two channels exchanged, the clamp missing, the mean over n + 1, the last of
several ties) while they accept the fp64 result rounded to fp32 and an fp32 accumulation in reversed order."""
import os
import re

import pytest
import torch

import test_head_fp64_gpu as T
import test_ops_gpu as O


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


@pytest.fixture
def F_(L):
    from hupr_amd import functional
    return functional


def cases(op):
    return [c for c in T.CASES if c.op == op]


def find(op, *p):
    (c,) = [c for c in T.CASES if c.op == op and c.p == p]
    return c


# ---- routes ------------------------------------------------------------------------------------------------------------------------
LAYERS = cases("layer")


@pytest.mark.parametrize("c", LAYERS, ids=[T.case_id(c) for c in LAYERS])
def test_layer_cases_take_the_route_the_table_names(c, F_, monkeypatch):
    B, F, relu, products = c.p
    monkeypatch.setattr(F_, "GCN_PRODUCTS", products)
    fwd = F_.gcn_route(B, F, 16, (F, F), torch.float32)
    bwd = F_.gcn_route(B, F, 16, (F, F), torch.float32, backward=True)
    assert fwd == c.route
    # restated: sliced iff B == 1 and F % 1024 == 0; the product kernels need GCN_PRODUCTS, ld = 16, F % 64 == 0, backward also B > 1
    ok = products and F % 64 == 0
    assert fwd == ("sliced" if B == 1 and F % 1024 == 0 else "products" if ok else "generic")
    assert bwd == ("products" if ok and B > 1 else "generic")
    # the entry points the case names are those of its two routes
    fwd_calls, _ = T.LAYER_CALLS[fwd]
    _, bwd_calls = T.LAYER_CALLS[bwd if bwd == "products" else "generic"]
    assert set(c.entry) == set(fwd_calls) | set(bwd_calls)


def test_layer_cases_cover_the_three_routes_both_activations_and_both_reasons_for_generic():
    assert {c.route for c in LAYERS} == {"sliced", "products", "generic"}
    for route in ("sliced", "products"):
        assert {c.p[2] for c in LAYERS if c.route == route} == {0, 1}, route
    generic = [c for c in LAYERS if c.route == "generic"]
    assert any(not c.p[3] for c in generic) and any(c.p[3] and c.p[1] == 96 for c in generic)
    assert {c.p[2] for c in generic} == {0, 1}
    assert any(c.route == "products" and c.p[0] == 1 for c in LAYERS)          # Bn = 1 through the product forward
    assert any(c.route == "sliced" and c.p[:2] == (1, 1024) for c in LAYERS)   # the path of every live-stream frame


def _params(test):
    (mark,) = [m for m in test.pytestmark if m.name == "parametrize"]
    return mark.args[0], mark.args[1]


def test_existing_layer_test_and_model_shapes_keep_their_kernels(F_, monkeypatch):
    names, params = _params(O.test_gcn_layer)
    assert names == "B,products" and len(params) >= 4
    for B, products in params:
        monkeypatch.setattr(F_, "GCN_PRODUCTS", products)
        want = "products" if products else "generic"
        assert B > 1
        assert F_.gcn_route(B, 1024, 16, (1024, 1024), torch.float32) == want, (B, products)
        assert F_.gcn_route(B, 1024, 16, (1024, 1024), torch.float32, backward=True) == want, (B, products)
    monkeypatch.setattr(F_, "GCN_PRODUCTS", True)
    # the model: F = 1024, ld = 16; B = 1 (inference, every live-stream frame) and B = 32 (the bench batch), in both math modes
    for mode in ("f32", "bf16"):
        with F_.math_mode(mode):
            assert F_.gcn_route(1, 1024, 16, (1024, 1024), torch.float32) == "sliced"
            assert F_.gcn_route(1, 1024, 16, (1024, 1024), torch.float32, backward=True) == "generic"
            assert F_.gcn_route(32, 1024, 16, (1024, 1024), torch.float32) == "products"
            assert F_.gcn_route(32, 1024, 16, (1024, 1024), torch.float32, backward=True) == "products"
    # what keeps a layer off the product kernels
    assert F_.gcn_route(32, 1024, 14, (1024, 1024), torch.float32) == "generic"
    assert F_.gcn_route(32, 1024, 16, (1024, 1024), torch.bfloat16) == "generic"
    assert F_.gcn_route(32, 1024, 16, (512, 1024), torch.float32) == "generic"
    assert F_.gcn_route(32, 96, 16, (96, 96), torch.float32) == "generic"
    assert F_.gcn_route(1, 2048, 14, (2048, 2048), torch.float32) == "sliced"
    assert F_.gcn_route(1, 192, 16, (192, 192), torch.float32) == "products"
    monkeypatch.setattr(F_, "GCN_MATH", "bf16")
    with F_.math_mode("bf16"):
        assert F_.gcn_route(32, 1024, 16, (1024, 1024), torch.float32) == "generic"
    assert F_.gcn_route(32, 1024, 16, (1024, 1024), torch.float32) == "products"          # (the calling thread's fp32 pipe)


class _FakeMap:
    """What head_conv looks at of its input."""

    def __init__(self, is_cuda, dtype, channels):
        self.is_cuda, self.dtype, self.shape = is_cuda, dtype, (2, 1, 8, 8, channels)


def test_head_conv_takes_the_dedicated_kernels_inside_a_switched_head_region_only(F_, monkeypatch):
    w = torch.zeros(14, 32, 1, 1)
    assert F_.head_route(True, True, torch.float32, 32, w.shape, 14) == "head1x1"
    for args in ((False, True, torch.float32, 32, w.shape, 14), (True, False, torch.float32, 32, w.shape, 14),
                 (True, True, torch.bfloat16, 32, w.shape, 14), (True, True, torch.float32, 64, w.shape, 14),
                 (True, True, torch.float32, 32, (16, 32, 1, 1), 14), (True, True, torch.float32, 32, (14, 32, 3, 3), 14)):
        assert F_.head_route(*args) == "generic", args
    # head_conv itself, with its two targets replaced by recorders
    calls = []
    monkeypatch.setattr(F_.Head1x1Fn, "apply", staticmethod(lambda x, weight, w16: calls.append("head1x1")))
    monkeypatch.setattr(F_, "conv", lambda *a: calls.append("generic"))
    monkeypatch.setattr(F_, "_head_w16_cached", lambda weight: None)
    monkeypatch.setattr(F_, "head_weight16", lambda weight, k: None)
    x = _FakeMap(True, torch.float32, 32)
    prev = F_.MATH
    F_.set_math("bf16")
    try:
        F_.head_conv(x, w, 14)                                   # a bf16 run outside the region
        with F_.region("head"):
            assert F_._REGION_SWITCHED == (F_.PRECISION.get("head") == "f32")
            F_.head_conv(x, w, 14)
            F_.head_conv(_FakeMap(True, torch.bfloat16, 32), w, 14)
        with F_.region("dec3"):
            F_.head_conv(x, w, 14)
        F_.set_math("f32")
        with F_.region("head"):                                  # the fp32 parity path: nothing is switched
            assert not F_._REGION_SWITCHED
            F_.head_conv(x, w, 14)
    finally:
        F_.set_math(prev)
    assert F_.PRECISION.get("head") == "f32"                     # the default: the model's head is on these kernels
    assert calls == ["generic", "head1x1", "generic", "generic", "generic"]


# ---- coverage of the table -----------------------------------------------------------------------------------------------------------
def wx_branches(F):
    """The prefetch branches hupr_k_gcn_wx takes over one K half of F / 2 elements, restated: per trip (kk + 32 < kend, kk + 64 < kend)."""
    kend, out = F // 2, []
    for kk in range(0, kend, 64):
        out.append((kk + 32 < kend, kk + 32 < kend and kk + 64 < kend))
    return out


def dw_branches(Bn):
    """... and hupr_k_gcn_dw over the batch, four samples per trip: (b + 2 < Bn, b + 4 < Bn) and whether the last pair is masked."""
    return [(b + 2 < Bn, b + 2 < Bn and b + 4 < Bn) for b in range(0, Bn, 4)], Bn % 2 == 1


def test_the_table_reaches_every_branch_of_the_product_kernels():
    for tw in (0, 1):
        mine = [c for c in cases("wx") if c.p[2] == tw and not c.p[3]]
        assert {c.p[0] // 64 for c in mine} == {1, 2, 3, 16}, tw                 # chunks of 32 per K half
        trips = {t for c in mine for t in wx_branches(c.p[0])}
        assert trips == {(False, False), (True, False), (True, True)}, tw
        assert wx_branches(64) == [(False, False)] and wx_branches(128) == [(True, False)]          # prologue only; one full round
        assert wx_branches(192) == [(True, True), (False, False)]                                      # an odd chunk count
        for F in (64, 128, 192):
            assert {c.p[1] for c in mine if c.p[0] == F} >= {1, 2, 5}, (tw, F)  # one sample, a pair, a masked odd sample
        assert {c.p[1] for c in mine if c.p[0] == 1024} >= {2, 3}, tw
        assert sum(1 for c in cases("wx") if c.p[2] == tw and c.p[3]) == 1       # the exact-index case
    mine = [c for c in cases("dw") if not c.p[2]]
    assert {c.p[1] % 4 for c in mine if c.p[0] == 64} == {0, 1, 2, 3} and {c.p[1] for c in mine if c.p[0] == 64} >= set(range(1, 9))
    trips, masked = set(), set()
    for c in mine:
        t, m = dw_branches(c.p[1])
        trips |= set(t)
        masked.add(m)
    assert trips == {(False, False), (True, False), (True, True)} and masked == {False, True}
    assert dw_branches(1) == ([(False, False)], True) and dw_branches(5) == ([(True, True), (False, False)], True)
    assert dw_branches(7) == ([(True, True), (True, False)], True) and dw_branches(6)[1] is False
    assert {c.p[0] for c in mine} >= {64, 192, 1024} and any(c.p[2] for c in cases("dw"))


def test_the_table_reaches_both_ld_branches_every_k_and_both_adjacencies():
    for op in ("adj_fwd", "adj_bwd"):
        mine = cases(op)
        assert {(c.p[2], c.p[3]) for c in mine} == set(T.K_LD) == {(14, 16), (14, 14), (5, 8), (16, 16), (1, 4)}
        for K, ld in T.K_LD:
            sub = [c for c in mine if (c.p[2], c.p[3]) == (K, ld)]
            assert {c.p[4] for c in sub} == {0, 1} and {c.p[0] for c in sub} >= {64, 1024} and {c.p[1] for c in sub} >= {1, 3}
            assert {c.p[5] for c in sub} == ({"dense", "model"} if K == 14 else {"dense"})
    assert {c.route for c in cases("adj_fwd")} == {"ld16", "scalar"} == {c.route for c in cases("adj_sliced")}
    assert all(c.route == T.ld_route(c.p[3]) for c in cases("adj_fwd") + cases("adj_sliced"))
    assert {c.p[6] for c in cases("adj_sliced")} == {1, 2, 8, 64}
    assert {c.p[4] for c in cases("adj_sliced")} == {0, 1}
    # the dense adjacency is not symmetric, and the model's is nearly so: only the dense one shows a transposition everywhere
    dense, model = T.adjacency_of("dense", 14), T.adjacency_of("model", 14)
    assert int((dense != dense.t()).sum()) == 14 * 13 and int((model != model.t()).sum()) == 4


def grid1d(n, bs=256, cap=4096):
    return min(cap, (n + bs - 1) // bs)


def loop_wraps(c):
    """{kernel: its grid-stride loop takes a second trip}, from the launchers' grid arithmetic restated."""
    p = c.p
    if c.op in ("adj_fwd", "adj_sliced"):
        rows = p[0] * p[1]
        return {"hupr_k_gcn_adj_fwd" + ("/sliced" if c.op == "adj_sliced" else ""): rows > min(4096, (rows + 15) // 16) * 16}
    if c.op == "adj_bwd":
        rows = p[0] * p[1]
        return {"hupr_k_gcn_adj_bwd": rows > grid1d(rows) * 256}
    if c.op == "sigmoid":
        Bn, K, ld, HW = p
        return {"hupr_k_sigmoid_to_nchw": Bn * K * HW > grid1d(Bn * K * HW) * 256,
                "hupr_k_sigmoid_to_nchw_bwd": Bn * HW * ld > grid1d(Bn * HW * ld) * 256}
    if c.op in ("bce", "bce_pair"):
        n, pair = p[0], "_pair" if c.op == "bce_pair" else ""
        return {"hupr_k_bce%s_fwd" % pair: n > grid1d(n, 256, 1024) * 256, "hupr_k_bce%s_bwd" % pair: n > grid1d(n) * 256}
    if c.op == "targets":
        n = p[0] * p[1] * p[2] * p[2]
        return {"hupr_k_gaussian_targets": n > grid1d(n) * 256}
    return {}


def test_every_grid_stride_loop_wraps_in_some_case_and_not_in_another():
    seen = {}
    for c in T.CASES:
        for kernel, wraps in loop_wraps(c).items():
            seen.setdefault(kernel, set()).add(wraps)
    want = {"hupr_k_gcn_adj_fwd", "hupr_k_gcn_adj_bwd", "hupr_k_sigmoid_to_nchw", "hupr_k_sigmoid_to_nchw_bwd", "hupr_k_bce_fwd",
            "hupr_k_bce_bwd", "hupr_k_bce_pair_fwd", "hupr_k_bce_pair_bwd", "hupr_k_gaussian_targets"}
    assert {k for k, v in seen.items() if True in v} == want
    assert all(False in seen[k] for k in want - {"hupr_k_gaussian_targets"})
    # both ld branches of the adjacency forward wrap
    assert {c.route for c in cases("adj_fwd") if True in loop_wraps(c).values()} == {"ld16", "scalar"}
    # the partial pass of the loss just below and just above its 1024 workgroups; the element-wise kernels above 2^20
    ns = {c.p[0] for c in cases("bce")}
    assert ns >= {1, 255, 257, 262144, 262145, 19 * 14 * 4096} == {c.p[0] for c in cases("bce_pair") if c.p[1] == "random"}
    assert 19 * 14 * 4096 > 1 << 20 and 64 * 16385 > 1 << 20 and 64 * 1041 > 1 << 16


def head_wgrad_plan(M):
    """The voxel count of every workgroup of hupr_k_head1x1_wgrad, restated: min(512, ceil(M / 128)) workgroups of ceil(M / grid)."""
    grid = min(512, (M + 127) // 128)
    per = (M + grid - 1) // grid
    return [max(0, min(M, (b + 1) * per) - b * per) for b in range(grid)]


def head_wgrad_kinds(M):
    kinds = set()
    for n in head_wgrad_plan(M):
        if n == 0:
            kinds.add("empty")
            continue
        kinds.add("one chunk" if n <= 128 else "two chunks")
        if n % 128:
            kinds.add("ragged last chunk")
    return kinds


def test_the_head_cases_reach_every_kind_of_workgroup():
    heads = cases("head")
    assert {c.p[0] for c in heads} >= {1, 127, 129, 256, 257, 65537, 65664}
    for M in T.HEAD_M:
        assert {c.p[1] for c in heads if c.p[0] == M and c.p[2] == ""} == {14, 16}, M
    assert {c.p[2] for c in heads} == {"", "dx", "dw"}
    assert {(c.p[1], c.p[2]) for c in heads if c.p[2]} == {(14, "dx"), (14, "dw"), (16, "dx"), (16, "dw")}
    kinds = {M: head_wgrad_kinds(M) for M in T.HEAD_M}
    assert set().union(*kinds.values()) == {"one chunk", "two chunks", "ragged last chunk", "empty"}
    assert kinds[256] == {"one chunk"} and kinds[1] == {"one chunk", "ragged last chunk"}
    assert "two chunks" in kinds[65537] and "ragged last chunk" in kinds[65537]
    # M = 65 664: 512 workgroups of 129 voxels; workgroup 509 holds 3, workgroups 510 and 511 are empty
    plan = head_wgrad_plan(65664)
    assert len(plan) == 512 and plan[:509] == [129] * 509 and plan[509:] == [3, 0, 0] and "empty" in kinds[65664]
    assert sum(plan) == 65664 and all(sum(head_wgrad_plan(M)) == M for M in T.HEAD_M)
    for c in heads:
        assert c.entry == (T.HEAD14 if c.p[1] == 14 else T.HEAD16)


def test_the_remaining_shapes_are_those_where_the_kernels_change_path():
    assert {c.p[1:3] for c in cases("sigmoid")} == {(14, 16), (14, 14), (3, 8)}
    for K, ld in ((14, 16), (14, 14), (3, 8)):
        assert {c.p[3] for c in cases("sigmoid") if c.p[1:3] == (K, ld)} >= {1, 63, 4096}
    assert find("sigmoid", 19, 14, 16, 4096)
    assert set(T.SPECIAL_LOGITS) == {0.0, 20.0, -20.0, 90.0, -90.0} and str(T.SPECIAL_LOGITS[1]) == "-0.0"
    assert all(2 * K * HW >= len(T.SPECIAL_LOGITS) for (_, K, _, HW) in (c.p for c in cases("sigmoid")))
    assert {c.p[0] for c in cases("argmax")} == {1, 63, 64, 65, 4096}
    assert {c.p[:2] for c in cases("softmax") if c.p[2] == 3.0} == {(r, n) for n in (4, 1020, 1024, 1028, 4096) for r in (1, 3)}
    assert any(c.p[2] == 80.0 for c in cases("softmax"))
    for op in ("bce", "bce_pair"):
        assert any(c.p[1] == "saturated" for c in cases(op))
        o = T.make_bce(find(op, 6, "saturated"))
        assert {(p, t) for p, t in zip(o["p1"].tolist(), o["t"].tolist())} == {(p, t) for p in (0.0, 1.0) for t in (0.0, 1.0, 0.5)}
        assert torch.equal(o["p2"], 1 - o["p1"])
    assert find("targets", 19, 14, 64)


def test_the_table_names_every_entry_point_of_the_two_sources(L):
    from hupr_amd import runtime
    csrc = os.path.join(os.path.dirname(runtime.__file__), "csrc")
    entries = set()
    for name in ("head.hip", "gcn_products.hip"):
        with open(os.path.join(csrc, name)) as f:
            entries |= set(re.findall(r'extern "C" int (hupr_\w+)\(', f.read()))
    assert len(entries) == 18 and entries <= set(runtime.SIGNATURES)
    named = {e for c in T.CASES for e in c.entry}
    assert entries <= named, sorted(entries - named)
    assert named - entries == {"hupr_gemm_f32"}
    assert set(T.LAYER_ENTRIES) <= named


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", T.REFUSED, ids=[r[0] for r in T.REFUSED])
def test_refused_calls_are_refused_by_host_checks(r, L):
    """On made-up addresses and without a device: the error comes back before anything is launched or dereferenced."""
    base = 1 << 24
    n0 = L.hupr_launch_count()
    rc = r[1](L, (base, 2 * base, 3 * base, 4 * base))
    assert rc in (T.HUPR_ERR_ARG, T.HUPR_ERR_WORKSPACE), (r[0], rc, L.hupr_last_error())
    assert L.hupr_launch_count() == n0


def test_the_refusals_cover_what_the_launchers_check():
    names = " | ".join(r[0] for r in T.REFUSED)
    for what in ("wx: ld = 14", "dw: ld = 14", "wx: ld = 16, F = 96", "dw: ld = 16, F = 96", "K = 17", "K = 14, ld = 12", "ld = 20",
                 "slices = 0", "slices = 65", "out_rows = 0", "out_rows = 17", "x misaligned", "dy misaligned", "workspace one byte short",
                 "softmax: n = 6", "bce: workspace one byte short"):
        assert what in names, what


def test_a_head_of_no_voxels_is_ok_without_a_launch(L):
    n0 = L.hupr_launch_count()
    assert L.hupr_head1x1_fwd_f32(None, None, None, 0, None) == 0
    assert L.hupr_head1x1_bwd_rows_f32(None, None, None, None, None, 14, 0, None, 0, None) == 0
    assert L.hupr_launch_count() == n0


# ---- gate sensitivity, on CPU fp64 data of the table's own cases ------------------------------------------------------------------------
def accepts(key, got, ref, A):
    A = A if isinstance(A, torch.Tensor) else torch.full_like(ref, A)
    return bool(T.within(got.float(), ref, A, T.GATE_C[key]).all())


def rejects(key, bad, ref, A, what, frac=0.8):
    """bad: faulty fp64 results; stored as fp32 they must fail the gate at >= frac of the outputs the fault touches and nowhere else."""
    A = A if isinstance(A, torch.Tensor) else torch.full_like(ref, A)
    ok = T.within(bad.float(), ref, A, T.GATE_C[key])
    touched = ~(bad == ref)                                        # (a NaN counts as touched)
    n, caught = int(touched.sum()), int((~ok & touched).sum())
    assert n > 0, what
    assert caught >= frac * n and caught >= 1, (what, caught, n)
    assert not bool((~ok & ~touched).any()), what


def test_gates_reject_wrong_products():
    for tw in (0, 1):
        c = find("wx", 192, 5, tw, False)
        o = T.make_wx(c)
        ref, A = T.wx_ref(o["W"], o["x"], tw)
        assert accepts(("wx", "any"), ref, ref, A)
        rejects(("wx", "any"), T.wx_ref(o["W"].t(), o["x"], tw)[0], ref, A, "W transposed (trans_w = %d)" % tw)
        # the last 32-element chunk of the first K half never multiplied
        W = o["W"].clone()
        if tw:
            W[96 - 32:96, :] = 0
        else:
            W[:, 96 - 32:96] = 0
        rejects(("wx", "any"), T.wx_ref(W, o["x"], tw)[0], ref, A, "a chunk dropped (trans_w = %d)" % tw)
        rejects(("wx", "any"), ref.roll(1, 0), ref, A, "samples mixed up (trans_w = %d)" % tw)
        # fp32 accumulation with the reduction axis reversed
        eq = "fg,bfn->bgn" if tw else "fg,bgn->bfn"
        got = torch.einsum(eq, o["W"].flip(0, 1), o["x"].flip(1))
        got = got.flip(1)
        assert got.dtype == torch.float32 and accepts(("wx", "any"), got, ref, A) and bool((got.double() != ref).any())
    # exact-index cases: a transposition is an exact mismatch
    for tw in (0, 1):
        o = T.make_wx(find("wx", 128, 3, tw, True))
        ref, _ = T.wx_ref(o["W"], o["x"], tw)
        assert torch.equal(ref.float().double(), ref) and int((o["W"] != 0).sum()) == 128
        assert not torch.equal(T.wx_ref(o["W"].t(), o["x"], tw)[0], ref) and not torch.equal(ref.roll(1, 0), ref)
    c = find("dw", 64, 7, False)
    o = T.make_dw(c)
    ref, A = T.dw_ref(o["dt"], o["x"])
    assert accepts(("dw", "any"), ref, ref, A)
    rejects(("dw", "any"), ref.t(), ref, A, "dW transposed")
    rejects(("dw", "any"), ref + T.dw_ref(o["dt"][-1:], o["x"][-1:])[0], ref, A, "the masked sample of an odd batch counted")
    rejects(("dw", "any"), ref - T.dw_ref(o["dt"][4:6], o["x"][4:6])[0], ref, A, "a pair of samples dropped")
    got = torch.einsum("bfn,bgn->fg", o["dt"].flip(0, 2), o["x"].flip(0, 2))
    assert got.dtype == torch.float32 and accepts(("dw", "any"), got, ref, A)
    o = T.make_dw(find("dw", 128, 3, True))
    ref, _ = T.dw_ref(o["dt"], o["x"])
    assert torch.equal(ref.float().double(), ref) and not torch.equal(ref.t(), ref)
    assert not torch.equal(ref + T.dw_ref(o["dt"][-1:], o["x"][-1:])[0], ref)


def test_gates_reject_wrong_adjacency_epilogues():
    for kind, frac in (("dense", 0.8), ("model", 0.8)):
        for K, ld in ((14, 16), (14, 14)):
            c = find("adj_fwd", 64, 3, K, ld, 0, kind)
            o = T.make_adj(c)
            key = ("adj_fwd", c.route)
            ref, A = T.adj_fwd_ref(o["t"], o["adj"], o["bias"], K, 0)
            assert accepts(key, ref, ref, A)
            rejects(key, T.adj_fwd_ref(o["t"], o["adj"].t(), o["bias"], K, 0)[0], ref, A, "adjacency transposed, forward", frac)
            bias_kf = o["bias"].reshape(-1).view(K, 64).t()            # bias[k * F + f] where bias[f * K + k] is meant
            rejects(key, T.adj_fwd_ref(o["t"], o["adj"], bias_kf, K, 0)[0], ref, A, "bias indexed [k][f]")
            got = (torch.einsum("bfk,kj->bfj", o["t"][..., :K].flip(2), o["adj"].flip(0)) + o["bias"])
            assert got.dtype == torch.float32 and accepts(key, got, ref, A)
            cb = find("adj_bwd", 64, 3, K, ld, 1, kind)
            ob = T.make_adj(cb)
            g, (ref, A), (bref, bA) = T.adj_bwd_ref(ob["dy"], ob["y"], ob["adj"], K, 1)
            assert accepts(("adj_bwd", "any"), ref, ref, A) and accepts(("dbias", "any"), bref, bref, bA)
            rejects(("adj_bwd", "any"), T.adj_bwd_ref(ob["dy"], ob["y"], ob["adj"].t(), K, 1)[1][0], ref, A,
                    "adjacency transposed, backward", frac)
            # the ReLU mask taken from dy > 0: another g (compared exactly), another dt, another dbias
            gbad, (bad, _), (bbad, _) = T.adj_bwd_ref(ob["dy"], ob["dy"], ob["adj"], K, 1)
            assert not torch.equal(gbad, g)
            rejects(("adj_bwd", "any"), bad, ref, A, "mask from dy")
            rejects(("dbias", "any"), bbad, bref, bA, "mask from dy, dbias")
            # y >= 0 instead of y > 0 shows at the exact zeros
            g0 = ob["dy"].double()[..., :K] * (ob["y"][..., :K] >= 0)
            assert not torch.equal(g0, g)
            got = g.float().flip(0).sum(0)
            assert accepts(("dbias", "any"), got, bref, bA)
    c = find("adj_sliced", 64, 3, 14, 16, 1, "dense", 8)
    o = T.make_adj(c)
    ref, A = T.adj_fwd_ref(o["t"], o["adj"], o["bias"], 14, 1)
    key = ("adj_sliced", "ld16")
    assert accepts(key, ref, ref, A)
    rejects(key, T.adj_fwd_ref(o["t"][:7], o["adj"], o["bias"], 14, 1)[0], ref, A, "the last K slice dropped", 0.7)
    rejects(key, T.adj_fwd_ref(o["t"][1:], o["adj"], o["bias"], 14, 1)[0], ref, A, "the first K slice dropped", 0.7)
    got = torch.relu(torch.einsum("bfk,kj->bfj", o["t"].flip(0).sum(0)[..., :14], o["adj"]) + o["bias"])
    assert got.dtype == torch.float32 and accepts(key, got, ref, A)


def test_gates_reject_wrong_heads_and_losses():
    c = find("head", 257, 14, "")
    o = T.make_head(c)
    (y, yA), (dx, dxA), (dw, dwA) = T.head_ref(o["x"], o["w"], o["dy"], 14)
    for key, ref, A in ((("head_fwd", "any"), y, yA), (("head_dgrad", "any"), dx, dxA), (("head_wgrad", "any"), dw, dwA)):
        assert accepts(key, ref, ref, A)
    rejects(("head_wgrad", "any"), dw - T.head_ref(o["x"][256:], o["w"], o["dy"][256:], 14)[2][0], dw, dwA, "the ragged chunk dropped")
    rejects(("head_wgrad", "any"), dw.flip(0), dw, dwA, "filters reversed")
    rejects(("head_fwd", "any"), y[:, :14].flip(1), y[:, :14], yA[:, :14], "channels reversed")
    got = (o["dy"][:, :14].flip(0).t() @ o["x"].flip(0))
    assert got.dtype == torch.float32 and accepts(("head_wgrad", "any"), got, dw, dwA)
    # sigmoid head: two heat-map channels exchanged in the NCHW transposition
    c = find("sigmoid", 2, 14, 16, 63)
    o = T.make_sigmoid(c)
    ref = T.sigmoid_ref(o["x"], 14)
    assert accepts(("sigmoid", "any"), ref, ref, 1.0)
    bad = ref.clone()
    bad[:, 2], bad[:, 3] = ref[:, 3], ref[:, 2]
    rejects(("sigmoid", "any"), bad, ref, 1.0, "channels 2 and 3 exchanged")
    assert accepts(("sigmoid", "any"), torch.sigmoid(o["x"][..., :14]).permute(0, 2, 1), ref, 1.0)
    # losses
    for op in ("bce", "bce_pair"):
        o = T.make_bce(find(op, 257, "random"))
        ref, A = T.bce_ref(o["p1"], o["t"])
        assert float(A) <= 1.0 and accepts(("bce", "any"), ref, ref, A)
        rejects(("bce", "any"), ref * 257 / 258, ref, A, "the mean over n + 1")
        gref = T.bce_grad_ref(o["p1"], o["t"], T.G_OUT)
        assert accepts(("bce_bwd", "any"), gref, gref, gref.abs())
        rejects(("bce_bwd", "any"), gref * 257 / 258, gref, gref.abs(), "the gradient's mean over n + 1")
        got = torch.nn.functional.binary_cross_entropy(o["p1"].flip(0), o["t"].flip(0))
        assert got.dtype == torch.float32 and accepts(("bce", "any"), got.view(1), ref, A)
        o = T.make_bce(find(op, 257, "saturated"))
        ref, A = T.bce_ref(o["p1"], o["t"])
        assert bool(ref.isfinite()) and accepts(("bce", "any"), ref, ref, A)
        p, t = o["p1"].double(), o["t"].double()
        unclamped = -(t * torch.log(p) + (1 - t) * torch.log(1 - p)).mean().view(1)
        assert not accepts(("bce", "any"), unclamped, ref, A)                                      # inf or NaN
        clamped_late = -(t * torch.log(p) + (1 - t) * torch.log(1 - p)).nan_to_num(0.0, 100.0, -100.0).mean().view(1)
        assert not accepts(("bce", "any"), clamped_late, ref, A)
        gref = T.bce_grad_ref(o["p1"], o["t"], T.G_OUT)
        unfloored = T.G_OUT * (p - t) / (p * (1 - p)) / 257
        assert bool(gref.isfinite().all()) and not accepts(("bce_bwd", "any"), unfloored, gref, gref.abs())


def test_arg_max_expectations_tell_the_first_tie_from_the_last_and_skip_nan():
    for c in cases("argmax"):
        o = T.make_argmax(c)
        p = o["p"]
        clean = torch.where(p.isnan(), torch.full_like(p, float("-inf")), p)
        mx = clean.max(dim=1, keepdim=True).values
        n = p.shape[1]
        first = (clean == mx).float().argmax(dim=1).int()
        last = (n - 1 - (clean == mx).flip(1).float().argmax(dim=1)).int()
        assert torch.equal(o["idx"], first)
        assert int(o["idx"][-1]) == 0 and bool((p[-1] == float("-inf")).all())              # all -inf: index 0
        assert not bool(p.isnan().all(dim=1).any())                                         # (no all-NaN row)
        if n >= 2:
            assert not torch.equal(last, o["idx"]), n                                       # the last of several ties is another answer
            nan_rows = p.isnan().any(dim=1)
            assert bool(nan_rows.any()) and bool((o["idx"][nan_rows] == 1).all())
        if n > 64:
            ties = [(clean[r] == mx[r]).nonzero().view(-1).tolist() for r in range(p.shape[0] - 1)]
            assert any(len(t) >= 2 and len({i % 64 for i in t}) == 1 for t in ties)         # inside one lane
            assert any(len({i % 64 for i in t}) >= 2 for t in ties)                         # across lanes


def test_softmax_gate_rejects_an_unshifted_or_unnormalised_row():
    c = find("softmax", 3, 1028, 80.0)
    o = T.make_softmax(c)
    ref = T.softmax_ref(o["x"])
    rowmax = ref.max(dim=1, keepdim=True).values.expand_as(ref)
    assert accepts(("softmax", "any"), ref, ref, rowmax)
    assert accepts(("softmax", "any"), torch.softmax(o["x"], dim=1), ref, rowmax)
    assert not accepts(("softmax", "any"), torch.exp(o["x"]) / torch.exp(o["x"]).sum(1, keepdim=True), ref, rowmax)   # overflow: NaN
    o = T.make_softmax(find("softmax", 3, 1028, 3.0))
    ref = T.softmax_ref(o["x"])
    rowmax = ref.max(dim=1, keepdim=True).values.expand_as(ref)
    assert accepts(("softmax", "any"), torch.softmax(o["x"], dim=1), ref, rowmax)
    partial = torch.exp(o["x"].double() - o["x"].double().max(1, keepdim=True).values)
    rejects(("softmax", "any"), partial / partial[:, :1024].sum(1, keepdim=True), ref, rowmax, "the last float4 missing from the sum", 0.01)
    gref, A = T.softmax_bwd_ref(ref.float(), o["dp"])
    assert accepts(("softmax_bwd", "any"), gref, gref, A)
    rejects(("softmax_bwd", "any"), ref.float().double() * o["dp"].double(), gref, A, "the dot product missing", 0.01)
