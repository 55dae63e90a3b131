"""CPU (no GPU needed): the attention launchers' one routing decision (hupr_attn_route, host code only) sends every case of the fp64
table (test_attn_fp64_gpu.py) and the attention cases of test_ops_gpu.py to the kernels they name — a change of the dispatch rules
that silently moves a case fails here — and the fp64 gate of the table rejects results of subtly wrong kernels while it accepts the
bf16 roundings of P and dS that correct kernels make."""
import pytest
import torch

import test_attn_fp64_gpu as A
import test_ops_gpu as O

FWD, DKV = 3, 12


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    L = runtime.lib()
    L.hupr_debug_attn_split(0)
    return L


@pytest.mark.parametrize("c", A.CASES, ids=[A.case_id(c) for c in A.CASES])
def test_fp64_case_table_routes(c, L):
    try:
        L.hupr_debug_attn_split(c.split or 0)
        assert A.route_of(L, c) == c.route
    finally:
        L.hupr_debug_attn_split(0)


@pytest.mark.parametrize("c", A.BATCH_CASES, ids=[A.batch_id(c) for c in A.BATCH_CASES])
def test_fp64_batch_table_routes(c, L):
    assert A.batch_route_of(L, c) == c.route
    assert A.expected_bwd_launches(c) == 2 + (c.n if c.route & DKV == A.DKV512 else A.ROUNDS[c.n])


def test_fp64_tables_reach_every_route(L):
    """Each forward kernel, each dK / dV kernel and xmap, in the single and in the batch table; both plain and QS forms; every
    item count of the batch entries; the tiling edges N = 128, 384, 1024, 4096; Bn = 1, 3, 8; C = 64, 128, 256."""
    for table in (A.CASES, A.BATCH_CASES):
        routes = {c.route for c in table}
        assert {r & FWD for r in routes} == {A.PP64, A.ONE_PASS, A.SPLIT}
        assert {r & DKV for r in routes} == {A.DKV512, A.NH1, A.NH2}
        assert any(r & A.XMAP for r in routes) and not all(r & A.XMAP for r in routes)
        assert {c.C for c in table} == {64, 128, 256}
    assert {c.fwd for c in A.CASES} == {"f32", "bf16in", "ld", "ld_ws", "ld_ws_qs"}
    assert {c.bwd for c in A.CASES} == {"dout32", "bf16", "acc"}
    assert {(c.residual, c.bwd) for c in A.CASES if c.fwd.startswith("ld")} >= {(True, "dout32"), (True, "bf16"), (False, "acc")}
    assert {c.regime for c in A.CASES} == {"mild", "peaky", "moving", "zero"}
    assert {c.split for c in A.CASES} == {None, 0, 1, -1}
    assert {c.N for c in A.CASES} >= {128, 384, 1024, 4096} and {c.B for c in A.CASES} >= {1, 3, 8}
    assert any(c.N == 4096 and c.B == 2 and c.route & FWD == A.PP64 and c.route & DKV == A.DKV512 for c in A.CASES)
    assert {c.n for c in A.BATCH_CASES} == {1, 2, 3, 4} and {c.qs for c in A.BATCH_CASES} == {True, False}
    assert {c.B for c in A.BATCH_CASES} >= {1, 3, 8}


def test_parity_test_cases_reach_the_forms_they_name(L):
    """test_flash_attention_qs_kernels_vs_fp64: (2, 4096, 64) and (8, 512, 64) take the ping-pong forward and the 512-thread dK / dV
    kernel, (2, 384, 64) the generic D = 64 kernels, the others levels 2 and 3; the deferred-maximum case the ping-pong forward; the
    split-key cases the key-split forward (test_attention_qs_split_keys: default policy; test_attention_split_keys_matches_plain_forward:
    under hupr_debug_attn_split(1) with a workspace, and without one the one-pass forms it compares against)."""
    for B, N, C, _ in O.QS_FP64_CASES:
        r = L.hupr_attn_route(B, N, C, C, 1, 0)
        if (B, N, C) in ((2, 4096, 64), (8, 512, 64)):
            assert r & FWD == A.PP64 and r & DKV == A.DKV512, (B, N, C)
        elif (B, N, C) == (2, 384, 64):
            assert r & FWD == A.ONE_PASS and r & DKV == A.NH1, (B, N, C)
        else:
            assert C in (128, 256) and r & FWD == A.ONE_PASS and r & DKV == (A.NH1 if C == 128 else A.NH2), (B, N, C)
    B, N, C = O.DEFERRED_MAXIMUM_SHAPE
    assert L.hupr_attn_route(B, N, C, C, 1, 0) & FWD == A.PP64
    for B, N, C in O.QS_SPLIT_KEYS_CASES:
        r = L.hupr_attn_route(B, N, C, C, 1, 1)
        assert r & FWD == A.SPLIT and r >> 8 > 1, (B, N, C)
    try:
        L.hupr_debug_attn_split(1)
        for B, N, C in O.SPLIT_KEYS_CASES:
            assert L.hupr_attn_route(B, N, C, C, 1, 1) & FWD == A.SPLIT, (B, N, C)
            assert L.hupr_attn_route(B, N, C, C, 1, 0) & FWD != A.SPLIT, (B, N, C)
    finally:
        L.hupr_debug_attn_split(0)


def test_route_refuses_what_the_launchers_refuse(L):
    for B, N, C, ldk in ((2, 192, 64, 64), (2, 256, 96, 96), (2, 256, 64, 68), (2, 256, 64, 56), (0, 256, 64, 64), (2, 64, 64, 64)):
        assert L.hupr_attn_route(B, N, C, ldk, 1, 0) == A.HUPR_ERR_ARG, (B, N, C, ldk)
    assert L.hupr_attn_route(2, 512, 64, 64, 0, 0) == A.route(A.ONE_PASS, A.NH1)        # fp32 operands: never the level-1 kernels
    assert L.hupr_attn_route(2, 1 << 20, 64, 1024, 1, 0) & FWD == A.ONE_PASS             # K beyond 32-bit offsets: not the ping-pong kernel


# ---- the gate rejects subtly wrong results -------------------------------------------------------------------------------
def _fake_case(N=256, C=64, seed=3):
    o = A.operands(1, N, C, "peaky", seed, True)
    r = A.reference(o["kb"][0], o["qr"][0], o["vb"][0], o["gb"][0], keep=True)
    assert r["smax"].max().item() > 20.0             # peaky: single key tiles dominate
    return o, r


def _ok(got, ref, A_, c, terms=(), U=0.0):
    return bool(A.within_gate(got, ref, A_, c, terms, U).all())


def test_gate_accepts_bf16_rounded_probabilities_and_score_gradients():
    """The reference with every P and dS rounded to bf16 (what the kernels feed the matrix pipe) passes: the bound is not tighter than
    legitimate rounding."""
    o, r = _fake_case()
    Pb = r["P"].bfloat16().double()
    dSb = (Pb * (r["dP"] - r["D"])).bfloat16().double()
    assert _ok(Pb.T @ r["v"], r["out"], r["A_out"], A.C_OUT, (), r["U_out"])
    assert _ok(Pb @ r["g"], r["dV"], r["A_dV"], A.C_DV, (), r["U_dV"])
    assert _ok(dSb.T @ r["k"], r["dQ"], r["A_dQ"], A.C_DQ, (), r["U_dQ"])
    assert _ok(dSb @ r["q"], r["dK"], r["A_dK"], A.C_DK, (), r["U_dK"])
    dv0 = A.rnd(*r["dV"].shape, seed=9).double()
    assert _ok(dv0 + Pb @ r["g"] + r["g"], dv0 + r["dV"] + r["g"], r["A_dV"], A.C_DV, U=r["U_dV"], terms=[dv0, r["g"]])


def test_gate_rejects_a_query_row_missing_its_dominant_key_tile():
    o, r = _fake_case()
    k0 = 37
    tiles = r["P"][:, k0].view(-1, 64).sum(1)
    t = int(tiles.argmax())
    p = r["P"][:, k0].clone()
    p[64 * t:64 * (t + 1)] = 0
    p = p / p.sum()                                   # the online softmax never saw the tile: renormalised over the others
    bad = r["out"].clone()
    bad[k0] = p @ r["v"]
    ok = A.within_gate(bad, r["out"], r["A_out"], A.C_OUT, (), r["U_out"])
    assert not bool(ok[k0].all()) and bool(ok[:k0].all()) and bool(ok[k0 + 1:].all())


def test_gate_rejects_swapped_log_sum_exps():
    """The lse of two query rows exchanged before the backward: P = exp(s - lse) is then wrong in both rows."""
    o, r = _fake_case()
    a, b = 10, 200
    lse = r["lse"].clone()
    lse[[a, b]] = lse[[b, a]]
    P = torch.exp(r["s"] - lse)
    dS = P * (r["dP"] - r["D"])
    assert not _ok(dS.T @ r["k"], r["dQ"], r["A_dQ"], A.C_DQ, (), r["U_dQ"])
    assert not _ok(dS @ r["q"], r["dK"], r["A_dK"], A.C_DK, (), r["U_dK"])


def test_gate_rejects_dk_missing_one_query_tile():
    o, r = _fake_case()
    keep = torch.ones(r["q"].shape[0], dtype=torch.bool)
    keep[128:192] = False
    bad = r["dS"][:, keep] @ r["q"][keep]
    assert not _ok(bad, r["dK"], r["A_dK"], A.C_DK, (), r["U_dK"])


def test_gate_rejects_wrong_dv_epilogues():
    """A residual dV without its dO term, and an accumulating dV that overwrote what was in place instead of adding to it."""
    o, r = _fake_case()
    assert not _ok(r["dV"], r["dV"] + r["g"], r["A_dV"], A.C_DV, U=r["U_dV"], terms=[r["g"]])
    dv0 = A.rnd(*r["dV"].shape, seed=9).double()
    assert not _ok(r["dV"], dv0 + r["dV"], r["A_dV"], A.C_DV, U=r["U_dV"], terms=[dv0])
