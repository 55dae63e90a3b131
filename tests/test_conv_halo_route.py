"""CPU (no GPU needed): the dispatch of the halo convolution (hupr_debug_halo_route, host code only) sends every case of the
fp64 table (test_conv_halo_fp64_gpu.py) and of the kernel-parity tests (test_ops_gpu.py) to the instantiation the case names —
a change of the dispatch rules that silently moves a case fails here — and the fp64 gate of those tests rejects a result that
lacks one (tap, 8-channel) product slice or carries one wrong bias channel."""
import pytest
import torch

import test_conv_halo_fp64_gpu as H
import test_ops_gpu as O


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    L = runtime.lib()
    L.hupr_debug_halo_tiles(31)
    L.hupr_debug_halo_variant(0)
    return L


@pytest.mark.parametrize("c", H.CASES, ids=[H.case_id(c) for c in H.CASES])
def test_fp64_case_table_routes(c, L):
    assert H.route_of(L, c) == c.route


def test_parity_test_cases_reach_the_forms_they_name(L):
    for shape, route in O.HALO256M_4X8X8_CASES:
        B, Ci, Co, D, H_, W = shape
        assert O.halo_route(L, B, Ci, Co, D, H_, W, 3) == route == H.T4X8X8, shape
    for shape, route in O.HALO256M_CO32_CASES:
        B, Ci, D, H_, W = shape
        assert O.halo_route(L, B, Ci, 32, D, H_, W, 3) == route == H.CO32, shape
    for shape, route in O.HALO256M_TWO_SLICE_CASES:
        B, Ci, Co, D, H_, W = shape
        assert O.halo_route(L, B, Ci, Co, D, H_, W, 3 if D > 1 else 1) == route, shape
        assert route in (H.T2X8X16, H.T1X16X16)
    for shape, route in O.RESIDUAL_PREFETCH_CASES:
        B, Ci, Co, D, H_, W, kd = shape
        assert O.halo_route(L, B, Ci, Co, D, H_, W, kd) == route, shape
        assert route in (H.T4X8X8, H.T1X16X16, H.T2X8X16)
    for shape, route in O.FIRST_LAYER_CASES:
        B, Co, D, H_, W, _ = shape
        assert O.halo_route(L, B, 32, Co, D, H_, W, 3) == route == H.CI32, shape


def test_parity_test_comparison_modes_leave_the_256_voxel_kernel(L):
    """The masks the parity tests clear send their cases to the 128-voxel kernel (the other side of each comparison)."""
    try:
        for mask, cases in ((0, [(s, 3) for s, _ in O.HALO256M_4X8X8_CASES]),
                            (1, [(s, 3 if s[3] > 1 else 1) for s, _ in O.HALO256M_TWO_SLICE_CASES])):
            L.hupr_debug_halo_tiles(mask)
            for (B, Ci, Co, D, H_, W), kd in cases:
                assert O.halo_route(L, B, Ci, Co, D, H_, W, kd) >= 256, (mask, B, Ci, Co, D, H_, W)
        L.hupr_debug_halo_tiles(7)
        for (B, Ci, D, H_, W), _ in O.HALO256M_CO32_CASES:
            assert O.halo_route(L, B, Ci, 32, D, H_, W, 3) >= 256
        L.hupr_debug_halo_tiles(15)
        for (B, Co, D, H_, W, _), _ in O.FIRST_LAYER_CASES:
            assert O.halo_route(L, B, 32, Co, D, H_, W, 3) >= 256
    finally:
        L.hupr_debug_halo_tiles(31)


@pytest.mark.parametrize("r", [r for r in H.REFUSED if not r[11]], ids=[r[0] for r in H.REFUSED if not r[11]])
def test_refused_calls_route_to_an_argument_error(r, L):
    what, B, Ci, Co, D, H_, W, kd, in_ld, out_ld, res_ld, has_res, stats = r
    assert L.hupr_debug_halo_route(B, D, H_, W, Ci, in_ld, Co, out_ld, kd, 1, int(stats), 0) == H.HUPR_ERR_ARG, what


def _case_operands(seed=5):
    B, Ci, Co, D, H_, W = 2, 64, 64, 4, 8, 8
    x = H.rnd(B, D, H_, W, Ci, seed=seed).to(torch.bfloat16).float()
    w = H.rnd(Co, Ci, 3, 3, 3, seed=seed + 1, scale=(Ci * 27) ** -0.5).to(torch.bfloat16).float()
    bias = H.rnd(Co, seed=seed + 2)
    res = H.rnd(B, D, H_, W, Co, seed=seed + 3).to(torch.bfloat16).float()
    return x, w, bias, res


@pytest.mark.parametrize("bf16_store", [True, False])
def test_fp64_gate_rejects_a_dropped_product_slice_and_a_wrong_bias_channel(bf16_store):
    """A faithful result (the fp64 sum rounded once to the storage type) passes the gate; the same with one (tap, 8-channel) slice of
    products missing, or with one bias channel negated, fails it: the slice at most of the outputs it touches (a sum of eight products
    can be near zero), the bias channel at every output of that channel and nowhere else."""
    x, w, bias, res = _case_operands()
    ref, A = H.conv_ref(x, w, bias, res, 3)
    store = (lambda t: t.to(torch.bfloat16).double()) if bf16_store else (lambda t: t.float().double())
    assert bool(H.within_bound(store(ref), ref, A, bf16_store).all())
    # one (tap, 8-channel) slice missing: tap (kz, ky, kx) = (1, 0, 2), input channels 16 .. 23
    w_drop = w.clone()
    w_drop[:, 16:24, 1, 0, 2] = 0
    bad, _ = H.conv_ref(x, w_drop, bias, res, 3)
    ok = H.within_bound(store(bad), ref, A, bf16_store)
    touched = (bad - ref).abs() > 0
    assert not bool(ok.all())
    assert (~ok & touched).sum().item() >= 0.8 * touched.sum().item() and not bool((~ok & ~touched).any())
    # one bias channel with the wrong sign
    ch = int(bias.abs().argmax())
    b_flip = bias.clone()
    b_flip[ch] = -b_flip[ch]
    bad, _ = H.conv_ref(x, w, b_flip, res, 3)
    ok = H.within_bound(store(bad), ref, A, bf16_store)
    assert not bool(ok[..., ch].any()) and bool(ok[..., :ch].all()) and bool(ok[..., ch + 1:].all())
