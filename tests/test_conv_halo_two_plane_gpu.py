"""GPU (-m gpu): the two-plane form of the 256-voxel kernel's 2 x 8 x 16 tile (depth-2 layers: the tile spans the depth, the halo
image holds the two real planes, six stages instead of nine) against the general four-plane instantiation it replaces
(hupr_debug_halo_two_plane(0)) — bit for bit: the dropped MFMAs only added the products of the zero padding planes — and against
fp64 under the gate of test_conv_halo_fp64_gpu.py.  The shapes are the smallest that reach the kernel (256 tiles; exactly 256 with
fused statistics): one / two / four channel chunks, one and two tiles per workgroup (next-halo prefetch, park and store), bias on the
deferred epilogue, residual on the immediate one, both statistics geometries; D = 6 stays on the four-plane form."""
import pytest
import torch

import test_conv_halo_fp64_gpu as H
from test_conv_halo_fp64_gpu import Case, operands, launch, conv_ref, assert_within, bits, view, lds, items

pytestmark = pytest.mark.gpu

D2_CASES = [
    Case(64, 64, 64, 2, 16, 32, 3, "bf16", "bias", H.S, H.T2X8X16),
    Case(33, 128, 128, 2, 16, 32, 3, "bf16", "", H.S, H.T2X8X16),
    Case(32, 256, 256, 2, 16, 16, 3, "bf16", "res", H.I, H.T2X8X16),
    Case(32, 128, 256, 2, 16, 16, 3, "stats", "", H.S, H.STATS_2X8X16),
    Case(16, 64, 128, 2, 32, 32, 3, "stats", "", H.S, H.STATS_2X8X16),
]
D6_CASE = Case(11, 64, 256, 6, 16, 16, 3, "bf16", "", H.S, H.T2X8X16)


@pytest.fixture
def lib():
    from hupr_amd import functional as F_
    L = F_.rt.lib()
    try:
        yield L
    finally:
        L.hupr_debug_halo_two_plane(1)


def run(L, c, ops, on):
    """One launch with the switch at `on`: (output buffer, output bits of the Co columns, statistics or None)."""
    dt, x, wq, wp, bias, res = ops
    _, out_ld, _ = lds(c)
    try:
        L.hupr_debug_halo_two_plane(on)
        assert H.route_of(L, c) == c.route
        rc, yb, st = launch(c, dt, x, wp, bias, res)
    finally:
        L.hupr_debug_halo_two_plane(1)
    assert rc == 0, L.hupr_last_error()
    H.assert_padding_untouched(yb, c, out_ld)          # NaN padding columns and the guard tail: NaN bit for bit
    return yb, bits(view(yb, c, out_ld)[..., :c.Co].cpu()), st


def fp64_gate(c, ops, yb, what):
    dt, x, wq, wp, bias, res = ops
    _, out_ld, _ = lds(c)
    y = view(yb, c, out_ld)[..., :c.Co].cpu()
    sel = items(c.B)
    ref, A = conv_ref(x[sel], wq, bias.cpu() if bias is not None else None, res[sel] if res is not None else None, c.kd)
    assert_within(y[sel], ref, A, True, what)
    return y


@pytest.mark.parametrize("c", D2_CASES, ids=[H.case_id(c) for c in D2_CASES])
def test_two_plane_form_stores_the_bits_of_the_four_plane_form(c, lib):
    ops = operands(c, seed=c.B * 131 + c.Ci + c.Co)
    yb_on, y_on, st_on = run(lib, c, ops, 1)
    yb_off, y_off, st_off = run(lib, c, ops, 0)
    assert torch.equal(y_on, y_off), "two-plane and four-plane outputs differ in %d elements" % (y_on != y_off).sum().item()
    y = fp64_gate(c, ops, yb_on, "%s (two-plane form)" % H.case_id(c))
    _, y_on2, st_on2 = run(lib, c, ops, 1)
    assert torch.equal(y_on2, y_on), "two launches of the two-plane form differ"
    if c.act == "stats":
        assert torch.equal(st_on, st_off), "per-workgroup statistics partials differ between the forms"
        assert torch.equal(st_on, st_on2)
        tot = st_on.sum(0).cpu()
        yd = y.double().reshape(-1, c.Co)
        s, q = yd.sum(0), (yd * yd).sum(0)
        assert bool(((tot[0] - s).abs() <= 2.0 ** -20 * yd.abs().sum(0)).all()), "fused column sums"
        assert bool(((tot[1] - q).abs() <= 2.0 ** -20 * q).all()), "fused sums of squares"


def test_depth_six_stays_on_the_four_plane_form(lib):
    """D = 6: three depth tiles per column, the middle one with real planes on both sides — the launcher keeps the four-plane
    instantiation whatever the switch says."""
    c = D6_CASE
    ops = operands(c, seed=c.B * 131 + c.Ci + c.Co)
    yb_on, y_on, _ = run(lib, c, ops, 1)
    _, y_off, _ = run(lib, c, ops, 0)
    assert torch.equal(y_on, y_off)
    fp64_gate(c, ops, yb_on, "%s (four-plane form)" % H.case_id(c))
