"""CPU (no GPU needed): the two-plane form of the 2 x 8 x 16 tile (depth-2 layers, hupr_debug_halo_two_plane) is a choice of the
launcher behind unchanged route codes — with the switch on and off the depth-2 cases of test_conv_halo_two_plane_gpu.py route to
the 2 x 8 x 16 tile (8; 6 with fused statistics), and a D = 6 case (interior depth tiles: always the four-plane form) to 8."""
import pytest

import test_conv_halo_fp64_gpu as H
import test_conv_halo_two_plane_gpu as G


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    L = runtime.lib()
    L.hupr_debug_halo_tiles(31)
    L.hupr_debug_halo_variant(0)
    return L


def test_case_table_names_the_expected_routes():
    assert H.T2X8X16 == 8 and H.STATS_2X8X16 == 6
    assert all(c.D == 2 and c.route == (H.STATS_2X8X16 if c.act == "stats" else H.T2X8X16) for c in G.D2_CASES)
    assert G.D6_CASE.D == 6 and G.D6_CASE.route == H.T2X8X16


@pytest.mark.parametrize("on", [1, 0])
def test_routes_do_not_depend_on_the_switch(on, L):
    try:
        L.hupr_debug_halo_two_plane(on)
        for c in G.D2_CASES + [G.D6_CASE]:
            assert H.route_of(L, c) == c.route, (on, H.case_id(c))
    finally:
        L.hupr_debug_halo_two_plane(1)
