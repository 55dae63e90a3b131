"""CPU (no GPU needed): the dispatch of the halo-tiled weight gradient (hupr_debug_wgrad_route, host code only) sends every case
of the fp64 table (test_wgrad_halo_fp64_gpu.py) and of the kernel-parity tests (test_ops_gpu.py) to the instantiation, grid and
partial-tensor count the case names — a change of the dispatch rules that silently moves a case fails here; refused calls return
their error; hupr_conv3x3_wgrad_halo_ws_bytes is always enough; and the fp64 gate of that table rejects sums that lack one voxel or
one K-step, exchange two channels or read a halo row across a batch border."""
import ctypes

import pytest
import torch

import test_ops_gpu as O
import test_wgrad_halo_fp64_gpu as G


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    L = runtime.lib()
    L.hupr_debug_wgrad_m16(1)
    L.hupr_debug_wgrad_ci32(1)
    return L


@pytest.mark.parametrize("c", G.CASES, ids=[G.case_id(c) for c in G.CASES])
def test_fp64_case_table_routes(c, L):
    assert G.route_of(L, c) == (c.route, c.groups)


@pytest.mark.parametrize("c", G.DUAL_CASES, ids=[G.case_id(c) for c in G.DUAL_CASES])
def test_fp64_dual_case_table_routes(c, L):
    assert G.route_of(L, c, dual=True) == (c.route, c.groups)
    assert G.route_of(L, c) == (c.route - G.DUAL, c.groups)            # the single calls it is compared with: the same plan
    n = c.Co * c.Ci * c.kd * 9 * 4
    assert G.route_of(L, c, dual=True, ws_bytes=2 * n - 1) == (G.HUPR_ERR_WORKSPACE, 0)
    assert G.route_of(L, c, dual=True, ws_bytes=2 * n)[1] == 1


def test_the_table_reaches_every_instantiation_on_padded_rows():
    """Every kernel instantiation appears in the table, dense and with padded rows; both grids and the dual launch too."""
    for k in range(1, 12):
        hits = [c for c in G.CASES if c.route & 15 == k]
        assert hits and any(c.pad != G.P for c in hits), G.ROUTE_NAMES[k]
        if k < G.REG_BF16_2D:
            assert any(c.pad == G.P for c in hits), G.ROUTE_NAMES[k]
    assert any(c.route & G.XCD and c.pad != G.P for c in G.CASES) and any(c.route & G.XCD for c in G.DUAL_CASES)
    assert any(c.pad != G.P for c in G.DUAL_CASES)


def _shapes(test):
    (mark,) = [m for m in test.pytestmark if m.name == "parametrize"]
    assert mark.args[0] == "shape"
    return mark.args[1]


def _route(L, shape, mode=None, dual=False):
    c = G.Case(*shape, "bf16", G.P, "full", mode, 0, 0)
    return G.route_of(L, c, dual=dual)


def test_parity_tests_reach_the_kernels_they_name(L):
    """The shapes of the weight-gradient tests of test_ops_gpu.py reach the kernels their names and docstrings claim, under the
    modes they set."""
    # the 16 x 16 x 32 kernel against the 32 x 32 x 16 one (two K halves, Ci > 32 or below the K-quarter threshold)
    seen = set()
    for s in _shapes(O.test_wgrad_halo_on_16x16x32_matches_the_32x32x16_kernel_and_fp64):
        r1, g1 = _route(L, s)
        r0, g0 = _route(L, s, mode=(0, 1))
        assert r1 & 15 == (G.M16_3D if s[6] == 3 else G.M16_2D), s
        assert r0 & 15 == (G.GLDS_3D if s[6] == 3 else G.GLDS_2D), s
        assert (r1 & ~15, g1) == (r0 & ~15, g0), s            # the same grid and partial tensors: only the kernel differs
        seen.add(r1)
    assert {G.M16_3D, G.M16_3D + G.XCD, G.M16_2D} <= seen     # "level-1 shape at the bench batch" (XCD grid), small 3-D, 2-D
    assert _route(L, (1, 64, 64, 2, 8, 8, 3)) == (G.M16_3D, 1)      # "a single tile per workgroup"
    # Ci <= 32: K halves (mode 0), K quarters on the 16 x 16 x 32 kernel (mode 2, 3-D taps only), on the 32 x 32 x 16 kernel (mode 3)
    for s in _shapes(O.test_wgrad_k_quarter_mode_for_narrow_inputs):
        d3 = s[6] == 3
        assert _route(L, s, mode=(1, 0))[0] & 15 == (G.M16_3D if d3 else G.M16_2D), s
        assert _route(L, s, mode=(1, 2))[0] & 15 == (G.M16_KQ if d3 else G.GLDS_2D_KQ), s
        assert _route(L, s, mode=(1, 3))[0] & 15 == (G.GLDS_3D_KQ if d3 else G.GLDS_2D_KQ), s
        assert len({_route(L, s, mode=(1, m))[1] for m in (0, 2, 3)}) == 1, s
    # two gradients in one launch: the single calls' plan + the dual bit; the XCD-aware grid and the K-quarter kernel are among them
    seen = set()
    for s in _shapes(O.test_two_weight_gradients_of_one_input_in_one_launch):
        r1, g1 = _route(L, s)
        r2, g2 = _route(L, s, dual=True)
        assert (r2, g2) == (r1 + G.DUAL, g1) and r1 & 15 in (G.M16_3D, G.M16_2D, G.M16_KQ), s
        seen.add(r1)
    assert _route(L, (8, 64, 64, 8, 32, 32, 3))[0] == G.M16_3D + G.XCD          # "level-1 shape with the XCD-aware grid"
    assert _route(L, (8, 32, 64, 8, 64, 64, 3))[0] == G.M16_KQ + G.XCD          # "32 input channels on the K-quarter kernel"
    assert _route(L, (8, 320, 64, 1, 64, 64, 1))[0] & 15 == G.M16_2D            # "a decoder block with five ci tiles"
    assert {G.M16_3D, G.M16_3D + G.XCD, G.M16_KQ + G.XCD} <= seen
    # the split-K reduction's slices: 16 x 16 x 32 launches; >= 32 partial tensors (the 16-slice class) and fewer (the 4-slice class)
    groups = []
    for s in _shapes(O.test_splitk_reduction_slices_agree):
        r, g = _route(L, s)
        assert r & 15 == (G.M16_3D if s[6] == 3 else G.M16_2D), s
        if s[2] % 64 == 0:
            assert _route(L, s, dual=True) == (r + G.DUAL, g), s
        groups.append(g)
    assert min(groups) < 32 <= max(groups)


def test_route_settings_are_restored(L):
    """(after the tests above) the defaults hold: the level-1 first-layer shape is back on K quarters."""
    assert _route(L, (8, 32, 64, 8, 64, 64, 3))[0] == G.M16_KQ + G.XCD


@pytest.mark.parametrize("r", G.REFUSED, ids=[r[0] for r in G.REFUSED])
def test_refused_calls_route_to_their_error(r, L):
    assert G.refused_route(L, r) == (r[1], 0), r[0]


def test_empty_tensors_are_refused(L):
    """No input channels or no voxels: an argument error (the plan divides by the tile-pair count and clamps by the tile count)."""
    for B, Ci, Co, D, H, W, kd in ((2, 0, 64, 4, 8, 8, 3), (2, 64, 0, 4, 8, 8, 3), (0, 64, 64, 4, 8, 8, 3), (2, 64, 64, 0, 8, 8, 3),
                                   (2, 64, 64, 4, 0, 8, 3), (2, 64, 64, 4, 8, 0, 3), (2, 64, 64, 1, 8, 0, 1)):
        for abf in (1, 0):
            assert L.hupr_debug_wgrad_route(B, D, H, W, Ci, max(Ci, 8), Co, max(Co, 8), kd, abf, 0, 1 << 30, None) == G.HUPR_ERR_ARG


def test_a_tensor_of_2_to_the_31_elements_is_refused(L):
    """32-bit element offsets: 2^31 - 2^20 elements pass (register-staged kernel: >= 2 GiB), exactly 2^31 do not."""
    g = ctypes.c_int(-1)
    args = lambda B: (B, 2, 32, 32, 512, 512, 64, 64, 3, 1, 0, 1 << 40, ctypes.byref(g))
    assert (1 << 11) * 2 * 32 * 32 * 512 == 1 << 31
    assert L.hupr_debug_wgrad_route(*args(1 << 11)) == G.HUPR_ERR_ARG and g.value == 0
    assert L.hupr_debug_wgrad_route(*args((1 << 11) - 1)) == G.REG_BF16_3D and g.value > 0
    # the same through the leading dimension alone
    assert L.hupr_debug_wgrad_route(1, 2, 8, 8, 64, 1 << 24, 64, 64, 3, 1, 0, 1 << 40, None) == G.HUPR_ERR_ARG
    assert L.hupr_debug_wgrad_route(1, 2, 8, 8, 64, 1 << 23, 64, 64, 3, 1, 0, 1 << 40, None) == G.REG_BF16_3D


CHANNELS = (8, 24, 32, 64, 72, 96, 128, 256, 320, 512)
GEOMETRIES = {3: [(1, 2, 8, 8), (2, 4, 16, 16), (32, 8, 64, 64)], 1: [(1, 1, 8, 16), (3, 1, 32, 32), (32, 1, 128, 128)]}


@pytest.mark.parametrize("kd", [1, 3])
def test_ws_bytes_is_enough(kd, L):
    """hupr_conv3x3_wgrad_halo_ws_bytes(Ci, Co, kd) never makes the single call return HUPR_ERR_WORKSPACE, twice that never the dual
    call, for bf16 and fp32 storage, from one tile to the bench batch."""
    for Ci in CHANNELS:
        for Co in CHANNELS:
            full = L.hupr_conv3x3_wgrad_halo_ws_bytes(Ci, Co, kd)
            assert full >= Co * Ci * kd * 9 * 4
            for (B, D, H, W) in GEOMETRIES[kd]:
                g = ctypes.c_int(-1)
                for abf in (1, 0):
                    r = L.hupr_debug_wgrad_route(B, D, H, W, Ci, Ci, Co, Co, kd, abf, 0, full, ctypes.byref(g))
                    assert r > 0 and g.value >= 1 and g.value * Co * Ci * kd * 9 * 4 <= full, (Ci, Co, B, abf, r)
                if L.hupr_conv3x3_wgrad_halo_dual_supported(B, D, H, W, Ci, Co, kd):
                    r = L.hupr_debug_wgrad_route(B, D, H, W, Ci, Ci, Co, Co, kd, 1, 1, 2 * full, ctypes.byref(g))
                    assert r > G.DUAL and g.value >= 1 and g.value * 2 * Co * Ci * kd * 9 * 4 <= 2 * full, (Ci, Co, B, r)
                else:
                    assert Co % 64 != 0


# ---- gate sensitivity, on fp64 references only -------------------------------------------------------------------------------
SENSITIVITY_SHAPES = [(2, 64, 64, 2, 8, 8, 3), (2, 64, 64, 1, 8, 16, 1), (3, 96, 72, 4, 16, 16, 3)]


def _rejects(bad, ref, A, what):
    """bad: a faulty fp64 sum; rounded once to fp32 it must fail the gate at >= 80 % of the outputs the fault touches and nowhere else."""
    ok = G.within(bad.float(), ref, A)
    touched = bad != ref
    n = int(touched.sum())
    assert n > 0, what
    assert int((~ok & touched).sum()) >= 0.8 * n, (what, int((~ok & touched).sum()), n)
    assert not bool((~ok & ~touched).any()), what


@pytest.mark.parametrize("shape", SENSITIVITY_SHAPES, ids=["x".join(map(str, s)) for s in SENSITIVITY_SHAPES])
def test_fp64_gate_rejects_faulty_sums(shape):
    """A faithful result (the fp64 sum rounded once to fp32) passes the gate; the same sum with one voxel of x missing, one 32-voxel
    K-step of one tile missing, two dy channels exchanged, or a halo row read across the batch border fails it."""
    B, Ci, Co, D, H, W, kd = shape
    x = G.rnd(B, D, H, W, Ci, seed=11).bfloat16()
    dy = G.rnd(B, D, H, W, Co, seed=12).bfloat16()
    ref, A = G.wgrad_ref(x, dy, kd)
    assert bool(G.within(ref.float(), ref, A).all())
    # (a) one voxel of x zeroed: the first corner, the last voxel, an interior one
    for vox in ((0, 0, 0, 0), (B - 1, D - 1, H - 1, W - 1), (B // 2, D // 2, H // 2, W // 2)):
        xz = x.clone()
        xz[vox] = 0
        _rejects(G.wgrad_ref(xz, dy, kd)[0], ref, A, ("voxel", vox))
    # (b) the second 32-voxel K-step of the first tile (2 x 8 x 8 voxels: depth 0, rows 4 .. 7; 1 x 8 x 16: rows 2, 3) is missing from
    # the first 64 x 64 (co, ci) tile
    part = torch.zeros_like(dy)
    if kd == 3:
        part[0, 0, 4:8, 0:8, :64] = dy[0, 0, 4:8, 0:8, :64]
    else:
        part[0, 0, 2:4, 0:16, :64] = dy[0, 0, 2:4, 0:16, :64]
    lost = G.wgrad_ref(x, part, kd)[0]
    bad = ref.clone()
    bad[:64, :64] -= lost[:64, :64]
    _rejects(bad, ref, A, "K-step")
    # (c) two dy channels exchanged
    sw = dy.clone()
    sw[..., 1], sw[..., Co - 2] = dy[..., Co - 2], dy[..., 1]
    _rejects(G.wgrad_ref(x, sw, kd)[0], ref, A, "channels")
    # (d) batch item 1's top halo row holds item 0's bottom row instead of zeros
    xp = G.zero_padded(x, kd)
    xp[1, :, 0] = xp[0, :, H]
    _rejects(G.wgrad_ref(x, dy, kd, xp)[0], ref, A, "halo row")
