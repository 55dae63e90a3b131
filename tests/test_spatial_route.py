"""CPU (no GPU needed): the launch plan of the spatial kernels (hupr_debug_interp_route, hupr_debug_mnet_grid: the host functions the
launchers of csrc/spatial.hip themselves call) sends every case of the fp64 table (test_spatial_fp64_gpu.py), the resampling and MNet
shapes of test_ops_gpu.py and the model's own maps at batch 1, 3 and 32 to the kernel and grid they name — the rule is restated here
(VPT = 4 iff C % (4 V) == 0 and voxels C / (4 V) >= 65536; 8192 / 16384 / 8192 / 1024 workgroups at most), so a change that silently
moves the training shapes off VPT = 4 or changes a cap fails; the table reaches both VPT values in both storage types, plain and
accumulating, the threshold from below, at and above, a wrapping and a non-wrapping grid of every looping kernel, every entry point
of spatial.hip, every kind of degenerate axis and non-integer ratios both ways; the refused calls are refused by host checks alone;
every MNet case is free of near-ties after its re-draws and the tie case holds its share of exact ties; and the gates reject the
results of subtly wrong kernels (mutated copies of the fp64 reference) while they accept an honest fp32 evaluation."""
import pytest
import torch

import test_ops_gpu as O
import test_spatial_fp64_gpu as S


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


# ---- routes ------------------------------------------------------------------------------------------------------------------------
def rule(op, T, B, din, dout, C):
    """The plan, restated: (channel vectors per thread, workgroups)."""
    if op == "fwd":
        return 1, min(8192, -(-B * S.vox(dout) * (C // 4) // 256))
    V = 8 if T == "bf16" else 4
    voxels = B * S.vox(din)
    vpt = 4 if C % (4 * V) == 0 and voxels * C // (4 * V) >= 65536 else 1
    return vpt, min(16384, -(-voxels * (C // (V * vpt)) // 256))


def mnet_rule(n_bg, pixels):
    total = n_bg * pixels
    return min(8192, -(-total // 256)), min(8192, -(-total // 256)), min(1024, -(-total // 64))


@pytest.mark.parametrize("c", S.CASES, ids=[c.name for c in S.CASES])
def test_fp64_case_table_routes(c, L):
    for T in c.types:
        for op in c.ops:
            lit = S.expected_route(c, T, op)
            assert lit is not None, (c.name, T, op)
            assert S.case_route(L, c, T, op) == lit == rule(op, T, c.B, c.din, c.dout, c.C), (c.name, T, op)
    # a literal stands only where the case runs that launch
    assert (c.fwd is None) == ("fwd" not in c.ops) and (c.bwd32 is None) == ("f32" not in c.types or c.ops == ("fwd",))
    assert (c.bwd16 is None) == ("bf16" not in c.types or c.ops == ("fwd",))
    assert c.in_ld >= c.C and c.off + c.C <= c.out_ld and c.off % 8 == 0


def test_sweep_identity_and_node_cases_take_one_workgroup(L):
    for T in S.BOTH:
        for op in S.OPS:
            for n_in in range(1, 13):
                for n_out in range(1, 13):
                    for din, dout in (((1, 1, n_in), (1, 1, n_out)), ((1, n_in, 3), (1, n_out, 3))):
                        assert S.route_of(L, op, T, 2, din, dout, 8, 8, 8) == (1, 1) == rule(op, T, 2, din, dout, 8)
            assert S.route_of(L, op, T, 2, (2, 3, 5), (2, 3, 5), 8, 8, 8) == (1, 1)
            assert S.route_of(L, op, T, 2, (3, 4, 5), (5, 7, 9), 8, 8, 8) == rule(op, T, 2, (3, 4, 5), (5, 7, 9), 8) == ((1, 5) if op == "fwd" else (1, 1))
            assert S.case_route(L, S.NODE, T, op) == S.expected_route(S.NODE, T, op)


@pytest.mark.parametrize("c", S.MCASES + [S.TIE_CASE], ids=[c.name for c in S.MCASES + [S.TIE_CASE]])
def test_mnet_case_table_grids(c, L):
    g = S.mnet_grids(L, c)
    assert g == mnet_rule(c.n_bg, c.pixels)
    assert g[1] == c.g_means
    assert c.x_fed == (c.g_fwd is not None) and c.bwd == (c.g_bwd is not None)
    if c.x_fed:
        assert g[0] == c.g_fwd
    if c.bwd:
        assert g[2] == c.g_bwd


def _params(test):
    (mark,) = [m for m in test.pytestmark if m.name == "parametrize"]
    return mark.args[0], mark.args[1]


# the model's resampling launches: (name, din, dout, C, storage types, VPT of the backward at batch 1, 3, 32)
MODEL = [("level 1 -> half", (8, 64, 64), (4, 32, 32), 64, {"bf16": (4, 4, 4), "f32": (4, 4, 4)}),
         ("level 2 -> half", (4, 32, 32), (2, 16, 16), 128, {"bf16": (1, 1, 4), "f32": (1, 4, 4)}),
         ("decoder 16 -> 32, C = 256", (1, 16, 16), (1, 32, 32), 256, {"bf16": (1, 1, 4), "f32": (1, 1, 4)}),
         ("decoder 32 -> 64, C = 128", (1, 32, 32), (1, 64, 64), 128, {"bf16": (1, 1, 4), "f32": (1, 1, 4)}),
         ("decoder 32 -> 64, C = 64", (1, 32, 32), (1, 64, 64), 64, {"bf16": (1, 1, 4), "f32": (1, 1, 4)}),
         ("PRGCN 64 -> 32", (1, 64, 64), (1, 32, 32), 16, {"f32": (1, 1, 4)}),
         ("PRGCN 32 -> 64", (1, 32, 32), (1, 64, 64), 16, {"f32": (1, 1, 1)})]


def test_existing_tests_and_model_shapes_keep_their_routes(L):
    names, params = _params(O.test_interp_align_corners)
    assert names == "shape,size" and len(params) >= 5
    for (B, D, H, W, C), size in list(params) + [((2, 8, 16, 16, 64), (4, 8, 8))]:
        for T in S.BOTH:
            if T == "bf16" and C % 8:
                continue
            for op in S.OPS:
                got = S.route_of(L, op, T, B, (D, H, W), tuple(size), C, C, C)
                assert got == rule(op, T, B, (D, H, W), tuple(size), C) and got[0] == 1, (B, D, H, W, C, T, op)      # all far below the threshold
                assert got[1] < (8192 if op == "fwd" else 16384)                                            # and none wraps
    for n_bg, pixels in ((6, 256), (16, 256)):              # test_mnet_front_end, test_interp_mnet_cast_bf16_activations
        assert tuple(L.hupr_debug_mnet_grid(op, n_bg, pixels) for op in (0, 1, 2)) == mnet_rule(n_bg, pixels) == (
            (6, 6, 24) if n_bg == 6 else (16, 16, 64))
    for name, din, dout, C, vpts in MODEL:
        for T, want in vpts.items():
            for B, vpt in zip((1, 3, 32), want):
                for op in ("bwd", "acc"):
                    got = S.route_of(L, op, T, B, din, dout, C, C, C)
                    assert got == rule(op, T, B, din, dout, C) and got[0] == vpt, (name, T, B, op, got)
                fw = S.route_of(L, "fwd", T, B, din, dout, C, C, C)
                assert fw == rule("fwd", T, B, din, dout, C) and fw[0] == 1
    # the decoder writes into, and reads its gradient from, channel slices of the 320-wide concatenation buffer: same plan
    assert S.route_of(L, "fwd", "bf16", 32, (1, 16, 16), (1, 32, 32), 256, 256, 320) == (1, 8192)
    assert S.route_of(L, "bwd", "bf16", 32, (1, 16, 16), (1, 32, 32), 256, 256, 320) == (4, 256)
    # MNet at the model's 64 x 64 pixels, n_bg = 8 B
    for B, want in ((1, (128, 128, 512)), (3, (384, 384, 1024)), (32, (4096, 4096, 1024))):
        assert tuple(L.hupr_debug_mnet_grid(op, 8 * B, 4096) for op in (0, 1, 2)) == want == mnet_rule(8 * B, 4096)
    # the caps themselves
    assert S.route_of(L, "fwd", "f32", 1, (1, 1, 1), (1, 8192, 256), 4, 4, 4) == (1, 8192)
    assert S.route_of(L, "fwd", "f32", 1, (1, 1, 1), (1, 8193, 256), 4, 4, 4) == (1, 8192)
    assert S.route_of(L, "fwd", "f32", 1, (1, 1, 1), (1, 8191, 256), 4, 4, 4) == (1, 8191)
    assert S.route_of(L, "bwd", "f32", 1, (1, 16385, 256), (1, 1, 1), 4, 4, 4) == (1, 16384)
    assert S.route_of(L, "bwd", "f32", 1, (1, 16383, 256), (1, 1, 1), 4, 4, 4) == (1, 16383)
    assert [L.hupr_debug_mnet_grid(0, 8193, 256), L.hupr_debug_mnet_grid(1, 8191, 256), L.hupr_debug_mnet_grid(2, 1025, 64),
            L.hupr_debug_mnet_grid(2, 1023, 64)] == [8192, 8191, 1024, 1023]
    assert L.hupr_debug_mnet_grid(3, 1, 1) == L.hupr_debug_mnet_grid(0, 0, 1) == L.hupr_debug_mnet_grid(2, 1, 0) == S.HUPR_ERR_ARG
    assert L.hupr_debug_interp_route(3, 0, 1, 1, 1, 1, 1, 1, 1, 4, 4, 4, None) == S.HUPR_ERR_ARG
    assert L.hupr_debug_interp_route(0, 0, 1, 1, 1, 1, 1, 1, 1, 4, 4, 4, None) == 1              # (a null grid_out is allowed)
    assert L.hupr_mnet_bwd_ws_bytes() == 1024 * 160 * 4                                           # the backward cap x partial[160]


# ---- coverage of the table ---------------------------------------------------------------------------------------------------------
def test_the_table_reaches_every_route_threshold_and_loop_kind():
    runs = [(c, T, op) for c in S.CASES for T in c.types for op in c.ops]
    routes = {(S.expected_route(c, T, op)[0], T, op) for c, T, op in runs if op != "fwd"}
    assert routes == {(vpt, T, op) for vpt in (1, 4) for T in S.BOTH for op in ("bwd", "acc")}
    for T, V in (("f32", 4), ("bf16", 8)):
        at = {c.B * S.vox(c.din) * c.C // (4 * V) for c in S.CASES if T in c.types and "bwd" in c.ops and c.C % (4 * V) == 0}
        assert 65535 in at and 65536 in at and any(n > 65536 for n in at), (T, sorted(at))
        # C a multiple of V but not of 4 V on a large map (a full grid at VPT = 1)
        assert any(c.C % V == 0 and c.C % (4 * V) and c.B * S.vox(c.din) * c.C // V >= 65536
                   for c in S.CASES if T in c.types and "bwd" in c.ops), T
    # a wrapping and a non-wrapping grid of every looping kernel: items against cap x 256
    fwd_items = [c.B * S.vox(c.dout) * (c.C // 4) for c in S.CASES if "fwd" in c.ops]
    assert max(fwd_items) > 8192 * 256 and min(fwd_items) < 8192 * 256
    for vpt in (1, 4):
        items = [rule("bwd", T, c.B, c.din, c.dout, c.C) + (c.B * S.vox(c.din) * c.C // ((8 if T == "bf16" else 4) * vpt),)
                 for c in S.CASES for T in c.types if "bwd" in c.ops]
        mine = [n for v, _, n in items if v == vpt]
        assert max(mine) > 16384 * 256 and min(mine) < 16384 * 256, vpt
    for c in S.CASES:
        if c.name.startswith("bwd-wrap"):
            assert set(c.ops) == {"bwd", "acc"}                           # the accumulating form wraps too
    totals = [c.n_bg * c.pixels for c in S.MCASES]
    assert max(totals) > 8192 * 256 and min(totals) < 256                 # hupr_k_mnet_fwd_means; the x-fed loop: see the GPU module
    bw = [c.n_bg * c.pixels for c in S.MCASES if c.bwd]
    assert min(bw) < 64 and 1024 * 64 in bw and any(n > 65536 and n % 65536 == 0 for n in bw) and any(n > 65536 and n % 64 for n in bw)
    assert any(c.n_bg > 1 and (c.n_bg * c.pixels) % 256 for c in S.MCASES)


def entries_named():
    """The entry points the table's cases call (as run by the GPU module's launch, mnet_forward and mnet_backward)."""
    names = {S.ENTRY[(op, T)] for c in S.CASES for T in c.types for op in c.ops}
    for c in S.MCASES:
        for T in ("f32", "bf16act"):
            names.add("hupr_mnet_fwd_means_" + T)
            if c.x_fed:
                names.add("hupr_mnet_fwd_" + T)
            if c.bwd:
                names |= {"hupr_mnet_bwd_" + T, "hupr_mnet_bwd_ws_bytes"}
    return names


def test_every_entry_point_of_spatial_hip_is_named_by_a_case():
    entries = S.spatial_entries()
    assert len(entries) == 13, entries          # six resampling, six MNet launches and the workspace size (hupr_mnet_stream_* lives elsewhere)
    assert entries_named() == set(entries)


def test_the_table_holds_every_degenerate_axis_and_ratio_kind():
    pairs = {(i, o) for c in S.CASES for i, o in zip(c.din, c.dout)}
    assert (1, 1) in pairs and any(i > 1 and o == 1 for i, o in pairs) and any(i == 1 and o > 1 for i, o in pairs)
    assert any(i == o > 1 for i, o in pairs)
    frac = lambda i, o: i > 1 and o > 1 and (i - 1) % (o - 1) != 0 and (o - 1) % (i - 1) != 0
    assert any(frac(i, o) and o > i for i, o in pairs) and any(frac(i, o) and o < i for i, o in pairs)
    assert {(7, 13), (13, 7), (31, 17), (5, 64), (64, 5)} <= pairs
    Ts = {c.name: S.contributors(c.din, c.dout) for c in S.CASES if not c.dev}
    assert Ts["5to64-many-contributors"][0] >= 400                        # many contributors per input voxel
    assert Ts["64to5-most-without"][1].float().mean() < 0.05             # most input voxels have none
    assert any(c.in_ld > c.C for c in S.CASES) and any(c.out_ld == c.C + 8 for c in S.CASES)
    assert any(c.out_ld == 320 and c.off for c in S.CASES)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", S.REFUSED, ids=[r[0] for r in S.REFUSED])
def test_refused_calls_are_refused_by_host_checks(r, L):
    """On made-up addresses and without a device: the error comes back before anything is launched or dereferenced."""
    n0 = L.hupr_launch_count()
    assert S.refused_call(L, r, 1 << 24, 2 << 24, None) == S.HUPR_ERR_ARG, (r[0], L.hupr_last_error())
    assert L.hupr_launch_count() == n0
    if r[4] is None:
        assert S.route_of(L, r[2], r[1], *r[3]) == S.HUPR_ERR_ARG


def test_refusal_table_covers_the_issue_list(L):
    whats = " | ".join(r[0] for r in S.REFUSED)
    for T in S.BOTH:
        for op in S.OPS:
            for frag in ("C = 6", "in_ld < C", "out_ld % 4 != 0", "extent of 0", "null source", "null destination"):
                assert "%s %s: %s" % (T, op, frag) in whats or frag == "extent of 0" and "%s %s: an input extent of 0" % (T, op) in whats
    assert "bf16 bwd: C = 12" in whats and "bf16 acc: C = 12" in whats
    assert S.route_of(L, "fwd", "bf16", 2, (2, 4, 4), (3, 5, 6), 12, 12, 12) == (1, 3)       # C = 12 goes forward
    assert L.hupr_mnet_bwd_f32(None, None, 1 << 24, 1 << 24, 1 << 24, 1 << 24, 1 << 24, 1, 37, 1 << 24, 1 << 20, None) == S.HUPR_ERR_ARG
    assert L.hupr_mnet_bwd_bf16act(None, 1 << 24, 1 << 24, 1 << 24, 1 << 24, 1 << 24, 1 << 24, 1, 37, 1 << 24,
                                   L.hupr_mnet_bwd_ws_bytes() - 1, None) == S.HUPR_ERR_WORKSPACE


# ---- the near-tie condition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.MCASES, ids=[c.name for c in S.MCASES])
def test_mnet_case_has_no_near_tie_after_redrawing(c):
    o = S.draw_mnet(c)
    w, b = o["w"].double(), o["b"].double()
    assert o["left"] == 0                                    # the last pass of the re-drawing loop found none
    if o["m"].shape[0] <= 1 << 18:                           # and, where it is cheap, once more from scratch
        assert not bool(S.near_ties(o["m"].double(), w, b).any())
    if c.x_fed:                                              # the drawn x has exactly these means, in fp32 and in any order
        x = o["x"].view(c.n_bg, 16, c.pixels, 8)
        assert bool((x.abs() < 4).all()) and torch.equal(x * 1024, (x * 1024).round())
        m = x.double().mean(-1).permute(0, 2, 1).reshape(-1, 16)
        assert torch.equal(m, o["m"].double()) and torch.equal(x.flip(-1).sum(-1) * 0.125, x.sum(-1) * 0.125)
    if c.name == "model-64x64-bg32":
        assert o["redrawn"] > 0                                # (the loop is exercised: a table this size does draw near-ties)


def test_tie_case_holds_its_share_of_exact_ties_and_matches_max_pool3d():
    o = S.draw_ties()
    m, w, b = o["m"].double(), o["w"].double(), o["b"].double()
    assert S.exact_ties(m, w, b).float().mean().item() >= S.TIE_SHARE
    ref, _, t = S.mnet_fwd_ref(m, w, b)
    dw, _, db, _ = S.mnet_bwd_ref(m, t, o["dy"].double())
    y64, dw64, db64 = S.tie_torch64(o)
    assert torch.equal(ref, y64) and torch.equal(dw, dw64) and torch.equal(db, db64)
    # the last of several ties winning: the same forward, another weight gradient — the exact comparison of the GPU test sees it
    last = lambda o_: 3 - S.first_max(o_.flip(-1))
    ref2, _, t2 = S.mnet_fwd_ref(m, w, b, pick=last)
    assert torch.equal(ref2, ref) and bool((t2 != t).any())
    assert not torch.equal(S.mnet_bwd_ref(m, t2, o["dy"].double())[0], dw)


# ---- gate sensitivity: resampling, on CPU fp64 data -----------------------------------------------------------------------------------
def stored(t, bf16):
    """What a kernel would leave in memory of the sums t: one rounding to fp32, one more to bf16 behind a bf16 store."""
    return t.float().to(torch.bfloat16) if bf16 else t.float()


def _rejects(ok, bad, ref, what, frac):
    """ok: the gate on the stored faulty result; it must fail at >= frac of the outputs the fault touches (at one at least) and nowhere else."""
    touched = (bad != ref) | bad.isnan()
    n, caught = int(touched.sum()), int((~ok & touched).sum())
    assert n > 0, what
    assert caught >= max(1, frac * n), (what, caught, n)
    assert not bool((~ok & ~touched).any()), what


GEO = ((3, 7, 10), (5, 4, 16))              # the table's trilinear case: another ratio on each axis
WIDE = ((1, 1, 300), (1, 1, 467))           # extents at which the fp32 rounding of src is far above the gate


@pytest.fixture(scope="module")
def data():
    d = {}
    for key, (din, dout) in (("geo", GEO), ("wide", WIDE), ("up", ((1, 1, 5), (1, 1, 64))), ("down", ((1, 1, 31), (1, 1, 17)))):
        g = torch.Generator().manual_seed(11)
        x = torch.randn(2, S.vox(din), 8, generator=g).to(torch.bfloat16).double()
        dy = torch.randn(2, S.vox(dout), 8, generator=g).to(torch.bfloat16).double()
        dx0 = torch.randn(2, S.vox(din), 8, generator=g).to(torch.bfloat16).double()
        taps = S.taps_of(din, dout)
        d[key] = {"din": din, "dout": dout, "x": x, "dy": dy, "dx0": dx0, "taps": taps, "fwd": S.fwd_ref(x, taps),
                  "bwd": S.bwd_ref(dy, taps, S.vox(din)), "acc": S.bwd_ref(dy, taps, S.vox(din), dx0),
                  "T": S.contributors(din, dout)[0]}
    return d


def mutated_axis_map(kind):
    f32 = torch.float32

    def axis_map(n_in, n_out, device="cpu"):
        (i0, i1), (w0, w1) = S.axis_map(n_in, n_out, device)
        if kind == "swap":
            return (i0, i1), (w1, w0)
        o = torch.arange(n_out, dtype=f32)
        if kind == "half-pixel":                             # align_corners=False coordinates
            src = ((o.double() + 0.5) * n_in / n_out - 0.5).clamp_min(0).float()
            i0 = src.to(torch.int64).clamp_max(n_in - 1)
            i1 = (i0 + 1).clamp_max(n_in - 1)
            w1 = src - i0.float()
            return (i0, i1), ((1 - w1).double(), w1.double())
        if kind == "unrounded-src":                          # src - i0 contracted into one fma: the product is never rounded
            scale = (torch.tensor(float(n_in - 1), dtype=f32) / torch.tensor(float(max(n_out - 1, 1)), dtype=f32)) if n_out > 1 else torch.zeros((), dtype=f32)
            w1 = (scale.double() * o.double() - i0.double()).float()
            return (i0, i1), ((1 - w1).double(), w1.double())
        raise KeyError(kind)
    return axis_map


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_resampling_gates_accept_faithful_results(data, bf16):
    """The fp64 sums rounded once (twice behind a bf16 store) and an fp32 accumulation in reversed tap order pass everywhere."""
    for key, d in data.items():
        for op in S.OPS:
            ref, A = d[op]
            gate = (lambda t: S.within_fwd(t, ref, A, bf16)) if op == "fwd" else (lambda t: S.within_bwd(t, ref, A, d["T"], bf16))
            assert bool(gate(stored(ref, bf16)).all()), (key, op)
            # fp32: the weight product rounded twice, then every tap accumulated in fp32, last tap first
            if op == "fwd":
                acc = torch.zeros_like(ref, dtype=torch.float32)
                for idx, w in reversed(d["taps"]):
                    acc = acc + w.float().view(1, -1, 1) * d["x"].float()[:, idx]
            else:
                acc = d["dx0"].float().clone() if op == "acc" else torch.zeros_like(ref, dtype=torch.float32)
                for idx, w in reversed(d["taps"]):
                    acc.index_add_(1, idx.flip(0), (w.float().view(1, -1, 1) * d["dy"].float()).flip(1))
            assert key == "down" or bool((acc.double() != ref).any())      # (another result than the reference's; 30 / 16 is exact)
            assert bool(gate(stored(acc, bf16)).all()), (key, op, "reversed fp32 accumulation")


def test_forward_gate_rejects_wrong_coordinates(data):
    d = data["geo"]
    ref, A = d["fwd"]
    for kind, frac in (("half-pixel", 0.8), ("swap", 0.8)):
        bad = S.fwd_ref(d["x"], S.taps_of(d["din"], d["dout"], axis_map=mutated_axis_map(kind)))[0]
        _rejects(S.within_fwd(stored(bad, False), ref, A, False), bad, ref, "fwd " + kind, frac)
        _rejects(S.within_fwd(stored(bad, True), ref, A, True), bad, ref, "fwd bf16 " + kind, 0.7)
        badb = S.bwd_ref(d["dy"], S.taps_of(d["din"], d["dout"], axis_map=mutated_axis_map(kind)), S.vox(d["din"]))[0]
        rb, Ab = d["bwd"]
        _rejects(S.within_bwd(stored(badb, False), rb, Ab, d["T"], False), badb, rb, "bwd " + kind, frac)


def test_forward_gate_rejects_an_unrounded_src(data):
    """src taken from the unrounded product (the fma contraction lin_coord's pragma forbids): the weights move by up to half an ulp of
    src; at extents of a few hundred that is far above 2^-20 A wherever neighbouring voxels differ."""
    d = data["wide"]
    ref, A = d["fwd"]
    bad = S.fwd_ref(d["x"], S.taps_of(d["din"], d["dout"], axis_map=mutated_axis_map("unrounded-src")))[0]
    _rejects(S.within_fwd(stored(bad, False), ref, A, False), bad, ref, "fwd unrounded src", 0.25)
    rb, Ab = d["bwd"]
    badb = S.bwd_ref(d["dy"], S.taps_of(d["din"], d["dout"], axis_map=mutated_axis_map("unrounded-src")), S.vox(d["din"]))[0]
    _rejects(S.within_bwd(stored(badb, False), rb, Ab, d["T"], False), badb, rb, "bwd unrounded src", 0.25)


def test_forward_gate_rejects_an_unclamped_upper_tap(data):
    """i1 = i0 + 1 without the clamp: at the upper edge the tap reads the next row, the next sample or — from the last voxel — the
    NaN guard tail behind x; its weight is 0 there, so only the NaN shows: the result must hold one and the gate must fail on it."""
    d = data["geo"]
    (Di, Hi, Wi), (Do, Ho, Wo) = d["din"], d["dout"]
    ref, A = d["fwd"]
    B, Vi, C = d["x"].shape
    flat = torch.cat([d["x"].reshape(B * Vi, C), torch.full((Hi * Wi + Wi + 2, C), float("nan"), dtype=torch.float64)])
    md, mh, mw = (S.axis_map(i, o) for i, o in zip(d["din"], d["dout"]))
    bad = torch.zeros_like(ref)
    for a in range(2):
        for b_ in range(2):
            for c_ in range(2):
                idx = ((md[0][0] + a).view(Do, 1, 1) * Hi + (mh[0][0] + b_).view(1, Ho, 1)) * Wi + (mw[0][0] + c_).view(1, 1, Wo)
                w = md[1][a].view(Do, 1, 1) * mh[1][b_].view(1, Ho, 1) * mw[1][c_].view(1, 1, Wo)
                for s in range(B):
                    bad[s] += w.reshape(-1, 1) * flat[idx.reshape(-1) + s * Vi]
    assert bool(bad.isnan().any())
    ok = S.within_fwd(stored(bad, False), ref, A, False)
    assert not bool(ok[bad.isnan()].any()) and bool(ok[~bad.isnan()].all())


def test_backward_gate_rejects_a_window_that_drops_an_edge_contributor(data):
    """lin_range one candidate too narrow at its lower or its upper end, strongly up-sampling (many contributors) and down-sampling."""
    for key in ("up", "down"):
        d = data[key]
        n_in, n_out = d["din"][2], d["dout"][2]
        (i0, i1), (w0, w1) = S.axis_map(n_in, n_out)
        M = torch.zeros(n_out, n_in, dtype=torch.float64)
        r = torch.arange(n_out)
        M.index_put_((r, i0), w0, accumulate=True)
        M.index_put_((r, i1), w1, accumulate=True)
        ref, A = d["bwd"]
        assert torch.allclose(torch.einsum("oi,bok->bik", M, d["dy"]), ref, rtol=0, atol=1e-12)
        for end in ("lowest", "highest"):
            Mm = M.clone()
            for i in range(n_in):
                nz = (M[:, i] != 0).nonzero().view(-1)
                if nz.numel() >= 1:                              # (down-sampling: often the only one)
                    Mm[nz[0] if end == "lowest" else nz[-1], i] = 0
            bad = torch.einsum("oi,bok->bik", Mm, d["dy"])
            for bf16, frac in ((False, 0.9), (True, 0.5)):
                _rejects(S.within_bwd(stored(bad, bf16), ref, A, d["T"], bf16), bad, ref, "%s: %s contributor dropped" % (key, end), frac)


def test_backward_gate_rejects_a_lost_dx0_and_a_shifted_channel_vector(data):
    d = data["geo"]
    ref, A = d["acc"]
    bad = d["bwd"][0]                                          # the accumulating form ignoring dx0
    for bf16 in (False, True):
        _rejects(S.within_bwd(stored(bad, bf16), ref, A, d["T"], bf16), bad, ref, "acc without dx0", 0.95)
    for op in S.OPS:
        ref, A = d[op]
        bad = ref.clone()
        bad[..., 4:8] = ref.roll(1, dims=1)[..., 4:8]           # one 4-channel vector taken from the neighbouring voxel
        gate = S.within_fwd(stored(bad, False), ref, A, False) if op == "fwd" else S.within_bwd(stored(bad, False), ref, A, d["T"], False)
        _rejects(gate, bad, ref, op + ": channel vector shifted", 0.95)


# ---- gate sensitivity: MNet ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mdata():
    c = S.MCASES[1]
    o = S.draw_mnet(c)
    o["c"] = c
    o["md"], o["wd"], o["bd"] = o["m"].double(), o["w"].double(), o["b"].double()
    o["ref"] = S.mnet_fwd_ref(o["md"], o["wd"], o["bd"])
    o["gref"] = S.mnet_bwd_ref(o["md"], o["ref"][2], o["dy"].double())
    return o


def test_mnet_gates_accept_faithful_results(mdata):
    ref, A, t = mdata["ref"]
    assert bool(S.mnet_within(ref.float(), ref, A).all())
    # the kernel's own order in fp32 without fused multiply-adds (eight roundings instead of four: inside 2^-21 A, and inside the gate
    # at all but a few entries) — and dW / dbias summed in fp32 in reversed pixel order, inside c A_d
    dw, dwA, db, dbA = mdata["gref"]
    v = mdata["m"].view(-1, 2, 4, 2).permute(0, 2, 1, 3)
    tk = v.gather(1, t.view(-1, 32, 1, 1).expand(-1, 32, 2, 2))
    dw32 = (mdata["dy"].view(-1, 32, 1, 1) * tk).flip(0).sum(0)
    db32 = mdata["dy"].flip(0).sum(0)
    assert dw32.dtype == torch.float32
    assert bool(S.grad_within(dw32, dw, dwA, S.MNET_C["dw"]).all()) and bool(S.grad_within(db32, db, dbA, S.MNET_C["db"]).all())


def test_mnet_gates_reject_wrong_front_ends(mdata):
    ref, A, t = mdata["ref"]
    md, wd, bd = mdata["md"], mdata["wd"], mdata["bd"]
    dy = mdata["dy"].double()
    dw, dwA, db, dbA = mdata["gref"]

    def check(what, bad_m=None, bad_w=None, steps=None, frac=0.9):
        if steps is None:
            out, _, tb = S.mnet_fwd_ref(md if bad_m is None else bad_m, wd if bad_w is None else bad_w, bd)
            gw = S.mnet_bwd_ref(md if bad_m is None else bad_m, tb, dy)[0]
        else:
            out, gw = steps
        _rejects(S.mnet_within(out.float(), ref, A), out, ref, "mnet fwd: " + what, frac)
        _rejects(S.grad_within(gw.float(), dw, dwA, S.MNET_C["dw"]), gw, dw, "mnet dW: " + what, frac)

    check("read as a permute (t = j / 2)", bad_m=md.view(-1, 8, 2).permute(0, 2, 1).reshape(-1, 16))
    check("kt taps exchanged", bad_w=wd.flip(-1))
    x = mdata["x"].double()                                      # [n_bg, 16, pixels, 8]
    m7 = x[..., :7].mean(-1).permute(0, 2, 1).reshape(-1, 16)
    check("mean over seven elevations", bad_m=m7)
    # conv stride 1: step t2 reads t = t2, t2 + 1 instead of 2 t2, 2 t2 + 1 (the pool then covers the first four of seven positions)
    v = md.view(-1, 2, 8)
    pairs = torch.stack([v[:, :, 0:4], v[:, :, 1:5]], dim=-1)           # [N, ch2, t2, kt]
    o = torch.einsum("nctk,ock->not", pairs, wd) + bd.view(1, 32, 1)
    tb = S.first_max(o)
    out = o.gather(2, tb.unsqueeze(-1)).squeeze(-1)
    tk = pairs.permute(0, 2, 1, 3).gather(1, tb.view(-1, 32, 1, 1).expand(-1, 32, 2, 2))
    check("conv stride 1", steps=(out, (dy.view(-1, 32, 1, 1) * tk).sum(0)))
