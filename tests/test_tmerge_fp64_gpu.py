"""GPU (-m gpu): every form of the temporal merges (Conv3d with a (G, 1, 1) kernel; csrc/tmerge_stream.hip and the generic engine they
fall back to) against an fp64 reference of exactly the operands the kernel reads, element by element, with the route of every launch
asserted first from the library's own answers (hupr_tmerge_stream_supported, hupr_tmerge_wgrad_stream_supported and, for a streaming
weight gradient, the workgroup count implied by hupr_tmerge_wgrad_stream_ws_bytes): the three instantiations of the persistent forward
kernel and of the input gradient with even and uneven persistent loops, the weight gradient on real and on virtual frames with both
reduce kernels, the generic kernels at the shapes that really fall through, refused calls, a map just under the 32-bit buffer bound,
and the two autograd nodes of functional.py with the entry points counted.

Reference: fp64 einsum over x (bf16-representable), W rounded to bf16 (nearest even) and, for the two gradients, dy rounded to bf16
(nearest even: the streaming and the generic kernels all convert it).  A is the same sum over absolute values.

Gate (``within``): the bf16 x bf16 products are exact in fp32, only the fp32 summation order is free, so no term is relative to the
result:  fp32 outputs (merged map, dW, the fp32 dx of the generic kernel)  |out - ref| <= c A;  bf16-stored dx  |out - ref| <=
2^-8 |ref| + c A.  c per operation (GATE_C) is the smallest power of two that is at least 8 x the worst err / A measured over this
table against fp64 on an MI355X, never above 2^-16 (the gate of an fp32-output convolution); the 8 x is room for legitimate changes of
tile and slot order.  For the bf16-stored dx the measured figure is the part of the error the store cannot explain (``measured``): where
the stored value is not the bf16 nearest to ref, the distance from ref to the rounding border the fp32 sum must have crossed.
Measured worst values per route:

    operation                      streaming kernel   generic engine
    fwd                            2^-22.74           2^-23.09
    dgrad, bf16 dx (lower bound)   2^-24.22           2^-25.78
    dgrad, fp32 dx                                    2^-23.62
    wgrad                          2^-23.50           2^-24.11

(fwd: the 520-tile case at G = 2; wgrad: the one-tile cases, whose short sums carry the fp32 rounding of the result itself, 2^-24 of
it; the 2 GiB weight gradient: 2^-28.46.)  8 x these: 2^-19.74, 2^-20.62, 2^-20.50, hence GATE_C = 2^-19 (fwd), 2^-20 (dgrad),
2^-20 (wgrad).

Outputs (merged map, dx, dW) are views at 16-byte-aligned offsets inside NaN-pattern buffers, preceded and followed by guards; the
workspace has exactly the byte count the library asks for, followed by a guard; every guard must come back bit-identical, no output
element may stay NaN, and a second launch into fresh buffers must give the same bits.  x and dy end in NaN guard tails, so a read
past their end shows.  The exact-index cases use one-hot operands: any slip in swizzle, frame order or tap reversal is an exact
mismatch there, not a tolerance question.

Near the 32-bit bound: x of 2^31 - 2^17 bytes (B = 1, G = 8, HW = 2^21 - 128; 16 383 tiles, 64 rounds of the 256 persistent
workgroups).  The forward compares the first and the last tile of every run of 2 048 tiles and the very last tile against a device-side
fp64 reference; the weight gradient of the same shape is compared entirely against a chunked device-side fp64 reference.

tests/test_tmerge_route.py checks the routes of this table, its coverage and the refusals without a GPU, and that the gate rejects
the results of subtly wrong kernels."""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

from test_conv_halo_fp64_gpu import GUARD, NAN16, NAN32, bits, nan_buffer, padded, rnd

pytestmark = pytest.mark.gpu

HUPR_ERR_ARG, HUPR_ERR_WORKSPACE = -1, -2
CAP = 2.0 ** -16                                       # the project's gate of an fp32-output convolution
GATE_C = {"fwd": 2.0 ** -19, "dgrad": 2.0 ** -20, "wgrad": 2.0 ** -20}
OPS = ("fwd", "dgrad", "wgrad")

# op: fwd / dgrad / wgrad.  store: how x (fwd, wgrad) or dx (dgrad) lives in memory, "bf16" or "f32".  route: "stream" or "generic".
# grid: (NB, n_slots) of a streaming weight gradient, else None.  why: for a generic case, what keeps it off the streaming kernels
# ("G", "HW", "C" or "storage").
Case = collections.namedtuple("Case", "op B G H W C store route grid why")

# ---- streaming forward and input gradient (C = 64): tiles = B HW / 128 over min(tiles, 256) persistent workgroups
FD_SHAPES = [(1, 8, 16),          # 1 tile
             (1, 16, 16),         # 2 tiles of one sample
             (3, 8, 16),          # 3 tiles, one per sample
             (257, 8, 16),        # 257: workgroup 0 walks two tiles, the others one
             (33, 32, 32),        # 264: workgroups 0 .. 7 walk two
             (32, 32, 64)]        # 512: two each, non-square map
FD_SHAPES_G2 = [(65, 32, 32),     # 520: workgroups 0 .. 7 walk three tiles, the others two
                (256, 8, 16)]     # 256: exactly one tile for each of the 256 workgroups
CASES = [Case(op, B, G, H, W, 64, "bf16", "stream", None, None)
         for op in ("fwd", "dgrad") for G in (8, 4, 2) for (B, H, W) in FD_SHAPES + (FD_SHAPES_G2 if G == 2 else [])]

# ---- streaming weight gradient: (B, G, H, W, C, NB, n_slots)
WGRAD_STREAM = [(B, G, 8, 16, 64, 1, min(B, 256)) for G in (8, 4, 2) for B in (1, 3, 17, 257)]     # reduce4 over 1, 3, 17, 256 partials
WGRAD_STREAM += [
    (256, 2, 8, 16, 64, 1, 256),        # tiles == slots
    (32, 2, 32, 64, 64, 1, 256),        # 512 tiles: two per slot
    (1, 4, 8, 16, 128, 2, 1),           # C = 128, F = 8: NB = 2, one slot per block
    (65, 4, 16, 16, 128, 2, 128),       # 130 tiles over 128 slots
    (129, 2, 8, 16, 128, 2, 128),       # F = 4, 129 tiles
    (1, 1, 8, 16, 128, 2, 1),           # F = 2
    (65, 1, 16, 16, 128, 2, 128),
    (1, 2, 8, 16, 256, 4, 1),           # C = 256, F = 8: NB = 4
    (32, 2, 16, 16, 256, 4, 64),        # 64 tiles == 64 slots
    (33, 2, 16, 16, 256, 4, 64),        # 66 tiles
    (65, 1, 8, 16, 256, 4, 64),         # F = 4 with SUB = 4
]
CASES += [Case("wgrad", B, G, H, W, C, "bf16", "stream", (NB, ns), None) for (B, G, H, W, C, NB, ns) in WGRAD_STREAM]

# ---- the generic engine at the shapes that fall through: (G, H, W, C, store, why for fwd and dgrad, why for wgrad)
GENERIC = [(6, 16, 16, 64, "bf16", "G", "G"),
           (8, 8, 8, 64, "bf16", "HW", "HW"),
           (1, 16, 16, 64, "bf16", "G", "G"),
           (3, 16, 16, 128, "bf16", "C", "G"),          # the weight gradient would take C = 128 with G = 4, 2 or 1
           (8, 16, 16, 128, "bf16", "C", "G"),          # F = 16 virtual frames
           (4, 16, 16, 64, "f32", "storage", "storage")]
CASES += [Case(op, 3, G, H, W, C, store, "generic", None, wg if op == "wgrad" else wf)
          for op in OPS for (G, H, W, C, store, wf, wg) in GENERIC]


def case_id(c):
    return "%s-%s-%s-B%d-G%d-%dx%d-C%d" % (c.op, c.route, c.store, c.B, c.G, c.H, c.W, c.C)


def tiles_of(c):
    return c.B * (c.H * c.W // 128)


def route_of(L, c):
    """(route, NB * n_slots or None) from the library's answers; a streaming kernel takes bf16 storage only."""
    HW = c.H * c.W
    if c.op == "wgrad":
        if c.store == "bf16" and L.hupr_tmerge_wgrad_stream_supported(c.G, HW, c.C, c.C):
            F_ = c.G * (c.C // 64)
            nbytes = L.hupr_tmerge_wgrad_stream_ws_bytes(c.B, c.G, HW, c.C, c.C)
            assert nbytes > 0 and nbytes % (64 * 64 * F_ * 4) == 0
            return "stream", nbytes // (64 * 64 * F_ * 4)
        return "generic", None
    if c.store == "bf16" and L.hupr_tmerge_stream_supported(c.G, HW, c.C, c.C):
        return "stream", None
    return "generic", None


def expected_route(c):
    return c.route, (c.grid[0] * c.grid[1] if c.grid else None)


# ---- the fp64 reference and the gate (any device) ----------------------------------------------------------------------------
def q(t):
    """Rounded to bf16 (nearest even), as fp64."""
    return t.to(torch.bfloat16).double()


def fwd_ref(x, wq):
    """x [B, G, V, Ci], wq [Co, Ci, G] fp64 -> (ref, A) [B, V, Co]."""
    xd = x.double()
    return torch.einsum("bgvc,ocg->bvo", xd, wq), torch.einsum("bgvc,ocg->bvo", xd.abs(), wq.abs())


def dgrad_ref(dyq, wq):
    """dyq [B, V, Co] fp64, wq [Co, Ci, G] fp64 -> (ref, A) [B, G, V, Ci]."""
    return torch.einsum("bvo,ocg->bgvc", dyq, wq), torch.einsum("bvo,ocg->bgvc", dyq.abs(), wq.abs())


def wgrad_ref(x, dyq):
    """x [B, G, V, Ci], dyq [B, V, Co] fp64 -> (ref, A) in the parameter layout [Co, Ci, G]."""
    xd = x.double()
    return torch.einsum("bvo,bgvc->ocg", dyq, xd), torch.einsum("bvo,bgvc->ocg", dyq.abs(), xd.abs())


def within(out, ref, A, c, bf16_store):
    """True where out meets the gate (a NaN never does)."""
    lim = c * A
    if bf16_store:
        lim = lim + 2.0 ** -8 * ref.abs()
    return (out.double() - ref).abs() <= lim


def measured(out, ref, A, bf16_store):
    """Worst err / A.  Behind a bf16 store the error of the fp32 sum shows only where it moved the sum across a rounding border: where
    the stored value is not the bf16 nearest to ref, the sum was at least |ref - midpoint of the two| off; together with any excess of
    the error over 2^-8 |ref| (the bound of one round-to-nearest-even store), over A.  A NaN gives inf."""
    err = (out.double() - ref).abs()
    if bf16_store:
        nearest = ref.to(torch.bfloat16).double()
        moved = (ref - (out.double() + nearest) / 2).abs() * (out.double() != nearest)
        err = torch.maximum(moved, err - 2.0 ** -8 * ref.abs()).clamp_min(0.0)            # (a NaN stays one)
    return (err / A).nan_to_num(float("inf")).max().item()


WORST = {}             # (op, route) -> worst measured value of this session (printed per case: pytest -s shows the measurements)


def assert_within(out, ref, A, op, bf16_store, what, route=None):
    worst = measured(out, ref, A, bf16_store)
    if route is not None:
        WORST[(op, route)] = max(WORST.get((op, route), 0.0), worst)
        print("tmerge fp64: %-46s worst %.3g = 2^%.2f   (so far %s %s: 2^%.2f)" % (
            what, worst, torch.log2(torch.tensor(worst)).item(), op, route, torch.log2(torch.tensor(WORST[(op, route)])).item()))
    ok = within(out, ref, A, GATE_C[op], bf16_store)
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d outside the gate, first at %s (out %r, ref %r, A %r), measured worst %.3g (c %.3g)"
                             % (what, bad.shape[0], ok.numel(), i, out[i].item(), ref[i].item(), A[i].item(), worst, GATE_C[op]))


def make_operands(B, G, H, W, C):
    """Seeded CPU operands of a shape: x [B, G, HW, C] bf16, the parameter w [C, C, G] fp32 and dy [B, HW, C] fp32 (NOT
    bf16-representable: the kernels round it)."""
    seed = 1000 * B + 100 * G + 3 * H + W + C
    x = rnd(B, G, H * W, C, seed=seed).to(torch.bfloat16)
    w = rnd(C, C, G, seed=seed + 1, scale=(C * G) ** -0.5)
    dy = rnd(B, H * W, C, seed=seed + 2)
    return x, w, dy


# ---- operands on the device, NaN-guarded buffers, the launches (GPU) ----------------------------------------------------------
def packed_weights(L, w):
    """{("bf16" | "f32", mode)}: hupr_pack_conv_weights_bf16 / _f32 of the parameter w [Co, Ci, G] in modes 0 and 1, each checked against
    the layout the kernels read: mode 0 [co][g][ci], mode 1 [ci][G - 1 - g][co]."""
    from hupr_amd import runtime as rt
    C, _, G = w.shape
    out = {}
    for kind, fn, dt in (("bf16", L.hupr_pack_conv_weights_bf16, torch.bfloat16), ("f32", L.hupr_pack_conv_weights_f32, torch.float32)):
        for mode in (0, 1):
            wp = nan_buffer(C * C * G + GUARD, dt)
            assert fn(rt.ptr(w), rt.ptr(wp), C, C, G, mode, rt.stream()) == 0, L.hupr_last_error()
            torch.cuda.synchronize()
            assert bool((bits(wp[C * C * G:]) == (NAN16 if dt == torch.bfloat16 else NAN32)).all())
            want = w.to(dt).permute(0, 2, 1) if mode == 0 else w.to(dt).permute(1, 2, 0).flip(1)
            assert torch.equal(wp[:C * C * G].view(C, G, C), want.contiguous()), (kind, mode)
            out[(kind, mode)] = wp
    return out


@functools.lru_cache(maxsize=None)
def operands(B, G, H, W, C):
    """The operands of a shape on the device, shared (and left unchanged) by every case on it."""
    from hupr_amd import runtime as rt
    x, w, dy = make_operands(B, G, H, W, C)
    o = {"x": padded(x, C, torch.bfloat16), "dy": padded(dy, C, torch.float32), "w": w.cuda(), "nx": x.numel(), "ndy": dy.numel()}
    o["xv"] = o["x"][:o["nx"]].view(B, G, H * W, C)
    o["dyq"] = q(o["dy"][:o["ndy"]]).view(B, H * W, C)
    o["wq"] = q(o["w"])
    o["wp"] = packed_weights(rt.lib(), o["w"])
    return o


def x_f32(o):
    if "x32" not in o:
        o["x32"] = padded(o["xv"].float(), o["xv"].shape[-1], torch.float32)
    return o["x32"]


def reference(c, o):
    if c.op == "fwd":
        return fwd_ref(o["xv"], o["wq"])
    if c.op == "dgrad":
        return dgrad_ref(o["dyq"], o["wq"])
    if "wgrad_ref" not in o:
        o["wgrad_ref"] = wgrad_ref(o["xv"], o["dyq"])
    return o["wgrad_ref"]


def out_shape(c):
    HW = c.H * c.W
    return {"fwd": (c.B, HW, c.C), "dgrad": (c.B, c.G, HW, c.C), "wgrad": (c.C, c.C, c.G)}[c.op]


def out_dtype(c):
    return torch.bfloat16 if c.op == "dgrad" and c.store == "bf16" else torch.float32


def guarded(n, dtype):
    """guard | n elements | guard in the NaN pattern; the view starts 512 (bf16) / 1024 (fp32) bytes into the allocation."""
    buf = nan_buffer(GUARD + n + GUARD, dtype)
    return buf, buf[GUARD:GUARD + n]


def assert_guards(buf, n, what):
    nan = NAN16 if buf.dtype == torch.bfloat16 else NAN32
    assert bool((bits(buf[:GUARD]) == nan).all()), "%s: the guard in front of the output was written" % what
    assert bool((bits(buf[GUARD + n:]) == nan).all()), "%s: the guard past the output was written" % what


def ws_bytes_of(L, c):
    if c.op != "wgrad":
        return 0
    if c.route == "stream":
        return L.hupr_tmerge_wgrad_stream_ws_bytes(c.B, c.G, c.H * c.W, c.C, c.C)
    return L.hupr_conv_wgrad_ws_bytes(c.B, 1, c.H, c.W, c.C, c.C, c.G, 1, 1)


def ws_buffer(nbytes):
    """Exactly nbytes of workspace in the NaN pattern (a partial that is read before it is written shows) + a guard."""
    assert nbytes % 4 == 0
    return nan_buffer(nbytes // 4 + GUARD, torch.float32)


def call(L, c, x, dy, wp, out, ws=None, nbytes=0, geo=None):
    """One call of the entry point the case's route names.  x / dy: the stored operand buffers, wp: the dictionary of packings, out: the
    output view; geo: (B, G, HW, Ci, Co) if it is to differ from the case's (refused calls)."""
    from hupr_amd import runtime as rt
    B, G, HW, Ci, Co = geo or (c.B, c.G, c.H * c.W, c.C, c.C)
    xbf = int(c.store == "bf16")
    s = rt.stream()
    if c.route == "stream":
        if c.op == "fwd":
            rc = L.hupr_tmerge_fwd_stream_bf16(x.data_ptr(), wp[("bf16", 0)].data_ptr(), out.data_ptr(), B, G, HW, Ci, Co, s)
        elif c.op == "dgrad":
            rc = L.hupr_tmerge_dgrad_stream_bf16(dy.data_ptr(), wp[("bf16", 1)].data_ptr(), out.data_ptr(), B, G, HW, Ci, Co, s)
        else:
            rc = L.hupr_tmerge_wgrad_stream_bf16(x.data_ptr(), dy.data_ptr(), out.data_ptr(), B, G, HW, Ci, Co, ws.data_ptr(), nbytes, s)
    else:
        if c.op == "fwd":
            rc = L.hupr_conv_fwd_bf16_mixed(x.data_ptr(), xbf, wp[("f32", 0)].data_ptr(), None, out.data_ptr(), 0, B, G, c.H, c.W, Ci, Ci,
                                            1, c.H, c.W, Co, Co, G, 1, 1, 0, 0, 0, s)
        elif c.op == "dgrad":
            rc = L.hupr_tmerge_dgrad_bf16(dy.data_ptr(), wp[("f32", 1)].data_ptr(), out.data_ptr(), xbf, B, G, HW, Ci, Co, s)
        else:
            rc = L.hupr_conv_wgrad_bf16_mixed(x.data_ptr(), xbf, dy.data_ptr(), out.data_ptr(), B, G, c.H, c.W, Ci, Ci, 1, c.H, c.W, Co,
                                              Co, G, 1, 1, 0, 0, 0, ws.data_ptr(), nbytes, s)
    torch.cuda.synchronize()
    return rc


def run(L, c, o, what):
    """One guarded launch of the case: the output view, with the guards around it and past the workspace verified."""
    n = 1
    for d in out_shape(c):
        n *= d
    buf, out = guarded(n, out_dtype(c))
    nbytes = ws_bytes_of(L, c)
    ws = ws_buffer(nbytes) if c.op == "wgrad" else None
    x = o["x"] if c.store == "bf16" else x_f32(o)
    rc = call(L, c, x, o["dy"], o["wp"], out, ws, nbytes)
    assert rc == 0, L.hupr_last_error()
    assert_guards(buf, n, what)
    if ws is not None:
        assert bool((bits(ws[nbytes // 4:]) == NAN32).all()), "%s: the guard past the workspace was written" % what
    assert not bool(out.isnan().any()), "%s: an output element was left NaN" % what
    return out.view(*out_shape(c))


@pytest.fixture
def lib():
    from hupr_amd import runtime
    return runtime.lib()


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_tmerge_form_matches_fp64(c, lib):
    """The routed kernel against fp64 under the gate, every element; guards untouched, nothing left NaN; the same bits from a second
    launch; the launch count of the route."""
    assert route_of(lib, c) == expected_route(c)
    o = operands(c.B, c.G, c.H, c.W, c.C)
    ref, A = reference(c, o)
    n0 = lib.hupr_launch_count()
    out = run(lib, c, o, case_id(c))
    if c.route == "stream":
        assert lib.hupr_launch_count() - n0 == (2 if c.op == "wgrad" else 1)
    assert_within(out, ref, A, c.op, out.dtype == torch.bfloat16, case_id(c), c.route)
    out2 = run(lib, c, o, case_id(c))
    assert torch.equal(bits(out2), bits(out)), "two launches differ"


# ---- exact-index regime: one-hot operands, bit-exact expectations -----------------------------------------------------------------
def one_hot_rows(B, V, C, key, device="cuda"):
    """[B, V, C] fp32 with a single 1 per voxel row at channel key[v]."""
    t = torch.zeros(B, V, C, device=device)
    t.scatter_(2, key.view(1, V, 1).expand(B, V, 1), 1.0)
    return t


@pytest.mark.parametrize("G", [8, 4, 2])
def test_one_hot_forward_reads_every_weight_exactly(G, lib):
    """x[b, g, v, ci] = 1 where ci == v % 64 and g == (v // 64) % G, else 0: the merged map must be the bf16-rounded
    W[co][v % 64][(v // 64) % G] bit for bit (24 tiles, 3 samples of 32 x 32)."""
    B, H, W, C = 3, 32, 32, 64
    V = H * W
    c = Case("fwd", B, G, H, W, C, "bf16", "stream", None, None)
    assert route_of(lib, c) == ("stream", None)
    v = torch.arange(V, device="cuda")
    rows = one_hot_rows(B, V, C, v % 64)
    x = torch.zeros(B, G, V, C, device="cuda")
    for g in range(G):
        x[:, g] = rows * ((v // 64) % G == g).view(1, V, 1)
    o = operands(B, G, H, W, C)
    buf, y = guarded(B * V * C, torch.float32)
    assert call(lib, c, padded(x, C, torch.bfloat16), None, o["wp"], y) == 0, lib.hupr_last_error()
    assert_guards(buf, B * V * C, "one-hot forward")
    want = o["w"].to(torch.bfloat16).float()[:, v % 64, (v // 64) % G].t().expand(B, V, C).contiguous()       # [b][v][co]
    bad = (bits(y.view(B, V, C)) != bits(want)).nonzero()
    assert bad.numel() == 0, "G = %d: %d elements differ, first (b, v, co) = %s" % (G, bad.shape[0], bad[0].tolist())


@pytest.mark.parametrize("G", [8, 4, 2])
def test_one_hot_input_gradient_reads_every_weight_exactly(G, lib):
    """dy[b, v, co] = 1 where co == v % 64: dx[b, g, v, ci] must be the bf16-rounded W[v % 64][ci][g] bit for bit."""
    B, H, W, C = 3, 32, 32, 64
    V = H * W
    c = Case("dgrad", B, G, H, W, C, "bf16", "stream", None, None)
    assert route_of(lib, c) == ("stream", None)
    v = torch.arange(V, device="cuda")
    dy = one_hot_rows(B, V, C, v % 64)
    o = operands(B, G, H, W, C)
    n = B * G * V * C
    buf, dx = guarded(n, torch.bfloat16)
    assert call(lib, c, None, padded(dy, C, torch.float32), o["wp"], dx) == 0, lib.hupr_last_error()
    assert_guards(buf, n, "one-hot input gradient")
    want = o["w"].to(torch.bfloat16)[v % 64].permute(2, 0, 1).expand(B, G, V, C).contiguous()          # [v][ci][g] -> [b][g][v][ci]
    bad = (bits(dx.view(B, G, V, C)) != bits(want)).nonzero()
    assert bad.numel() == 0, "G = %d: %d elements differ, first (b, g, v, ci) = %s" % (G, bad.shape[0], bad[0].tolist())


@pytest.mark.parametrize("G", [8, 4, 2])
def test_one_hot_weight_gradient_is_exact(G, lib):
    """dy[b, v, co] = p[b, v] at co == v % 64 and x[b, g, v, ci] = r[b, g, v] at ci == (v // 64) % 64 with small integers p, r on a
    64 x 64 map: every (co, ci) pair meets at exactly one voxel per sample, the sums are small integers, exact in any order —
    dW[co][ci][g] must equal sum_b p[b, v*] r[b, g, v*] at v* = 64 ci + co exactly."""
    B, H, W, C = 2, 64, 64, 64
    V = H * W
    c = Case("wgrad", B, G, H, W, C, "bf16", "stream", (1, 64), None)
    assert route_of(lib, c) == ("stream", 64)
    gen = torch.Generator().manual_seed(40 + G)
    p = torch.randint(-8, 9, (B, V), generator=gen).float().cuda()
    r = torch.randint(-8, 9, (B, G, V), generator=gen).float().cuda()
    v = torch.arange(V, device="cuda")
    dy = one_hot_rows(B, V, C, v % 64) * p.view(B, V, 1)
    x = one_hot_rows(B, V, C, (v // 64) % 64).view(B, 1, V, C) * r.view(B, G, V, 1)
    n = C * C * G
    buf, dw = guarded(n, torch.float32)
    nbytes = ws_bytes_of(lib, c)
    ws = ws_buffer(nbytes)
    assert call(lib, c, padded(x, C, torch.bfloat16), padded(dy, C, torch.float32), None, dw, ws, nbytes) == 0, lib.hupr_last_error()
    assert_guards(buf, n, "one-hot weight gradient")
    assert bool((bits(ws[nbytes // 4:]) == NAN32).all())
    vs = (torch.arange(C, device="cuda").view(1, C) * 64 + torch.arange(C, device="cuda").view(C, 1)).reshape(-1)    # [co][ci] -> v*
    want = (p[:, None, vs] * r[:, :, vs]).sum(0).view(G, C, C).permute(1, 2, 0).contiguous()
    got = dw.view(C, C, G)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, "G = %d: %d elements differ, first (co, ci, g) = %s" % (G, bad.shape[0], bad[0].tolist())
    ref, _ = wgrad_ref(x, dy.double().view(B, V, C))
    assert torch.equal(want.double(), ref)


# ---- refused calls ------------------------------------------------------------------------------------------------------------------
# (what, op, route, (B, G, HW, Ci, Co), byte offset added to (x, dy, w, out, ws), workspace bytes relative to the library's figure)
OK_GEO = (1, 2, 128, 64, 64)
REFUSED = []
for _op in OPS:
    REFUSED += [("%s: G = 6" % _op, _op, "stream", (1, 6, 128, 64, 64), (0, 0, 0, 0, 0), 0),
                ("%s: HW = 192" % _op, _op, "stream", (1, 2, 192, 64, 64), (0, 0, 0, 0, 0), 0),
                ("%s: Ci != Co" % _op, _op, "stream", (1, 2, 128, 64, 128), (0, 0, 0, 0, 0), 0),
                ("%s: output misaligned by 4 bytes" % _op, _op, "stream", OK_GEO, (0, 0, 0, 4, 0), 0)]
REFUSED += [("fwd: x misaligned by 4 bytes", "fwd", "stream", OK_GEO, (4, 0, 0, 0, 0), 0),
            ("fwd: weights misaligned by 4 bytes", "fwd", "stream", OK_GEO, (0, 0, 4, 0, 0), 0),
            ("dgrad: dy misaligned by 4 bytes", "dgrad", "stream", OK_GEO, (0, 4, 0, 0, 0), 0),
            ("dgrad: weights misaligned by 4 bytes", "dgrad", "stream", OK_GEO, (0, 0, 4, 0, 0), 0),
            ("wgrad: x misaligned by 4 bytes", "wgrad", "stream", OK_GEO, (4, 0, 0, 0, 0), 0),
            ("wgrad: dy misaligned by 4 bytes", "wgrad", "stream", OK_GEO, (0, 4, 0, 0, 0), 0),
            ("wgrad: workspace misaligned by 4 bytes", "wgrad", "stream", OK_GEO, (0, 0, 0, 0, 4), 0),
            ("wgrad: workspace one byte short", "wgrad", "stream", OK_GEO, (0, 0, 0, 0, 0), -1),
            ("wgrad: workspace one byte short, 256 slots of C = 256", "wgrad", "stream", (64, 2, 128, 256, 256), (0, 0, 0, 0, 0), -1),
            ("fwd: x of 2^31 bytes", "fwd", "stream", (16384, 8, 128, 64, 64), (0, 0, 0, 0, 0), 0),
            ("fwd: x of 2^31 bytes, G = 2", "fwd", "stream", (65536, 2, 128, 64, 64), (0, 0, 0, 0, 0), 0),
            ("wgrad: x of 2^31 bytes", "wgrad", "stream", (16384, 8, 128, 64, 64), (0, 0, 0, 0, 0), 0),
            ("wgrad: dy of 2^31 bytes", "wgrad", "stream", (16384, 1, 128, 256, 256), (0, 0, 0, 0, 0), 0),
            ("generic dgrad: Bn G = 65536", "dgrad", "generic", (8192, 8, 128, 64, 64), (0, 0, 0, 0, 0), 0)]
assert 16384 * 8 * 128 * 64 * 2 == 1 << 31 and 65536 * 2 * 128 * 64 * 2 == 1 << 31 and 16384 * 128 * 256 * 4 == 1 << 31


def refused_call(L, r, x, dy, w, out, ws, stream):
    """The refused call on the given base addresses (integers): every one is rejected by host checks, nothing is dereferenced."""
    what, op, route, (B, G, HW, Ci, Co), off, ws_delta = r
    x, dy, w, out, ws = (p + d for p, d in zip((x, dy, w, out, ws), off))
    if route == "generic":
        return L.hupr_tmerge_dgrad_bf16(dy, w, out, 1, B, G, HW, Ci, Co, stream)
    if op == "fwd":
        return L.hupr_tmerge_fwd_stream_bf16(x, w, out, B, G, HW, Ci, Co, stream)
    if op == "dgrad":
        return L.hupr_tmerge_dgrad_stream_bf16(dy, w, out, B, G, HW, Ci, Co, stream)
    nbytes = L.hupr_tmerge_wgrad_stream_ws_bytes(B, G, HW, Ci, Co) or (1 << 20)          # (0 for an unsupported geometry)
    return L.hupr_tmerge_wgrad_stream_bf16(x, dy, out, B, G, HW, Ci, Co, ws, nbytes + ws_delta, stream)


@pytest.mark.parametrize("r", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_calls_leave_everything_untouched(r, lib):
    """Calls the launchers refuse return HUPR_ERR_ARG or HUPR_ERR_WORKSPACE before any launch: the output, the workspace and their
    guards keep the NaN pattern bit for bit and hupr_launch_count() does not move.  (All buffers are those of a one-tile call: the
    refusals are host checks — tests/test_tmerge_route.py verifies that without a device.)"""
    from hupr_amd import runtime as rt
    what, op, route = r[:3]
    n = 1 << 16
    x = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    dy = torch.zeros(n, dtype=torch.float32, device="cuda")
    w = torch.zeros(n, dtype=torch.float32, device="cuda")
    buf, out = guarded(n, torch.bfloat16 if op == "dgrad" else torch.float32)
    ws = nan_buffer(n, torch.float32)
    n0 = lib.hupr_launch_count()
    rc = refused_call(lib, r, x.data_ptr(), dy.data_ptr(), w.data_ptr(), out.data_ptr(), ws.data_ptr(), rt.stream())
    torch.cuda.synchronize()
    assert rc in (HUPR_ERR_ARG, HUPR_ERR_WORKSPACE), (what, rc)
    assert lib.hupr_launch_count() == n0, what
    assert bool((bits(buf) == (NAN16 if buf.dtype == torch.bfloat16 else NAN32)).all()), what
    assert bool((bits(ws) == NAN32).all()), what


# ---- through functional.py ----------------------------------------------------------------------------------------------------------
STREAM_ENTRIES = ("hupr_tmerge_fwd_stream_bf16", "hupr_tmerge_dgrad_stream_bf16", "hupr_tmerge_wgrad_stream_bf16")
GENERIC_ENTRIES = ("hupr_conv_fwd_bf16_mixed", "hupr_tmerge_dgrad_bf16", "hupr_conv_wgrad_bf16_mixed")


class Counted:
    """The six merge entry points of rt.lib() wrapped by call counters for the block."""

    def __init__(self, L):
        self.L, self.n, self.orig = L, collections.Counter(), {}

    def __enter__(self):
        for name in STREAM_ENTRIES + GENERIC_ENTRIES:
            self.orig[name] = orig = getattr(self.L, name)

            def f(*a, _name=name, _orig=orig):
                self.n[_name] += 1
                return _orig(*a)
            setattr(self.L, name, f)
        return self

    def __exit__(self, *exc):
        for name, orig in self.orig.items():
            setattr(self.L, name, orig)

    def take(self):
        n, self.n = dict(self.n), collections.Counter()
        return n


@pytest.fixture
def bf16_math():
    from hupr_amd import functional as F_
    F_.set_math("bf16")
    yield
    F_.set_math("f32")
    F_.TMERGE_STREAM = True


def _node_operands(G):
    B, H, W, C = 3, 16, 16, 64
    o = operands(B, G, H, W, C)
    x = o["xv"].reshape(B, G, H, W, C).clone().requires_grad_(True)
    w = o["w"].reshape(C, C, G, 1, 1).clone().requires_grad_(True)
    dy = o["dy"][:o["ndy"]].view(B, 1, H, W, C).clone()
    return (B, H, W, C), o, x, w, dy


@pytest.mark.parametrize("G,stream", [(4, True), (2, True), (4, False)], ids=["G4", "G2", "G4-TMERGE_STREAM-off"])
def test_temporal_merge_node_calls_each_entry_once(G, stream, lib, bf16_math):
    """TemporalMergeFn at (G, 16 x 16, C = 64): one call of each streaming entry point per forward / backward and none of the generic
    ones — with TMERGE_STREAM off exactly the reverse — and all three results inside the gates."""
    from hupr_amd import functional as F_
    (B, H, W, C), o, x, w, dy = _node_operands(G)
    want, other = (STREAM_ENTRIES, GENERIC_ENTRIES) if stream else (GENERIC_ENTRIES, STREAM_ENTRIES)
    F_.TMERGE_STREAM = stream
    with Counted(lib) as n:
        y = F_.TemporalMergeFn.apply(x, w)
        assert n.take() == {want[0]: 1}
        y.backward(dy)
        assert n.take() == {want[1]: 1, want[2]: 1}
    torch.cuda.synchronize()
    what = "TemporalMergeFn G = %d%s" % (G, "" if stream else " (generic)")
    assert_within(y.detach().view(B, H * W, C), *fwd_ref(o["xv"], o["wq"]), "fwd", False, what + " forward")
    assert x.grad.dtype == torch.bfloat16
    assert_within(x.grad.view(B, G, H * W, C), *dgrad_ref(o["dyq"], o["wq"]), "dgrad", True, what + " dx")
    assert_within(w.grad.view(C, C, G), *wgrad_ref(o["xv"], o["dyq"]), "wgrad", False, what + " dW")


@pytest.mark.parametrize("G", [4, 2])
def test_merge_down_node_calls_each_entry_once_and_dx_matches_fp64(G, lib, bf16_math):
    """MergeDownFn at (G, 16 x 16, C = 64) with the half-size resampling as second consumer: each streaming entry point once, no
    generic one; merged map and dW inside their gates; dx against fp64 of merge gradient M + resampling gradient R.  The merge writes
    M as bf16 (error e1 <= 2^-8 |M| + c A_M, the input-gradient gate), the resampling backward adds its fp32 gather sum onto it
    (8 weighted terms per voxel at most, weights of three fp32 factors: e2 <= 2^-20 (A_R + |M|)) and stores once more as bf16:
    |dx - ref| <= 2^-8 |ref| + (1 + 2^-8) (e1 + e2)."""
    from hupr_amd import functional as F_
    (B, H, W, C), o, x, w, dy = _node_operands(G)
    size = (G // 2, H // 2, W // 2)
    dd = rnd(B, *size, C, seed=77 + G).to(torch.bfloat16).cuda()
    with Counted(lib) as n:
        merged, down = F_.MergeDownFn.apply(x, w, size)
        assert n.take() == {STREAM_ENTRIES[0]: 1}
        torch.autograd.backward((merged, down), (dy, dd))
        assert n.take() == {STREAM_ENTRIES[1]: 1, STREAM_ENTRIES[2]: 1}
    torch.cuda.synchronize()
    what = "MergeDownFn G = %d" % G
    assert_within(merged.detach().view(B, H * W, C), *fwd_ref(o["xv"], o["wq"]), "fwd", False, what + " forward")
    assert_within(w.grad.view(C, C, G), *wgrad_ref(o["xv"], o["dyq"]), "wgrad", False, what + " dW")
    M, AM = dgrad_ref(o["dyq"], o["wq"])

    def resampling_gradient(g):
        xr = torch.zeros(B, C, G, H, W, dtype=torch.float64, device="cuda", requires_grad=True)
        F.interpolate(xr, size=size, mode="trilinear", align_corners=True).backward(g.double().permute(0, 4, 1, 2, 3))
        return xr.grad.permute(0, 2, 3, 4, 1).reshape(B, G, H * W, C)
    R, AR = resampling_gradient(dd), resampling_gradient(dd.abs())
    ref = M + R
    e1 = 2.0 ** -8 * M.abs() + GATE_C["dgrad"] * AM
    e2 = 2.0 ** -20 * (AR + M.abs())
    lim = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * (e1 + e2)
    got = x.grad.view(B, G, H * W, C).double()
    ok = (got - ref).abs() <= lim
    assert bool(ok.all()), "%s dx: %d outside, worst err / bound %.3g" % (what, (~ok).sum().item(), ((got - ref).abs() / lim).max().item())


# ---- near the 32-bit bound of the buffer offsets -----------------------------------------------------------------------------------
BIG_G, BIG_HW, BIG_C = 8, (1 << 21) - 128, 64


@pytest.fixture(scope="module")
def big():
    """x of 2^31 - 2^17 bytes and its dy, generated on the device; freed after the two tests that use them."""
    assert BIG_G * BIG_HW * BIG_C * 2 == (1 << 31) - (1 << 17)
    gen = torch.Generator(device="cuda").manual_seed(31)
    o = {"x": torch.randn(BIG_G * BIG_HW * BIG_C, device="cuda", dtype=torch.bfloat16, generator=gen),
         "dy": torch.randn(BIG_HW * BIG_C, device="cuda", dtype=torch.float32, generator=gen)}
    small = operands(1, BIG_G, 8, 16, BIG_C)
    o["wp"], o["wq"] = small["wp"], small["wq"]
    yield o
    o.clear()
    torch.cuda.empty_cache()


def test_forward_just_under_the_32_bit_bound(big, lib):
    """16 383 tiles over 256 workgroups (63 or 64 tiles each; the last source offsets end 2^17 bytes under 2^31): the first and the last
    tile of every run of 2 048 tiles and the very last tile against fp64; nothing left NaN anywhere; guards untouched."""
    c = Case("fwd", 1, BIG_G, BIG_HW // 128, 128, BIG_C, "bf16", "stream", None, None)
    assert route_of(lib, c) == ("stream", None)
    n = BIG_HW * BIG_C
    buf, y = guarded(n, torch.float32)
    assert call(lib, c, big["x"], None, big["wp"], y) == 0, lib.hupr_last_error()
    assert_guards(buf, n, "forward near 2^31")
    assert not bool(y.isnan().any())
    n_tiles = BIG_HW // 128
    tiles = sorted({t for k in range(0, n_tiles, 2048) for t in (k, min(k + 2047, n_tiles - 1))} | {n_tiles - 1})
    vox = (torch.tensor(tiles, device="cuda").view(-1, 1) * 128 + torch.arange(128, device="cuda").view(1, -1)).reshape(-1)
    xs = big["x"].view(1, BIG_G, BIG_HW, BIG_C)[:, :, vox]
    ref, A = fwd_ref(xs, big["wq"])
    assert_within(y.view(1, BIG_HW, BIG_C)[:, vox], ref, A, "fwd", False, "forward near 2^31 (%d tiles)" % len(tiles), "stream")


def test_weight_gradient_just_under_the_32_bit_bound(big, lib):
    """The same x with its dy (2^29 - 2^15 bytes): 256 slots of 63 or 64 tiles, reduce4 over 256 partials; every element of dW against
    an fp64 reference summed on the device in 16 voxel chunks."""
    c = Case("wgrad", 1, BIG_G, BIG_HW // 128, 128, BIG_C, "bf16", "stream", (1, 256), None)
    assert route_of(lib, c) == ("stream", 256)
    n = BIG_C * BIG_C * BIG_G
    buf, dw = guarded(n, torch.float32)
    nbytes = ws_bytes_of(lib, c)
    ws = ws_buffer(nbytes)
    assert call(lib, c, big["x"], big["dy"], None, dw, ws, nbytes) == 0, lib.hupr_last_error()
    assert_guards(buf, n, "weight gradient near 2^31")
    assert bool((bits(ws[nbytes // 4:]) == NAN32).all())
    xv, dyv = big["x"].view(1, BIG_G, BIG_HW, BIG_C), big["dy"].view(1, BIG_HW, BIG_C)
    ref = torch.zeros(BIG_C, BIG_C, BIG_G, dtype=torch.float64, device="cuda")
    A = torch.zeros_like(ref)
    step = 1 << 17
    for v0 in range(0, BIG_HW, step):
        r, a = wgrad_ref(xv[:, :, v0:v0 + step], q(dyv[:, v0:v0 + step]))
        ref += r
        A += a
    assert_within(dw.view(BIG_C, BIG_C, BIG_G), ref, A, "wgrad", False, "weight gradient near 2^31", "stream")
