"""Encoder level 3 (D = 2, 16 x 16 maps, B = 32): the two-plane form of the 256-voxel kernel's 2 x 8 x 16 tile against the general
four-plane instantiation (hupr_debug_halo_two_plane(0)) at the four launch shapes of the training step: 128 -> 256 and 256 -> 256 with
fused statistics, 256 -> 256 plain and with a residual.  One process; after warm-up the switch alternates off / on in BLOCKS blocks of
N launches per form, HIP events around each block; per form the median and the range of the block means, and whether on < off by more
than the larger range.  usage (GPU box, repo root): python scripts/conv_two_plane_ab.py > profiles/conv_two_plane_ab.txt"""
import os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hupr_amd import functional as F_
F_.set_math("bf16")
rt, L = F_.rt, F_.rt.lib()
B, D, H, W = 32, 2, 16, 16
BLOCKS, N = 8, 100
g = torch.Generator(device="cuda").manual_seed(0)
SHAPES = [("128 -> 256 statistics", 128, 256, "stats"), ("256 -> 256 statistics", 256, 256, "stats"),
          ("256 -> 256 plain", 256, 256, ""), ("256 -> 256 residual", 256, 256, "res")]
def make(Ci, Co, kind):
    x = torch.randn(B, D, H, W, Ci, device="cuda", generator=g).bfloat16()
    wp = F_.pack_weights_bf16(torch.randn(Co, Ci, 3, 3, 3, device="cuda", generator=g) * (Ci * 27) ** -0.5, 0)
    y = torch.empty(B, D, H, W, Co, device="cuda", dtype=torch.bfloat16)
    res = torch.randn(B, D, H, W, Co, device="cuda", generator=g).bfloat16() if kind == "res" else None
    st = torch.empty(L.hupr_conv3x3_halo_stats_rows(), 2, Co, device="cuda", dtype=torch.float64) if kind == "stats" else None
    want = 6 if kind == "stats" else 8
    assert L.hupr_debug_halo_route(B, D, H, W, Ci, Ci, Co, Co, 3, 1, int(kind == "stats"), 0) == want
    if kind == "stats":
        return lambda: rt.check(L.hupr_conv3x3_halo_bf16act_stats(rt.ptr(x), rt.ptr(wp), rt.ptr(y), B, D, H, W, Ci, Ci, Co, Co, 3,
                                                                  rt.ptr(st), rt.stream())), y
    return lambda: rt.check(L.hupr_conv3x3_halo_bf16act(rt.ptr(x), rt.ptr(wp), None, rt.ptr(res), rt.ptr(y), B, D, H, W, Ci, Ci, Co, Co,
                                                        Co, 3, rt.stream())), y
def block(call, on):
    L.hupr_debug_halo_two_plane(on)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N * 1e3
try:
    print("B = %d, D = %d, %d x %d; %d blocks of %d launches per form, alternating; us per launch (block means)" % (B, D, H, W, BLOCKS, N))
    for name, Ci, Co, kind in SHAPES:
        call, y = make(Ci, Co, kind)
        outs = []
        for on in (0, 1, 0, 1):                                   # warm-up of both forms; equal bits
            block(call, on)
            outs.append(y.view(torch.int16).clone())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[3]), "the two forms store different bits"
        t = {0: [], 1: []}
        for _ in range(BLOCKS):
            for on in (0, 1):
                t[on].append(block(call, on))
        med = {k: statistics.median(v) for k, v in t.items()}
        rng = {k: max(v) - min(v) for k, v in t.items()}
        gf = 2 * 27 * Ci * Co * B * D * H * W / 1e9
        gain = med[0] - med[1]
        print("%-22s four planes %6.2f (%.2f .. %.2f)   two planes %6.2f (%.2f .. %.2f)   gain %5.2f us = %4.1f %%   %s   "
              "[%.0f -> %.0f TF/s of the useful products x 1.5 / x 1]"
              % (name, med[0], min(t[0]), max(t[0]), med[1], min(t[1]), max(t[1]), gain, 100 * gain / med[0],
                 "MET" if gain > max(rng.values()) else "NOT MET (gain <= larger range %.2f)" % max(rng.values()),
                 gf / med[0] * 1e3, gf / med[1] * 1e3))
finally:
    L.hupr_debug_halo_two_plane(1)
