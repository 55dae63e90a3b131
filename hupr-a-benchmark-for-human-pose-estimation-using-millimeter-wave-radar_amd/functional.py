"""autograd.Function wrappers: one forward/backward pair of C-ABI calls per operator, plus a few fused nodes where a
chain of reference operators is cheaper as one (MSCSALevelFn, TemporalMergeFn, DualConvFn, the two-branch BatchNorm tail).

Activations are channels-last 5-D tensors ``(B, D, H, W, C)`` (2-D maps use D == 1), contiguous, fp32 — or, with
bf16 math and ``ACT_BF16``, bf16-stored inside the encoders / decoder stacks (arithmetic and parameters stay fp32).
Parameters keep the reference's shapes; the packed layouts the convolution kernels read are cached per parameter and
refreshed by ONE table-driven launch per optimiser step (``weight_cache``; ``_packed`` / ``invalidate_packed``).  Parameter gradients
are written straight into the flat all-reduce buckets when a gradient sink is installed (``GRAD_SINK``).

Nothing here computes with torch ops except allocation, views, concatenation of small weight matrices and gradient
bookkeeping; every kernel is reached through ``runtime.lib()`` and fails loudly without the HIP library.
"""
import ctypes
import math
import os
import threading

import numpy as np
import torch

from . import runtime as rt
from . import weight_cache as wcache

_ws_cache = {}
CONV_PROBE = None      # bench.py installs a callable(x, co, k) -> (start_event, end_event) | None
# Precision state, per THREAD (two models driven from two threads of one process must not share one pipe selection).  ``_st.math`` =
# matrix-pipe arithmetic of the GEMM-shaped ops: "f32" (parity path) or "bf16"; ``_st.act_f32_here`` / ``_st.region_switched`` = inside a
# region switched to "f32act" / to the fp32 pipe.  ``set_math`` sets the calling thread's mode (and the default a thread that never chose
# one starts from), ``math_mode`` scopes it, ``HuPRNet.math_mode`` pins it per model, and every autograd node carries the state of its
# forward into its backward on whatever thread the engine runs it (``_math_scoped``).  ``F_.MATH`` etc. stay readable (module
# ``__getattr__``) and name the calling thread's values.
_DEFAULT_MATH = ["f32"]


class _State(threading.local):
    def __init__(self):            # runs once per thread, on its first access
        self.math = _DEFAULT_MATH[0]
        self.act_f32_here = False
        self.region_switched = False

    def get(self):
        return self.math, self.act_f32_here, self.region_switched

    def set(self, triple):
        self.math, self.act_f32_here, self.region_switched = triple


_st = _State()


def __getattr__(name):             # PEP 562: F_.MATH / F_._ACT_F32_HERE / F_._REGION_SWITCHED of the calling thread
    if name == "MATH":
        return _st.math
    if name == "_ACT_F32_HERE":
        return _st.act_f32_here
    if name == "_REGION_SWITCHED":
        return _st.region_switched
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
ACT_BF16 = True        # bf16 mode only: the 3-D encoders keep their activations in HBM as bf16 ("bf16act" kernels)
ACT_BF16_DECODER = True    # ... and so do the BasicBlock2D decoder stacks


def set_math(mode):
    """Select v_mfma_f32_32x32x2_f32 ("f32", exact) or the bf16 matrix pipe ("bf16", fp32 accumulate) for the CALLING thread, and as
    the mode threads that have not chosen one start from."""
    if mode not in ("f32", "bf16"):
        raise ValueError("math mode must be 'f32' or 'bf16'")
    _st.math = mode
    _DEFAULT_MATH[0] = mode


class math_mode:
    """``with math_mode("bf16"):`` — the calling thread's matrix-pipe mode for the block (nothing process-wide changes)."""

    def __init__(self, mode):
        if mode not in ("f32", "bf16"):
            raise ValueError("math mode must be 'f32' or 'bf16'")
        self.mode = mode

    def __enter__(self):
        self.prev = _st.get()
        _st.set((self.mode, False, False))
        return self

    def __exit__(self, *exc):
        _st.set(self.prev)
        return False


# Per-region precision inside a bf16 run: PRECISION[region] = "f32" runs that region of HuPRNet.forward on the fp32 matrix
# pipe with fp32-stored activations, "f32act" keeps the bf16 matrix pipe but leaves the region's activations fp32 in HBM
# (models/layers.py wraps its regions in ``region(name)``); casts happen at the region borders (``to_act``).  Every autograd
# node remembers the mode of its forward and restores it for its backward, so the switches hold for training too.
# scripts/precision_regions.py uses them to localise where the bf16 path loses arg-max agreement on a trained network
# (profiles/r03_precision_regions.txt): everything but the last decoder block and the 1x1 head is >= 99.8 % on its own, those
# two alone cost 2 % / 1.3 % of the first head's joints.  DEFAULT therefore: the last BasicBlock2D keeps fp32 activations and the
# 14-channel head runs on the fp32 pipe (first head 99.1 -> 99.8-100 % identical arg-max, decoded head's max-abs error 3.8e-2 ->
# 1.1e-2, for +0.4 ms / step).  HUPR_F32_REGIONS / HUPR_F32ACT_REGIONS (comma lists) replace the default; "none" clears it.
REGIONS = ("mnet", "enc1", "enc2", "enc3", "merge", "lvl0", "lvl1", "lvl2", "dec3", "dec2", "dec1a", "dec1b", "head")
if "HUPR_F32_REGIONS" in os.environ or "HUPR_F32ACT_REGIONS" in os.environ:
    PRECISION = {r: "f32" for r in os.environ.get("HUPR_F32_REGIONS", "").split(",") if r and r != "none"}
    PRECISION.update({r: "f32act" for r in os.environ.get("HUPR_F32ACT_REGIONS", "").split(",") if r and r != "none"})
else:
    PRECISION = {"dec1b": "f32act", "head": "f32"}
assert all(r in REGIONS for r in PRECISION), PRECISION


class region:
    """``with region("dec1"):`` — the ops inside follow PRECISION["dec1"] when the run is a bf16 run."""

    def __init__(self, name):
        assert name in REGIONS, name
        self.name = name

    def __enter__(self):
        self.prev = _st.get()
        mode = PRECISION.get(self.name)
        if _st.math == "bf16" and mode == "f32":
            _st.math = "f32"
            _st.region_switched = True
        _st.act_f32_here = _st.math == "bf16" and mode == "f32act"
        return self

    def __exit__(self, *exc):
        _st.set(self.prev)
        return False


def _math_scoped(cls):
    """Class decorator for the autograd nodes: the backward pass runs under the matrix-pipe mode of its forward."""
    fwd, bwd = cls.forward, cls.backward

    def forward(ctx, *a):
        ctx._hupr_math = _st.get()
        return fwd(ctx, *a)

    def backward(ctx, *g):
        # (the engine runs this on ITS thread: that thread's state is set from the node and restored afterwards)
        prev = _st.get()
        _st.set(ctx._hupr_math)
        try:
            return bwd(ctx, *g)
        finally:
            _st.set(prev)
    cls.forward, cls.backward = staticmethod(forward), staticmethod(backward)
    return cls


def _fn(stem):
    return getattr(rt.lib(), "hupr_%s_%s" % (stem, _st.math))


def act_bf16():
    """True when the encoder island stores activations as bf16 (bf16 math + ACT_BF16)."""
    return _st.math == "bf16" and ACT_BF16 and not _st.act_f32_here


def _act(stem, t):
    """C entry point of an activation-dtype-generic operator for tensor ``t`` (fp32 or bf16 storage)."""
    return getattr(rt.lib(), "hupr_%s_%s" % (stem, "bf16act" if t.dtype == torch.bfloat16 else "f32"))


def workspace(nbytes, device):
    """Stream-ordered scratch shared by all ops of one (device, stream): the two encoder branches may run on two streams."""
    key = (device.type, device.index, rt.stream() if device.type == "cuda" else 0)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _ws_args(ws):
    """(pointer, bytes) of an optional workspace."""
    return (rt.ptr(ws), ws.numel()) if ws is not None else (None, 0)


def _probe_begin(probe, *key):
    """Open a measured bracket on the current stream.  ``probe``: CONV_PROBE / ATTN_PROBE as the caller reads it at call time
    (bench.py installs and removes them between phases), a callable(*key) -> (start_event, end_event) | None."""
    ev = probe(*key) if probe is not None else None
    if ev is not None:
        ev[0].record()
    return ev


def _probe_end(ev):
    if ev is not None:
        ev[1].record()


# ---- two compute streams ------------------------------------------------------------------------------------------
# The horizontal and the vertical branch of HuPRNet (chirp net + 3-D encoder each) are independent until the decoder.
# On one stream the GPU idles through every kernel tail and every few-microsecond kernel (two whole training processes
# sharing one GPU reach 1.15x the throughput of one); with the vertical branch on a side stream — forward and, because
# autograd runs a node's backward on the stream of its forward, backward too — the two branches fill each other's gaps.
TWO_STREAMS = os.environ.get("HUPR_ONE_STREAM", "0") != "1"
_side_streams = {}


def side_stream(device):
    """The per-device side compute stream (created on first use)."""
    s = _side_streams.get(device.index)
    if s is None:
        s = _side_streams[device.index] = torch.cuda.Stream(device=device)
    return s


def side_streams_in_use(device):
    """Side streams that have been handed out for ``device`` (the all-reduce launcher waits for them as well)."""
    s = _side_streams.get(device.index)
    return [s] if s is not None else []


def two_streams_ok(t):
    return TWO_STREAMS and t.is_cuda


# The derived copies of the parameters that the kernels read (packed layouts, concatenated projections, the padded head filter) live
# in ``weight_cache``: ``invalidate_packed()`` after changing parameters behind torch's version counter, ``refresh_packed(device)``
# to refill the stale ones in place — in front of a two-stream fork, or before replaying a captured inference graph.
invalidate_packed = wcache.invalidate
refresh_packed = wcache.refresh


# Direct gradient sink (installed by tools.distributed.GradientBuckets): parameter gradients are written by the kernels
# straight into the flat-bucket views, the autograd Functions return None for them, and the 165 per-parameter
# AccumulateGrad add kernels of a step disappear.  Without a sink every Function returns ordinary gradient tensors.
GRAD_SINK = None
PRELU_DEFER = True         # test aid: False = every PReLU backward sums its slope gradient at once
BN_COUNTER_SINK = None      # list collecting the BatchNorm modules whose num_batches_tracked is due (tools.engine)


def _pgrad(param):
    """-> (tensor the kernel writes the gradient of ``param`` into, direct?)."""
    if GRAD_SINK is not None and param is not None:
        v = GRAD_SINK.take(param)
        if v is not None:
            return v, True
    return torch.empty_like(param), False


def _pret(param, g, direct):
    """Value a backward() returns for ``param``: None after a direct write (the sink is told the gradient landed)."""
    if direct:
        GRAD_SINK.done(param)
        return None
    return g


def _vox(x):
    """(B, D, H, W) extents and channel count of a channels-last 5-D tensor."""
    assert x.dim() == 5 and x.dtype in (torch.float32, torch.bfloat16), (x.shape, x.dtype)
    return x.shape[0], x.shape[1], x.shape[2], x.shape[3], x.shape[4]


def pack_weights(w, mode):
    co, ci = w.shape[0], w.shape[1]
    taps = int(np.prod(w.shape[2:]))
    wp = torch.empty(w.numel(), dtype=torch.float32, device=w.device)
    rt.check(rt.lib().hupr_pack_conv_weights_f32(rt.ptr(_c(w)), rt.ptr(wp), co, ci, taps, mode, rt.stream()))
    return wp


def pack_weights_bf16(w, mode):
    co, ci = w.shape[0], w.shape[1]
    taps = int(np.prod(w.shape[2:]))
    wp = torch.empty(w.numel(), dtype=torch.bfloat16, device=w.device)
    rt.check(rt.lib().hupr_pack_conv_weights_bf16(rt.ptr(_c(w)), rt.ptr(wp), co, ci, taps, mode, rt.stream()))
    return wp


def _alloc_packed(ws, kinds):
    pk = pack_weights_bf16 if kinds[0] == wcache.PACK_BF16 else pack_weights
    wp = (pk(ws[0], 0), pk(ws[0], 1))
    return wp, (wp,), True


_PACKED_KINDS = ((wcache.PACK_F32,), (wcache.PACK_BF16,))


def _packed(weight, mode, kind):
    """Packed layout ``mode`` (0 forward, 1 input gradient) of ``weight`` as fp32 (kind 0) or bf16 (kind 1): the cached pair of a
    parameter (``weight_cache``; an inference graph reads it too, ~60 pack launches less per replay), a single pack otherwise."""
    wp = wcache.lookup((weight,), _PACKED_KINDS[kind], _alloc_packed)
    if wp is None:
        return pack_weights_bf16(weight, mode) if kind else pack_weights(weight, mode)
    return wp[mode]


# The eight 1x1 projection weights of an MSCSA level as the two (4C, C) matrices its two GEMMs read — [phi_cross | theta_cross |
# phi_self | theta_self] per map — kept as ENTRIES OF THE PACK TABLE: the one table-driven launch after an optimiser step refreshes
# them with everything else.  Two copies per map: the plain one (backward GEMMs, GEMM-attention fallback) and the one whose query
# (theta) rows carry log2(e) for the QS attention kernels (csrc/attention_bf16.hip, kDeferBits).
_PROJ_KINDS = (wcache.COPY, wcache.COPY_LOG2E, wcache.COPY, wcache.COPY_LOG2E)
QS_ATTN = True             # test aid: False = the plain-Q kernels (fma per score)


def _alloc_proj(ws, kinds):
    C = ws[0].shape[0]
    wc = torch.empty((4 * C, C), dtype=torch.float32, device=ws[0].device)
    wq = torch.empty_like(wc)
    return (wc, wq), [(wc[j * C:(j + 1) * C], wq[j * C:(j + 1) * C]) for j in range(4)], False


def _proj_cat(ws, C):
    """-> (Wc, Wc_qs): (4C, C) fp32 concatenations of the four (C, C, 1, 1) projection weights ``ws`` of one map."""
    cat = wcache.lookup(ws, _PROJ_KINDS, _alloc_proj)
    if cat is None:
        wc = torch.cat([w.detach().reshape(C, C) for w in ws], 0)
        wq = wc.clone()
        wq[C:2 * C] *= 1.4426950408889634
        wq[3 * C:] *= 1.4426950408889634
        return wc, wq
    return cat


USE_FLASH = True       # bf16 mode: fused attention kernels where supported (C in {64,128}, N % 128 == 0)
USE_HALO = True        # bf16 mode: LDS halo-tiled kernel for 3x3(x3) "same" convolutions


def _halo_ok(x, k, pad, co=4):
    if _st.math != "bf16" or not USE_HALO or co % 4 != 0:
        return False
    B, Di, Hi, Wi, Ci = _vox(x)
    if x.dtype == torch.bfloat16 and Ci % 8 != 0:
        return False
    return bool(rt.lib().hupr_conv3x3_halo_supported(Di, Hi, Wi, Ci, k[0], k[1], k[2], pad[0], pad[1], pad[2]))


# BatchNorm statistics fused into the producing convolution (hupr_conv3x3_halo_bf16act_stats, 64-channel 3-D layers = the
# largest tensors of the step): the column sums wait here, keyed by the output's address, for the BatchNorm that consumes that
# tensor next (_bn_params pops them).  The kernel keeps running per-lane-pair sums in LDS and reduces across lanes once per launch:
# +6 us on a 222 us launch, -0.16 ms / +0.7 % frames/s per step measured in interleaved same-box runs -> ON by default
# (CONV_STATS = False switches it off: the parity tests compare the two).
CONV_STATS = True
ATTN_LEVEL_BATCH = True    # test aid: False = one launch per attention at every level
ATTN_PROBE = None          # measurement hook (bench.py): (kind, B, N, C) -> (start, end) events around one attention's launches, or None
_conv_stats = {}


def _conv_raw(x, weight, mode, bias, res, co, k, pad, out_extent, out=None, stats=False, infer=False):
    """weight: parameter-layout tensor (Co', Ci', taps...) packed here (mode 0 forward / 1 input gradient).
    out: write here instead of a fresh tensor (may be ``res`` itself: the epilogue reads a residual element right
    before the same lane overwrites it)."""
    B, Di, Hi, Wi, Ci = _vox(x)
    Do, Ho, Wo = out_extent
    y = torch.empty((B, Do, Ho, Wo, co), dtype=x.dtype, device=x.device) if out is None else out
    abf = x.dtype == torch.bfloat16
    L = rt.lib()
    if _halo_ok(x, k, pad, co):
        assert res is None or res.dtype == x.dtype
        wp = _packed(weight, mode, 1)
        ev = _probe_begin(CONV_PROBE, x, co, k)
        if (stats and CONV_STATS and abf and bias is None and res is None and out is None
                and L.hupr_conv3x3_halo_stats_supported(B, Di, Hi, Wi, Ci, co, k[0])):
            rows = L.hupr_conv3x3_halo_stats_rows()
            st = torch.empty((rows, 2, co), dtype=torch.float64, device=x.device)
            rt.check(L.hupr_conv3x3_halo_bf16act_stats(rt.ptr(x), rt.ptr(wp), rt.ptr(y), B, Di, Hi, Wi, Ci, Ci, co, co, k[0], rt.ptr(st),
                                                       rt.stream()))
            _conv_stats[y.data_ptr()] = (st, rows, B * Do * Ho * Wo, co)
            _probe_end(ev)
            return y
        # inference on small grids (config C2: B = 1): the reduction is sliced over workgroups, partial sums through a workspace
        nws = L.hupr_conv3x3_halo_splitk_ws_bytes(B, Di, Hi, Wi, Ci, co, k[0]) if (abf and infer) else 0
        if nws:
            ws = workspace(nws, x.device)
            rt.check(L.hupr_conv3x3_halo_bf16act_ws(rt.ptr(x), rt.ptr(wp), rt.ptr(bias), rt.ptr(res), rt.ptr(y), B, Di, Hi, Wi, Ci, Ci,
                                                    co, co, co, k[0], rt.ptr(ws), ws.numel(), rt.stream()))
        else:
            fn = L.hupr_conv3x3_halo_bf16act if abf else L.hupr_conv3x3_halo_bf16
            rt.check(fn(rt.ptr(x), rt.ptr(wp), rt.ptr(bias), rt.ptr(res), rt.ptr(y), B, Di, Hi, Wi, Ci, Ci, co, co, co, k[0], rt.stream()))
        _probe_end(ev)
        return y
    if abf:
        raise rt.HuprError("bf16-stored activations are only supported by the halo-tiled 3x3 convolutions "
                           "(shape %r, kernel %r); cast to fp32 first" % (tuple(x.shape), k))
    wp = _packed(weight, mode, 0)
    ev = _probe_begin(CONV_PROBE, x, co, k)
    rt.check(_fn("conv_fwd")(rt.ptr(x), rt.ptr(wp), rt.ptr(bias), rt.ptr(res), rt.ptr(y), B, Di, Hi, Wi, Ci, Ci, Do, Ho, Wo, co, co,
                             co, k[0], k[1], k[2], pad[0], pad[1], pad[2], 0, rt.stream()))
    _probe_end(ev)
    return y


class ConvPartial:
    """A K-sliced inference convolution that has not been summed yet: ``slices`` fp32 tensors (n, B, D, H, W, Co) for a consumer
    that sums them itself (``infer_tail``).  See hupr_conv3x3_halo_bf16act_partial in include/hupr.h."""
    __slots__ = ("slices", "n", "shape")

    def __init__(self, slices, n, shape):
        self.slices, self.n, self.shape = slices, n, shape


INFER_TAILS = True         # test aid


def infer_fast_ok(x):
    """Single-sample style inference on the bf16 path: no autograd, bf16-stored channels-last input, bf16 matrix pipe."""
    return INFER_TAILS and _st.math == "bf16" and not torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.bfloat16


def conv_infer_sliced(shape, weight, pad):
    """Would ``conv_infer`` K-slice this convolution (input extent ``shape`` = (B, D, H, W, Ci))?"""
    B, D, H, W, Ci = shape
    k = _ksize(weight)
    return bool(rt.lib().hupr_conv3x3_halo_supported(D, H, W, Ci, k[0], k[1], k[2], pad[0], pad[1], pad[2])) and \
        rt.lib().hupr_conv3x3_halo_splitk_ws_bytes(B, D, H, W, Ci, weight.shape[0], k[0]) > 0


def conv_infer(x, weight, pad):
    """Bias-free 3x3(x3) "same" convolution under ``infer_fast_ok``: a ConvPartial where the reduction is K-sliced (small grids),
    else the stored bf16 tensor."""
    x = _c(x)
    k = _ksize(weight)
    B, D, H, W, Ci = _vox(x)
    co = weight.shape[0]
    L = rt.lib()
    nws = L.hupr_conv3x3_halo_splitk_ws_bytes(B, D, H, W, Ci, co, k[0]) if _halo_ok(x, k, pad, co) else 0
    if not nws:
        return conv(x, weight, None, None, pad)
    n = nws // (B * D * H * W * co * 4)
    part = torch.empty((n, B, D, H, W, co), dtype=torch.float32, device=x.device)
    rt.check(L.hupr_conv3x3_halo_bf16act_partial(rt.ptr(x), rt.ptr(_packed(weight, 0, 1)), B, D, H, W, Ci, Ci, co, k[0],
                                                 rt.ptr(part), nws, rt.stream()))
    return ConvPartial(part, n, (B, D, H, W, co))


def _tail_side(t):
    """(pointer, slice count) of one input of ``infer_tail``: a ConvPartial's slices, a stored tensor (0 slices), or nothing."""
    if t is None:
        return None, 0
    return (rt.ptr(t.slices), t.n) if isinstance(t, ConvPartial) else (rt.ptr(_c(t)), 0)


def _bn_eval_args(bn):
    """(gamma, beta, running mean, running variance, eps) as an eval-mode kernel takes them; the null set for an absent second side."""
    if bn is None:
        return None, None, None, None, 0.0
    return rt.ptr(bn.weight), rt.ptr(bn.bias), rt.ptr(bn.running_mean), rt.ptr(bn.running_var), float(bn.eps)


def infer_tail(a, b=None, bn_a=None, bn_b=None, relu=False, prelu=None):
    """One launch for the elementwise tail of an inference block; ``a`` / ``b``: bf16 tensors or ConvPartials.
    BatchNorm form (bn_a given): relu?(bn_a(a) [+ bn_b(b)]) on running statistics; PReLU form: prelu(a [+ b])."""
    shape = a.shape
    C = shape[-1]
    M = int(np.prod(shape[:-1]))
    dev = (a.slices if isinstance(a, ConvPartial) else a).device
    y = torch.empty(tuple(shape), dtype=torch.bfloat16, device=dev)
    rt.check(rt.lib().hupr_infer_tail_bf16act(0 if bn_a is not None else 1, *_tail_side(a), *_bn_eval_args(bn_a), *_tail_side(b),
                                              *_bn_eval_args(bn_b), rt.ptr(prelu), 1 if relu else 0, rt.ptr(y), M, C, rt.stream()))
    return y


def _ksize(w):
    k = tuple(w.shape[2:])
    return (1,) + k if len(k) == 2 else k


def _dgrad_pad(k, pad):
    """Padding of the input-gradient convolution (the forward's taps reversed) of a stride-1 convolution."""
    return k[0] - 1 - pad[0], k[1] - 1 - pad[1], k[2] - 1 - pad[2]


def _halo_wgrad(x, dy, weight):
    """Weight gradient of a halo-tiled 3x3(x3) "same" convolution -> (dw in the parameter layout, written into the gradient sink?)."""
    B, D, H, W, Ci = _vox(x)
    Co, k0 = weight.shape[0], _ksize(weight)[0]
    L = rt.lib()
    dw, direct = _pgrad(weight)
    ws = workspace(L.hupr_conv3x3_wgrad_halo_ws_bytes(Ci, Co, k0), x.device)
    fn = L.hupr_conv3x3_wgrad_halo_bf16act if x.dtype == torch.bfloat16 else L.hupr_conv3x3_wgrad_halo_bf16
    rt.check(fn(rt.ptr(x), rt.ptr(dy), rt.ptr(dw), B, D, H, W, Ci, Ci, Co, Co, k0, rt.ptr(ws), ws.numel(), rt.stream()))
    return dw, direct


@_math_scoped
class ConvFn(torch.autograd.Function):
    """Stride-1 convolution (nn.Conv3d / nn.Conv2d of the reference) with optional bias and fused
    residual add.  ``pad`` is (pd, ph, pw)."""

    @staticmethod
    def forward(ctx, x, weight, bias, res, pad, want_stats=False, infer=False):
        x = _c(x)
        k = _ksize(weight)
        B, Di, Hi, Wi, Ci = _vox(x)
        assert weight.shape[1] == Ci, (weight.shape, x.shape)
        out_extent = (Di + 2 * pad[0] - k[0] + 1, Hi + 2 * pad[1] - k[1] + 1, Wi + 2 * pad[2] - k[2] + 1)
        y = _conv_raw(x, weight, 0, bias, _c(res) if res is not None else None, weight.shape[0], k, pad, out_extent,
                      stats=want_stats, infer=infer)
        ctx.save_for_backward(x, weight)
        ctx.bias_ref = bias                       # only its identity/shape is needed (gradient destination)
        ctx.pad, ctx.k, ctx.has_bias, ctx.has_res = pad, k, bias is not None, res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = _c(dy)
        assert dy.dtype == x.dtype, (dy.dtype, x.dtype)
        k, pad = ctx.k, ctx.pad
        B, Di, Hi, Wi, Ci = _vox(x)
        _, Do, Ho, Wo, Co = _vox(dy)
        L = rt.lib()
        dx = dw = db = None
        dw_direct = db_direct = False
        if ctx.needs_input_grad[0]:
            co_pad = Co
            dyp, wsrc = dy, weight
            if Co % 32 != 0:                      # e.g. the 14-channel head: zero-pad the K axis
                co_pad = (Co + 31) // 32 * 32
                dyp = torch.zeros((B, Do, Ho, Wo, co_pad), dtype=dy.dtype, device=dy.device)
                dyp[..., :Co] = dy
                wsrc = torch.zeros((co_pad,) + tuple(weight.shape[1:]), dtype=torch.float32, device=dy.device)
                wsrc[:Co] = weight
            dx = _conv_raw(dyp, wsrc, 1, None, None, Ci, k, _dgrad_pad(k, pad), (Di, Hi, Wi))      # packs [Ci][taps reversed][Co]
        if ctx.needs_input_grad[1] and _halo_ok(x, k, pad) and Ci % 32 == 0 and Co % 8 == 0:
            dw, dw_direct = _halo_wgrad(x, dy, weight)
        elif ctx.needs_input_grad[1] and x.dtype == torch.bfloat16:
            raise rt.HuprError("no bf16-activation weight-gradient kernel for shape %r" % (tuple(x.shape),))
        elif ctx.needs_input_grad[1]:
            dw, dw_direct = _pgrad(weight)
            ws = workspace(L.hupr_conv_wgrad_ws_bytes(B, Do, Ho, Wo, Ci, Co, k[0], k[1], k[2]), x.device)
            rt.check(_fn("conv_wgrad")(rt.ptr(x), rt.ptr(dy), rt.ptr(dw), B, Di, Hi, Wi, Ci, Ci, Do, Ho, Wo, Co, Co, k[0], k[1], k[2],
                                       pad[0], pad[1], pad[2], rt.ptr(ws), ws.numel(), rt.stream()))
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db, db_direct = _pgrad(ctx.bias_ref)
            ws = workspace(L.hupr_bn_ws_bytes(Co), dy.device)
            rt.check(_act("colsum", dy)(rt.ptr(dy), B * Do * Ho * Wo, Co, rt.ptr(db), rt.ptr(ws), ws.numel(), rt.stream()))
        dres = dy if ctx.has_res else None
        return dx, _pret(weight, dw, dw_direct), _pret(ctx.bias_ref, db, db_direct), dres, None, None, None


@_math_scoped
class DualConvFn(torch.autograd.Function):
    """Two bias-free "same" 3x3(x3) convolutions of one bf16-stored map (the main[0] / downsample[0] pair of a
    BasicBlock3D, reference models/layers.py:55-65) as one autograd node, so that the two input gradients are summed
    in the second kernel's residual epilogue instead of by a separate accumulation kernel."""

    @staticmethod
    def forward(ctx, x, w_a, w_b, pad, want_stats=False, infer=False):
        x = _c(x)
        k = _ksize(w_a)
        B, D, H, W, Ci = _vox(x)
        co = w_a.shape[0]
        assert w_b.shape == w_a.shape and _halo_ok(x, k, pad, co)
        y_a = _conv_raw(x, w_a, 0, None, None, co, k, pad, (D, H, W), stats=want_stats, infer=infer)
        y_b = _conv_raw(x, w_b, 0, None, None, co, k, pad, (D, H, W), stats=want_stats, infer=infer)
        ctx.save_for_backward(x, w_a, w_b)
        ctx.k, ctx.pad = k, pad
        return y_a, y_b

    @staticmethod
    def backward(ctx, dy_a, dy_b):
        x, w_a, w_b = ctx.saved_tensors
        dy = (_c(dy_a), _c(dy_b))
        k, pad = ctx.k, ctx.pad
        B, D, H, W, Ci = _vox(x)
        Co = w_a.shape[0]
        L = rt.lib()
        dx = None
        if ctx.needs_input_grad[0]:
            dpad = _dgrad_pad(k, pad)
            dx = _conv_raw(dy[0], w_a, 1, None, None, Ci, k, dpad, (D, H, W))
            dx = _conv_raw(dy[1], w_b, 1, None, dx, Ci, k, dpad, (D, H, W), out=dx)
        if (ctx.needs_input_grad[1] and ctx.needs_input_grad[2] and x.dtype == torch.bfloat16
                and L.hupr_conv3x3_wgrad_halo_dual_supported(B, D, H, W, Ci, Co, k[0])):
            # both weight gradients read the same x: one launch over 2 Co output channels, one reduction (same sums as two calls)
            (dwa, da), (dwb, db_) = _pgrad(w_a), _pgrad(w_b)
            ws = workspace(2 * L.hupr_conv3x3_wgrad_halo_ws_bytes(Ci, Co, k[0]), x.device)
            rt.check(L.hupr_conv3x3_wgrad_halo_bf16act_dual(rt.ptr(x), rt.ptr(dy[0]), rt.ptr(dy[1]), rt.ptr(dwa), rt.ptr(dwb), B, D, H, W,
                                                            Ci, Ci, Co, Co, k[0], rt.ptr(ws), ws.numel(), rt.stream()))
            return dx, _pret(w_a, dwa, da), _pret(w_b, dwb, db_), None, None, None
        grads = [_pret(w, *_halo_wgrad(x, g, w)) if need else None
                 for w, g, need in zip((w_a, w_b), dy, ctx.needs_input_grad[1:3])]
        return dx, grads[0], grads[1], None, None, None


def dual_conv(x, w_a, w_b, pad, stats=False):
    """(conv(x, w_a), conv(x, w_b)); fused input-gradient accumulation where the halo kernels apply."""
    k = _ksize(w_a)
    if w_a.shape == w_b.shape and _halo_ok(x, k, pad, w_a.shape[0]) and x.shape[-1] % 32 == 0 and w_a.shape[0] % 8 == 0:
        return DualConvFn.apply(x, w_a, w_b, tuple(pad), bool(stats), not torch.is_grad_enabled())
    infer = not torch.is_grad_enabled()
    return (ConvFn.apply(x, w_a, None, None, tuple(pad), bool(stats), infer),
            ConvFn.apply(x, w_b, None, None, tuple(pad), bool(stats), infer))


def conv(x, weight, bias=None, res=None, pad=(0, 0, 0), stats=False):
    """stats: a BatchNorm in training mode consumes the output next — let the convolution leave its column sums."""
    # (grad mode is read HERE: inside an autograd.Function's forward it is always off)
    return ConvFn.apply(x, weight, bias, res, tuple(pad), bool(stats), not torch.is_grad_enabled())


TMERGE_STREAM = True       # test aid: False = the generic mixed-storage convolution for the temporal merges


def _tmerge_fwd(x, weight, y):
    """merged map y (B,1,H,W,Co) fp32 of x (B,G,H,W,Ci): the LDS-DMA streaming kernel for bf16 64-channel maps (level 1),
    the generic mixed-storage convolution otherwise."""
    B, G, H, W, Ci = _vox(x)
    Co = weight.shape[0]
    L = rt.lib()
    if TMERGE_STREAM and x.dtype == torch.bfloat16 and L.hupr_tmerge_stream_supported(G, H * W, Ci, Co):
        rt.check(L.hupr_tmerge_fwd_stream_bf16(rt.ptr(x), rt.ptr(_packed(weight, 0, 1)), rt.ptr(y), B, G, H * W, Ci, Co, rt.stream()))
        return
    rt.check(L.hupr_conv_fwd_bf16_mixed(rt.ptr(x), int(x.dtype == torch.bfloat16), rt.ptr(_packed(weight, 0, 0)), None, rt.ptr(y), 0,
                                        B, G, H, W, Ci, Ci, 1, H, W, Co, Co, G, 1, 1, 0, 0, 0, rt.stream()))


def _tmerge_dgrad(dy, weight, dx):
    """dx (B,G,H,W,Ci) of the merge from the merged map's gradient dy (B,1,H,W,Co) fp32."""
    B, G, H, W, Ci = _vox(dx)
    Co = weight.shape[0]
    L = rt.lib()
    if TMERGE_STREAM and dx.dtype == torch.bfloat16 and L.hupr_tmerge_stream_supported(G, H * W, Ci, Co):
        rt.check(L.hupr_tmerge_dgrad_stream_bf16(rt.ptr(dy), rt.ptr(_packed(weight, 1, 1)), rt.ptr(dx), B, G, H * W, Ci, Co, rt.stream()))
        return
    rt.check(L.hupr_tmerge_dgrad_bf16(rt.ptr(dy), rt.ptr(_packed(weight, 1, 0)), rt.ptr(dx), int(dx.dtype == torch.bfloat16), B, G,
                                      H * W, Ci, Co, rt.stream()))


def _tmerge_wgrad(x, dy, weight):
    """-> (dw in the parameter layout, written directly into the gradient sink?)."""
    B, G, H, W, Ci = _vox(x)
    Co = weight.shape[0]
    L = rt.lib()
    dw, direct = _pgrad(weight)
    if TMERGE_STREAM and x.dtype == torch.bfloat16 and L.hupr_tmerge_wgrad_stream_supported(G, H * W, Ci, Co):
        ws = workspace(L.hupr_tmerge_wgrad_stream_ws_bytes(B, G, H * W, Ci, Co), x.device)
        rt.check(L.hupr_tmerge_wgrad_stream_bf16(rt.ptr(x), rt.ptr(dy), rt.ptr(dw), B, G, H * W, Ci, Co, rt.ptr(ws), ws.numel(), rt.stream()))
        return dw, direct
    ws = workspace(L.hupr_conv_wgrad_ws_bytes(B, 1, H, W, Ci, Co, G, 1, 1), x.device)
    rt.check(L.hupr_conv_wgrad_bf16_mixed(rt.ptr(x), int(x.dtype == torch.bfloat16), rt.ptr(dy), rt.ptr(dw), B, G, H, W, Ci, Ci, 1,
                                          H, W, Co, Co, G, 1, 1, 0, 0, 0, rt.ptr(ws), ws.numel(), rt.stream()))
    return dw, direct


@_math_scoped
class TemporalMergeFn(torch.autograd.Function):
    """Frame-axis merge: Conv3d with kernel (G,1,1), no padding and no bias on a (B,G,H,W,C) map (the
    l1temporalMerge / l2temporalMerge / temporalMerge of the reference, models/layers.py:195-197,218-220), taking
    the bf16-stored feature maps of the bf16-activation encoder directly: bf16 in, fp32 merged map out; the
    input gradient (G*B batched GEMMs — every frame slice sees exactly one tap) is written as bf16."""

    @staticmethod
    def forward(ctx, x, weight):
        x = _c(x)
        B, G, H, W, Ci = _vox(x)
        Co = weight.shape[0]
        assert tuple(weight.shape[1:]) == (Ci, G, 1, 1), (weight.shape, x.shape)
        y = torch.empty((B, 1, H, W, Co), dtype=torch.float32, device=x.device)
        _tmerge_fwd(x, weight, y)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = _c(dy)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _tmerge_dgrad(dy, weight, dx)
        dw, direct = _tmerge_wgrad(x, dy, weight) if ctx.needs_input_grad[1] else (None, False)
        return dx, _pret(weight, dw, direct)


@_math_scoped
class MergeDownFn(torch.autograd.Function):
    """An encoder level map feeds TWO consumers (reference models/layers.py:212-217): its temporal merge and the next level's
    align_corners down-sampling.  As separate nodes autograd adds their two input gradients with a kernel of its own (three
    tensor passes over the largest activations of the network); as one node the merge's input gradient is written first and
    the resampling backward accumulates onto it (hupr_interp_linear_bwd_acc_*).  bf16-stored maps, bf16 math.
    -> (merged fp32 (B,1,H,W,Co), down-sampled bf16 (B, D', H', W', C))."""

    @staticmethod
    def forward(ctx, x, weight, size):
        x = _c(x)
        B, G, H, W, Ci = _vox(x)
        Co = weight.shape[0]
        assert tuple(weight.shape[1:]) == (Ci, G, 1, 1) and x.dtype == torch.bfloat16
        L = rt.lib()
        merged = torch.empty((B, 1, H, W, Co), dtype=torch.float32, device=x.device)
        _tmerge_fwd(x, weight, merged)
        Do, Ho, Wo = size
        down = torch.empty((B, Do, Ho, Wo, Ci), dtype=x.dtype, device=x.device)
        rt.check(L.hupr_interp_linear_fwd_bf16act(rt.ptr(x), rt.ptr(down), B, G, H, W, Do, Ho, Wo, Ci, Ci, Ci, rt.stream()))
        ctx.save_for_backward(x, weight)
        ctx.size = size
        return merged, down

    @staticmethod
    def backward(ctx, d_merged, d_down):
        x, weight = ctx.saved_tensors
        B, G, H, W, Ci = _vox(x)
        Do, Ho, Wo = ctx.size
        L = rt.lib()
        d_merged, d_down = _c(d_merged), _c(d_down)
        dx = torch.empty_like(x)
        _tmerge_dgrad(d_merged, weight, dx)
        rt.check(L.hupr_interp_linear_bwd_acc_bf16act(rt.ptr(d_down), rt.ptr(dx), B, G, H, W, Do, Ho, Wo, Ci, Ci, Ci, rt.stream()))
        dw, direct = _tmerge_wgrad(x, d_merged, weight) if ctx.needs_input_grad[1] else (None, False)
        return dx, _pret(weight, dw, direct), None


def merge_down_ok(x):
    return _st.math == "bf16" and x.dtype == torch.bfloat16 and x.is_cuda


def temporal_merge(x, weight):
    """(B,G,H,W,C) -> (B,1,H,W,Co) fp32.  bf16-stored maps go through the mixed-storage kernels (bf16 math only);
    fp32 maps through the generic convolution."""
    if x.dtype == torch.bfloat16:
        if _st.math != "bf16":
            raise rt.HuprError("bf16-stored activations need the bf16 math mode")
        return TemporalMergeFn.apply(x, weight)
    return ConvFn.apply(x, weight, None, None, (0, 0, 0))


# ----------------------------------------------------------------------------------------------
# BatchNorm (+ReLU), and the BasicBlock3D tail  relu(bn_a(x1) + bn_b(x2))
# ----------------------------------------------------------------------------------------------
def _bn_bump(bn):
    """A training-mode pass updated ``bn``'s running statistics: its num_batches_tracked is due."""
    if bn.running_mean is not None and bn.num_batches_tracked is not None:
        if BN_COUNTER_SINK is not None:
            BN_COUNTER_SINK.append(bn)          # the engine bumps all counters of a step with one launch
        else:
            bn.num_batches_tracked.add_(1)


def _bn_params(x, bn, training, need_bwd=True):
    """-> (scale, shift, save_mean, save_invstd) for one nn.BatchNorm3d-like parameter holder."""
    L = rt.lib()
    C = x.shape[-1]
    M = x.numel() // C
    scale, shift, mean, invstd = [torch.empty(C, dtype=torch.float32, device=x.device) for _ in range(4)]
    fused = _conv_stats.pop(x.data_ptr(), None)
    if fused is not None and not (training and fused[2] == M and fused[3] == C):
        fused = None
    if training:            # (the running statistics are null pointers where the module does not track them)
        if fused is not None:           # the producing convolution left the column sums: finalize only
            rt.check(L.hupr_bn_train_finalize_f32(
                rt.ptr(fused[0]), fused[1], M, C, rt.ptr(bn.weight), rt.ptr(bn.bias), rt.ptr(bn.running_mean), rt.ptr(bn.running_var),
                float(bn.momentum), float(bn.eps), rt.ptr(mean), rt.ptr(invstd), rt.ptr(scale), rt.ptr(shift), rt.stream()))
        else:
            ws = workspace(L.hupr_bn_ws_bytes(C), x.device)
            rt.check(_act("bn_train_stats", x)(
                rt.ptr(x), M, C, rt.ptr(bn.weight), rt.ptr(bn.bias), rt.ptr(bn.running_mean), rt.ptr(bn.running_var), float(bn.momentum),
                float(bn.eps), rt.ptr(mean), rt.ptr(invstd), rt.ptr(scale), rt.ptr(shift), rt.ptr(ws), ws.numel(), rt.stream()))
        _bn_bump(bn)
    else:
        rt.check(L.hupr_bn_eval_params_f32(rt.ptr(bn.weight), rt.ptr(bn.bias), rt.ptr(bn.running_mean), rt.ptr(bn.running_var),
                                           float(bn.eps), C, rt.ptr(scale), rt.ptr(shift), rt.stream()))
        if need_bwd:                         # only a backward pass through eval-mode statistics reads these two
            mean.copy_(bn.running_mean)
            invstd = torch.rsqrt(bn.running_var + bn.eps)
    return scale, shift, mean, invstd


def _bn_params_pair(x1, bn1, x2, bn2):
    """Training-mode coefficients of the two BatchNorms of a block tail when BOTH producing convolutions left their column sums:
    one finalize launch for the pair (hupr_bn_train_finalize2_f32).  None: not applicable — the caller takes them one by one."""
    f1, f2 = _conv_stats.get(x1.data_ptr()), _conv_stats.get(x2.data_ptr())
    C = x1.shape[-1]
    M = x1.numel() // C
    if (f1 is None or f2 is None or x1.shape != x2.shape or x1.data_ptr() == x2.data_ptr()
            or (f1[2], f1[3]) != (M, C) or (f2[2], f2[3]) != (M, C)):
        return None
    _conv_stats.pop(x1.data_ptr())
    _conv_stats.pop(x2.data_ptr())
    dev = x1.device
    out = [[torch.empty(C, dtype=torch.float32, device=dev) for _ in range(4)] for _ in range(2)]      # scale, shift, mean, invstd
    args = []
    for f, bn, (scale, shift, mean, invstd) in ((f1, bn1, out[0]), (f2, bn2, out[1])):
        args += [rt.ptr(f[0]), f[1], rt.ptr(bn.weight), rt.ptr(bn.bias), rt.ptr(bn.running_mean), rt.ptr(bn.running_var),
                 float(bn.momentum), float(bn.eps), rt.ptr(mean), rt.ptr(invstd), rt.ptr(scale), rt.ptr(shift)]
        _bn_bump(bn)
    rt.check(rt.lib().hupr_bn_train_finalize2_f32(*args, M, C, rt.stream()))
    return tuple(out[0]), tuple(out[1])


def _bn_bwd(dy, x, mean, invstd, gamma, training, beta=None, fwd=None):
    """-> (dx, dgamma, dbeta) as backward() return values (None for parameters written through the gradient sink).
    fwd = (scale, shift) of the forward pass of a BatchNorm + ReLU: the ReLU mask is recomputed from x (the very expression the
    forward evaluated) instead of read back as a third tensor; None: no ReLU."""
    L = rt.lib()
    C = x.shape[-1]
    M = x.numel() // C
    dx = torch.empty_like(x)
    dg, dg_direct = _pgrad(gamma)
    db, db_direct = _pgrad(beta) if beta is not None else (torch.empty_like(gamma), False)
    ws = workspace(L.hupr_bn_ws_bytes(C), x.device)
    assert dy.dtype == x.dtype
    if fwd is not None:
        rt.check(_act("bn_bwd_remask", x)(rt.ptr(dy), rt.ptr(fwd[0]), rt.ptr(fwd[1]), rt.ptr(x), rt.ptr(mean), rt.ptr(invstd),
                                          rt.ptr(gamma), rt.ptr(dx), rt.ptr(dg), rt.ptr(db), M, C, 1 if training else 0,
                                          rt.ptr(ws), ws.numel(), rt.stream()))
    else:
        rt.check(_act("bn_bwd", x)(rt.ptr(dy), None, rt.ptr(x), rt.ptr(mean),
                                   rt.ptr(invstd), rt.ptr(gamma), rt.ptr(dx), rt.ptr(dg), rt.ptr(db), M, C,
                                   1 if training else 0, rt.ptr(ws), ws.numel(), rt.stream()))
    return dx, _pret(gamma, dg, dg_direct), _pret(beta, db, db_direct)


def _bn_eval_act(x1, bn1, relu, x2=None, bn2=None):
    """Inference: y = [relu](bn1(x1) [+ bn2(x2)]) on running statistics, coefficients and apply in one launch."""
    assert x2 is None or x1.dtype == x2.dtype
    C = x1.shape[-1]
    y = torch.empty_like(x1)
    rt.check(_act("bn_eval_act", x1)(rt.ptr(x1), *_bn_eval_args(bn1), rt.ptr(x2), *_bn_eval_args(bn2), rt.ptr(y), x1.numel() // C, C,
                                     1 if relu else 0, rt.stream()))
    return y


def _scale_shift_act(x1, s1, t1, relu, x2=None, s2=None, t2=None):
    """y = [relu](s1 x1 + t1 [+ s2 x2 + t2]) with per-channel coefficients."""
    assert x2 is None or x1.dtype == x2.dtype
    C = x1.shape[-1]
    y = torch.empty_like(x1)
    rt.check(_act("scale_shift_act", x1)(rt.ptr(x1), rt.ptr(s1), rt.ptr(t1), rt.ptr(x2), rt.ptr(s2), rt.ptr(t2), rt.ptr(y),
                                         x1.numel() // C, C, 1 if relu else 0, rt.stream()))
    return y


@_math_scoped
class BNActFn(torch.autograd.Function):
    """y = [relu](batch_norm(x)).  ``bn`` is the parameter holder (running stats updated in place)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bn, training, relu, no_bwd=False):
        # no_bwd: the caller runs under torch.no_grad() (grad mode is always off in here, and needs_input_grad reflects the
        # tensors' flags whatever the mode) — eval-mode statistics then skip what only a backward pass reads
        x = _c(x)
        if no_bwd and not training:
            return _bn_eval_act(x, bn, relu)
        scale, shift, mean, invstd = _bn_params(x, bn, training, not no_bwd)
        y = _scale_shift_act(x, scale, shift, relu)
        ctx.save_for_backward(x, mean, invstd, gamma, scale if relu else None, shift if relu else None)
        ctx.beta_ref = beta
        ctx.training = training
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, invstd, gamma, scale, shift = ctx.saved_tensors
        dx, dg, db = _bn_bwd(_c(dy), x, mean, invstd, gamma, ctx.training, ctx.beta_ref,
                             fwd=(scale, shift) if scale is not None else None)
        return dx, dg, db, None, None, None, None


@_math_scoped
class BNAddBNReLUFn(torch.autograd.Function):
    """y = relu(bn_a(x1) + bn_b(x2)) — the tail of BasicBlock3D.forward (models/layers.py:66-70)."""

    @staticmethod
    def forward(ctx, x1, g1, b1, bn1, x2, g2, b2, bn2, training, no_bwd=False):
        x1, x2 = _c(x1), _c(x2)
        if no_bwd and not training:
            return _bn_eval_act(x1, bn1, True, x2, bn2)
        pair = _bn_params_pair(x1, bn1, x2, bn2) if training else None
        if pair is not None:
            (s1, t1, m1, i1), (s2, t2, m2, i2) = pair
        else:
            s1, t1, m1, i1 = _bn_params(x1, bn1, training, not no_bwd)
            s2, t2, m2, i2 = _bn_params(x2, bn2, training, not no_bwd)
        y = _scale_shift_act(x1, s1, t1, True, x2, s2, t2)
        ctx.save_for_backward(x1, x2, m1, i1, g1, m2, i2, g2, s1, t1, s2, t2)
        ctx.beta_refs = (b1, b2)
        ctx.training = training
        return y

    @staticmethod
    def backward(ctx, dy):
        x1, x2, m1, i1, g1, m2, i2, g2, s1, t1, s2, t2 = ctx.saved_tensors
        dy = _c(dy)
        # both branches share dy and the ReLU mask: one statistics pass + one apply pass for the pair
        L = rt.lib()
        C = x1.shape[-1]
        M = x1.numel() // C
        assert dy.dtype == x1.dtype == x2.dtype
        dx1, dx2 = torch.empty_like(x1), torch.empty_like(x2)
        b1, b2 = ctx.beta_refs
        (dg1, dg1_d), (db1, db1_d), (dg2, dg2_d), (db2, db2_d) = _pgrad(g1), _pgrad(b1), _pgrad(g2), _pgrad(b2)
        ws = workspace(L.hupr_bn_ws_bytes(C), x1.device)
        # ReLU mask recomputed from x1, x2 and the forward coefficients
        rt.check(_act("bn_bwd2_remask", x1)(rt.ptr(dy), rt.ptr(x1), rt.ptr(s1), rt.ptr(t1), rt.ptr(m1), rt.ptr(i1), rt.ptr(g1),
                                            rt.ptr(x2), rt.ptr(s2), rt.ptr(t2), rt.ptr(m2), rt.ptr(i2), rt.ptr(g2), rt.ptr(dx1),
                                            rt.ptr(dx2), rt.ptr(dg1), rt.ptr(db1), rt.ptr(dg2), rt.ptr(db2), M, C,
                                            1 if ctx.training else 0, rt.ptr(ws), ws.numel(), rt.stream()))
        return (dx1, _pret(g1, dg1, dg1_d), _pret(b1, db1, db1_d), None, dx2, _pret(g2, dg2, dg2_d), _pret(b2, db2, db2_d),
                None, None, None)


@_math_scoped
class PReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, alpha):
        x = _c(x)
        y = torch.empty_like(x)
        rt.check(_act("prelu_fwd", x)(rt.ptr(x), rt.ptr(alpha), rt.ptr(y), x.numel(), rt.stream()))
        ctx.save_for_backward(x, alpha)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, alpha = ctx.saved_tensors
        L = rt.lib()
        dx = torch.empty_like(x)
        da, da_direct = _pgrad(alpha)
        dy = _c(dy)
        assert dy.dtype == x.dtype
        if da_direct and PRELU_DEFER and getattr(GRAD_SINK, "can_defer", None) is not None and GRAD_SINK.can_defer(x.device):
            # the slope gradient's final sum waits until its gradient bucket is complete: the twelve of a step then take one launch
            part = torch.empty(L.hupr_prelu_ws_bytes() // 8, dtype=torch.float64, device=x.device)
            npart = ctypes.c_int(0)
            rt.check(_act("prelu_bwd_partials", x)(rt.ptr(dy), rt.ptr(x), rt.ptr(alpha), rt.ptr(dx), x.numel(), rt.ptr(part),
                                                   part.numel() * 8, ctypes.byref(npart), rt.stream()))
            GRAD_SINK.defer_sum(alpha, part, npart.value, da)
            return dx, None
        ws = workspace(L.hupr_prelu_ws_bytes(), x.device)
        rt.check(_act("prelu_bwd", x)(rt.ptr(dy), rt.ptr(x), rt.ptr(alpha), rt.ptr(dx), rt.ptr(da), x.numel(),
                                      rt.ptr(ws), ws.numel(), rt.stream()))
        return dx, _pret(alpha, da, da_direct)


# ----------------------------------------------------------------------------------------------
@_math_scoped
class MNetFn(torch.autograd.Function):
    """x (B,G,F,2,R,A,E) — or its elevation mean as planes (B,G,16,R,A) — -> (B, G, R, A, 32) channels-last, depth = group frame."""

    @staticmethod
    def forward(ctx, x, weight, bias, out_dtype=torch.float32):
        x = _c(x)
        if weight.shape != (32, 2, 2, 1, 1):
            raise ValueError("MNet kernel is specialised for F=8, 2 (re/im), E=8, 32 filters")
        from_means = x.dim() == 5            # (B, G, 16, R, A): the fused loader's elevation-mean planes (fft_chain_loader_means)
        if from_means:
            B, G, P16, R, A = x.shape
            if P16 != 16:
                raise ValueError("elevation-mean input must be (B, G, 16, R, A)")
        else:
            B, G, F, two, R, A, E = x.shape
            if (F, two, E) != (8, 2, 8):
                raise ValueError("MNet kernel is specialised for F=8, 2 (re/im), E=8, 32 filters")
        out = torch.empty((B, G, R, A, 32), dtype=out_dtype, device=x.device)
        # training: keep the 16 elevation means per pixel (1/8 of x) — the backward pass recomputes everything from them
        need = weight.requires_grad or bias.requires_grad
        means = torch.empty((B * G, R * A, 16), dtype=torch.float32, device=x.device) if need else None
        rt.check(_act("mnet_fwd_means" if from_means else "mnet_fwd", out)(
            rt.ptr(x), rt.ptr(_c(weight)), rt.ptr(bias), rt.ptr(out), rt.ptr(means), B * G, R * A, rt.stream()))
        ctx.save_for_backward(means, weight, bias)
        ctx.geom = (B, G, R, A)
        return out

    @staticmethod
    def backward(ctx, dy):
        means, weight, bias = ctx.saved_tensors
        L = rt.lib()
        B, G, R, A = ctx.geom
        dw, dw_direct = _pgrad(weight)
        db, db_direct = _pgrad(bias)
        ws = workspace(L.hupr_mnet_bwd_ws_bytes(), dy.device)
        dy = _c(dy)
        rt.check(_act("mnet_bwd", dy)(None, rt.ptr(means), rt.ptr(_c(weight)), rt.ptr(bias), rt.ptr(dy), rt.ptr(dw), rt.ptr(db),
                                      B * G, R * A, rt.ptr(ws), ws.numel(), rt.stream()))
        return None, _pret(weight, dw, dw_direct), _pret(bias, db, db_direct), None


def _ld_view_ok(t, C):
    """``t`` (B, D, H, W, C) is a channel slice of a wider contiguous channels-last tensor (row stride = t.stride(3) elements, dense
    voxel order): kernels with a leading-dimension argument read / write it in place."""
    B, D, H, W, _ = t.shape
    ld = t.stride(3)
    return (t.stride(4) == 1 and ld >= C and t.stride(2) == W * ld and t.stride(1) == H * W * ld
            and (B == 1 or t.stride(0) == D * H * W * ld) and t.data_ptr() % 16 == 0 and ld % 8 == 0)


@_math_scoped
class InterpFn(torch.autograd.Function):
    """align_corners=True linear resampling of a channels-last (B,D,H,W,C) tensor to ``size``.  ``out`` (optional): a channel
    slice of a wider channels-last buffer to write into (the decoder's concatenated input: no concatenation copy); the incoming
    gradient may be such a slice too and is read in place."""

    @staticmethod
    def forward(ctx, x, size):
        x = _c(x)
        B, Di, Hi, Wi, C = _vox(x)
        Do, Ho, Wo = size
        out = _interp_out.pop("out", None)           # (a side channel, not an argument: an argument returned as the output would be an
        if out is None:                               # input alias in autograd's eyes)
            y, ld = torch.empty((B, Do, Ho, Wo, C), dtype=x.dtype, device=x.device), C
        else:
            assert tuple(out.shape) == (B, Do, Ho, Wo, C) and out.dtype == x.dtype and _ld_view_ok(out, C), (out.shape, out.stride())
            y, ld = out, out.stride(3)
        rt.check(_act("interp_linear_fwd", x)(rt.ptr(x), rt.ptr_ld(y), B, Di, Hi, Wi, Do, Ho, Wo, C, C, ld, rt.stream()))
        ctx.in_shape = (B, Di, Hi, Wi, C)
        ctx.size = size
        return y

    @staticmethod
    def backward(ctx, dy):
        B, Di, Hi, Wi, C = ctx.in_shape
        Do, Ho, Wo = ctx.size
        if dy.is_contiguous() or not _ld_view_ok(dy, C):
            dy, ld = _c(dy), C
        else:
            ld = dy.stride(3)
        dx = torch.empty(ctx.in_shape, dtype=dy.dtype, device=dy.device)
        rt.check(_act("interp_linear_bwd", dy)(rt.ptr_ld(dy), rt.ptr(dx), B, Di, Hi, Wi, Do, Ho, Wo, C, C, ld, rt.stream()))
        return dx, None


class JoinFn(torch.autograd.Function):
    """The decoder's channel concatenation (reference models/layers.py:166-178) without a copy: the parts were WRITTEN as adjacent
    channel slices of ``wide`` by their producers (InterpFn / MSCSALevelFn with an output placement), so the forward just hands
    ``wide`` on, and the backward hands each producer its slice of the gradient (views; the producers' backward kernels read them in
    place)."""

    @staticmethod
    def forward(ctx, wide, *parts):
        off = 0
        for t in parts:
            assert t.data_ptr() == wide.data_ptr() + off * wide.element_size() and t.stride(3) == wide.shape[-1], "parts must be slices of wide"
            off += t.shape[-1]
        assert off == wide.shape[-1]
        ctx.widths = [t.shape[-1] for t in parts]
        return wide.view(wide.shape)

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        outs, off = [], 0
        for w in ctx.widths:
            outs.append(g[..., off:off + w])
            off += w
        return (None,) + tuple(outs)


_interp_out = {}


def interp(x, size, out=None):
    """out: optional output placement (see InterpFn)."""
    _interp_out.clear()
    if out is not None:
        _interp_out["out"] = out
    return InterpFn.apply(x, tuple(size))


def _cast(x, dtype):
    x = _c(x)
    if x.dtype == dtype:
        return x
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    fn = rt.lib().hupr_cast_f32_to_bf16 if dtype == torch.bfloat16 else rt.lib().hupr_cast_bf16_to_f32
    rt.check(fn(rt.ptr(x), rt.ptr(y), x.numel(), rt.stream()))
    return y


@_math_scoped
class CastFn(torch.autograd.Function):
    """Boundary of the bf16-activation region: y = x in ``dtype``; the gradient comes back in x's dtype."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.in_dtype = x.dtype
        return _cast(x, dtype)

    @staticmethod
    def backward(ctx, dy):
        return _cast(dy, ctx.in_dtype), None


def cast(x, dtype):
    return x if x.dtype == dtype else CastFn.apply(x, dtype)


def to_act(x, decoder=False):
    """Region border: ``x`` in the activation storage type of the current mode (bf16 inside bf16-activation regions)."""
    want = torch.bfloat16 if (act_bf16() and (ACT_BF16_DECODER or not decoder)) else torch.float32
    return cast(x, want)


# ----------------------------------------------------------------------------------------------
def gemm(ta, tb, A, B, M, N, K, lda, ldb, batch, a_bs, b_bs, out=None, res=None, accumulate=False, math=None):
    """Batched row-major fp32 GEMM on raw strides; returns C (batch, M, N) dense.  ``math`` overrides the global matrix-pipe
    mode for this call ("f32" keeps an operator on the exact fp32 pipe inside a bf16 run)."""
    if out is None:
        out = torch.empty((batch, M, N), dtype=torch.float32, device=A.device)
    fn = _fn("gemm") if math is None else getattr(rt.lib(), "hupr_gemm_%s" % math)
    rt.check(fn(ta, tb, rt.ptr(A), rt.ptr(B), rt.ptr(out), M, N, K, lda, ldb, N, batch, a_bs, b_bs, M * N, rt.ptr(res), N,
                M * N if res is not None else 0, 1 if accumulate else 0, rt.stream()))
    return out


def _attn_ws(B, N, C, device):
    """Workspace of the split-key forward (small batches: the plain grid would leave most CUs idle), or None."""
    nbytes = rt.lib().hupr_attn_fwd_split_ws_bytes(B, N, C)
    return workspace(nbytes, device) if nbytes else None


# The GEMM / row-softmax attention core, shared by AttentionFn (``dense``: K, Q, dK, dQ are (B, N, C) tensors; ``fn`` follows the math
# mode) and MSCSALevelFn (column blocks of the (B, N, 4C) projections and of their gradient; always the bf16 pipe).  kp / qp / dkp / dqp / g
# are raw pointers, the rest dense fp32 tensors.  (``nl``: the ignored leading dimension beside a NULL residual, as each caller spells it.)
def _attn_gemm_fwd(fn, dense, kp, qp, v, vres, P, out, B, N, C):
    """P[q][j] = Q[q] . K[j], softmax over the keys j (a row softmax), out = P V (+ vres)."""
    ld, nl = (C, 1) if dense else (4 * C, 0)
    rt.check(fn(0, 1, qp, kp, rt.ptr(P), N, N, C, ld, ld, N, B, N * ld, N * ld, N * N, None, nl * N, 0, 0, rt.stream()))
    rt.check(rt.lib().hupr_softmax_rows_f32(rt.ptr(P), B * N, N, rt.stream()))
    rt.check(fn(0, 0, rt.ptr(P), rt.ptr(v), rt.ptr(out), N, C, N, N, C, C, B, N * N, N * C, N * C, rt.ptr(vres), C,
                N * C if vres is not None else 0, 0, rt.stream()))


def _attn_gemm_bwd(fn, dense, kp, qp, v, P, g, residual, accumulate, dv, dS, dkp, dqp, B, N, C):
    """Backward of ``_attn_gemm_fwd`` from the output gradient at ``g``; dS (B, N, N) is scratch."""
    ld, nl = (C, 1) if dense else (4 * C, 0)
    # dV[j] = sum_q P[q][j] dout[q]  (+ dout: residual form; ``accumulate``: added onto the dV already there)
    rt.check(fn(1, 0, rt.ptr(P), g, rt.ptr(dv), N, C, N, N, C, C, B, N * N, N * C, N * C, g if residual else None, C,
                N * C if residual else 0, 1 if accumulate else 0, rt.stream()))
    # dP[q][j] = dout[q] . V[j]; dS = softmax backward in place
    rt.check(fn(0, 1, g, rt.ptr(v), rt.ptr(dS), N, N, C, C, C, N, B, N * C, N * C, N * N, None, nl * N, 0, 0, rt.stream()))
    rt.check(rt.lib().hupr_softmax_rows_bwd_f32(rt.ptr(P), rt.ptr(dS), B * N, N, rt.stream()))
    # dQ[q] = sum_j dS[q][j] K[j];  dK[j] = sum_q dS[q][j] Q[q]
    rt.check(fn(0, 0, rt.ptr(dS), kp, dqp, N, C, N, N, ld, ld, B, N * N, N * ld, N * ld, None, nl * C, 0, 0, rt.stream()))
    rt.check(fn(1, 0, rt.ptr(dS), qp, dkp, N, C, N, N, ld, ld, B, N * N, N * ld, N * ld, None, nl * C, 0, 0, rt.stream()))


@_math_scoped
class AttentionFn(torch.autograd.Function):
    """MSCSA attention (models/layers.py:126-133) on token-major tensors (B, N, C):
    S[j,k] = sum_c K[j,c] Q[k,c];  P = softmax over keys j;  out[k,c] = sum_j P[j,k] V[j,c] (+ V[k,c])."""

    @staticmethod
    def forward(ctx, k, q, v, residual):
        k, q, v = _c(k), _c(q), _c(v)
        B, N, C = v.shape
        L = rt.lib()
        ctx.flash = _st.math == "bf16" and USE_FLASH and bool(L.hupr_attn_flash_supported(N, C))
        ctx.residual = residual
        if ctx.flash:
            out = torch.empty_like(v)
            lse = torch.empty((B, N), dtype=torch.float32, device=v.device)
            # bf16 copies of the MFMA operands: each is re-read by every workgroup (N / 128 times), and the kernels
            # would round them to bf16 per tile anyway — same bits, half the traffic, also half the saved activations
            kb, qb, vb = _cast(k, torch.bfloat16), _cast(q, torch.bfloat16), _cast(v, torch.bfloat16)
            ws = _attn_ws(B, N, C, v.device)
            rt.check(L.hupr_attn_fwd_bf16in_ld_ws(rt.ptr(kb), C, rt.ptr(qb), C, rt.ptr(vb), rt.ptr(v) if residual else None,
                                                  rt.ptr(out), rt.ptr(lse), None, 0, B, N, C, *_ws_args(ws), rt.stream()))
            ctx.save_for_backward(kb, qb, vb, v, out, lse)
            return out
        P = torch.empty((B, N, N), dtype=torch.float32, device=v.device)
        out = torch.empty((B, N, C), dtype=torch.float32, device=v.device)
        _attn_gemm_fwd(_fn("gemm"), True, rt.ptr(k), rt.ptr(q), v, v if residual else None, P, out, B, N, C)
        ctx.save_for_backward(k, q, v, P)
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = _c(dout)
        if ctx.flash:
            kb, qb, vb, v, out, lse = ctx.saved_tensors
            B, N, C = v.shape
            dk, dq, dv = torch.empty_like(v), torch.empty_like(v), torch.empty_like(v)
            dq_scr = torch.empty((B, N), dtype=torch.float32, device=v.device)
            gb = _cast(dout, torch.bfloat16)
            rt.check(rt.lib().hupr_attn_bwd_bf16in(rt.ptr(kb), rt.ptr(qb), rt.ptr(vb), rt.ptr(gb), rt.ptr(v), rt.ptr(out), rt.ptr(dout),
                                                  rt.ptr(lse), rt.ptr(dk), rt.ptr(dq), rt.ptr(dv), rt.ptr(dq_scr), B, N, C,
                                                  1 if ctx.residual else 0, rt.stream()))
            return dk, dq, dv, None
        k, q, v, P = ctx.saved_tensors
        B, N, C = v.shape
        dv, dS, dq, dk = [torch.empty(s, dtype=torch.float32, device=v.device) for s in ((B, N, C), (B, N, N), (B, N, C), (B, N, C))]
        _attn_gemm_bwd(_fn("gemm"), True, rt.ptr(k), rt.ptr(q), v, P, rt.ptr(dout), ctx.residual, False, dv, dS, rt.ptr(dk), rt.ptr(dq),
                       B, N, C)
        return dk, dq, dv, None


_level_cat_out = {}      # {"out": view}: where the NEXT fused level writes its concatenated bf16 output (models/layers.py sets it)
CAT_FUSION = True          # fused levels return their maps concatenated as bf16
PROJ_STREAM = True         # test aid: False = the level's projections through the generic implicit-GEMM engine
CAT_INPLACE = True         # test aid: False = concatenation copies per decoder stage
ATTN_BATCH = True          # test aid: False = one launch pair per attention in single-sample inference


def mscsa_level_fused_ok(ra):
    """One MSCSA level can run as MSCSALevelFn (bf16 math; any (N, C) — shapes without a fused attention kernel keep the
    GEMM / row-softmax attention core inside the node)."""
    return _st.math == "bf16" and ra.dtype == torch.float32 and ra.shape[-1] % 8 == 0


def level_cat_placement_ok(ra):
    """The fused level node of map ``ra`` returns ONE concatenated bf16 tensor and can write it into a slice of a wider buffer."""
    B, _, H, W, C = ra.shape
    return CAT_INPLACE and mscsa_level_fused_ok(ra) and USE_FLASH and CAT_FUSION and bool(rt.lib().hupr_attn_flash_supported(H * W, C))


def _level_blocks(Y, C):
    """[(K pointer, Q pointer)] of the four attentions: column blocks (width C) of the two (B, N, 4C) tensors ``Y`` — the projections, or
    their gradient (dK / dQ).  The one place that does this arithmetic."""
    step = C * Y[0].element_size()
    return [(Y[ks].data_ptr() + kslot * step, Y[qs].data_ptr() + qslot * step) for ks, kslot, qs, qslot, _, _ in MSCSALevelFn.SPEC]


def _level_project(x, wc, y, flash):
    """The four projections of map ``x`` (B,1,H,W,C) fp32 as one product with wc (4C, C) -> y (B, N, 4C), bf16 for the fused
    attention kernels (``flash``), else fp32.  (A 1x1 kernel's packed layout IS the parameter layout (Co, Ci).)"""
    B, _, H, W, C = x.shape
    L = rt.lib()
    if flash and PROJ_STREAM and L.hupr_mscsa_proj_supported(B * H * W, C):
        # one HBM-bound streaming product (csrc/projection.hip)
        rt.check(L.hupr_mscsa_proj_fwd_bf16(rt.ptr(x), rt.ptr(wc), rt.ptr(y), B * H * W, C, rt.stream()))
        return
    rt.check(L.hupr_conv_fwd_bf16_mixed(rt.ptr(x), 0, rt.ptr(wc), None, rt.ptr(y), 1 if flash else 0, B, 1, H, W, C, C,
                                        1, H, W, 4 * C, 4 * C, 1, 1, 1, 0, 0, 0, rt.stream()))


def _level_fwd_flash(tab, ld16, qscaled, infer, B, N, C, dev):
    """The four attentions on the fused kernels.  ``tab`` rows: (K ptr, Q ptr, V bf16, V residual fp32 | None, out, log-sum-exp,
    bf16 cat slice ptr | None)."""
    L = rt.lib()
    # single-sample inference (config C2): the four attentions of the level as ONE split launch + ONE merge launch instead of eight
    split_ws = L.hupr_attn_fwd_split_ws_bytes(B, N, C)       # (> 0: the key-split form applies to this batch)
    split_bytes = split_ws if (infer and ATTN_BATCH) else 0
    # training batches, levels 2 and 3 (C = 128 / 256: one attention's grid is 256 / 64 workgroups): the four as ONE launch of the
    # one-pass kernel (not where the single-sample split form applies: its shares round differently)
    if split_bytes or (ATTN_LEVEL_BATCH and not split_ws and C != 64):
        items = (rt.AttnItem * 4)()
        for it, (kp, qp, v16, vres, out, lse, out16) in zip(items, tab):
            it.K, it.Q, it.V, it.Vres = kp, qp, rt.ptr(v16), rt.ptr(vres)
            it.out, it.lse, it.out16 = rt.ptr(out), rt.ptr(lse), out16
        ws = workspace(4 * split_bytes, dev) if split_bytes else None
        fwd = L.hupr_attn_fwd_bf16in_ld_ws_batch_qs if qscaled else L.hupr_attn_fwd_bf16in_ld_ws_batch
        rt.check(fwd(items, 4, 4 * C, 4 * C, ld16, B, N, C, *_ws_args(ws), rt.stream()))
        return
    fwd = L.hupr_attn_fwd_bf16in_ld_ws_qs if qscaled else L.hupr_attn_fwd_bf16in_ld_ws
    for kp, qp, v16, vres, out, lse, out16 in tab:
        ws = _attn_ws(B, N, C, dev)
        ev = _probe_begin(ATTN_PROBE, "fwd", B, N, C)
        rt.check(fwd(kp, 4 * C, qp, 4 * C, rt.ptr(v16), rt.ptr(vres), rt.ptr(out), rt.ptr(lse), out16, ld16, B, N, C, *_ws_args(ws),
                     rt.stream()))
        _probe_end(ev)


def _level_bwd_flash(tab, dcat, ld, douts, qscaled, scr, B, N, C):
    """Backward of ``_level_fwd_flash``.  ``tab`` rows: (K ptr, Q ptr, V bf16, V fp32, out, log-sum-exp, dK ptr, dQ ptr, dV, residual);
    the output gradients are the four column blocks of ``dcat`` (bf16, row stride ``ld``) or, without it, the fp32 ``douts``."""
    L = rt.lib()
    if dcat is not None and ATTN_LEVEL_BATCH:
        # row sums and dQ of the four attentions in one launch each; dK / dV: levels 2 and 3 in two launches of two (the residual
        # attentions of the two maps, then the two that add onto their dV) — 4 launches instead of 12, grids four / two times as
        # large; level 1 one launch per attention (12 -> 6 launches)
        scr4 = torch.empty((4, B, N), dtype=torch.float32, device=dcat.device)
        items = (rt.AttnBwdItem * 4)()
        for i, (it, (kp, qp, v16, v32, out, lse, dkp, dqp, dv, residual)) in enumerate(zip(items, tab)):
            it.K, it.Q, it.V, it.dO = kp, qp, rt.ptr(v16), dcat.data_ptr() + i * C * 2
            it.V32, it.out, it.lse = rt.ptr(v32), rt.ptr(out), rt.ptr(lse)
            it.dK, it.dQ, it.dV, it.Dq = dkp, dqp, rt.ptr(dv), scr4.data_ptr() + i * B * N * 4
            it.residual, it.accumulate = (1, 0) if residual else (0, 1)
        bwd = L.hupr_attn_bwd_bf16in_ld_batch_qs if qscaled else L.hupr_attn_bwd_bf16in_ld_batch
        ev = _probe_begin(ATTN_PROBE, "bwd_level", B, N, C)
        rt.check(bwd(items, 4, 4 * C, 4 * C, ld, 4 * C, 4 * C, B, N, C, rt.stream()))
        _probe_end(ev)
        return
    bwd = L.hupr_attn_bwd_bf16in_ld_qs if qscaled else L.hupr_attn_bwd_bf16in_ld
    for i, ((kp, qp, v16, v32, out, lse, dkp, dqp, dv, residual), dout) in enumerate(zip(tab, douts)):
        if dcat is not None:
            gp, ldg, g32 = dcat.data_ptr() + i * C * 2, ld, None
        else:
            dout = _c(dout)
            gb = _cast(dout, torch.bfloat16)
            gp, ldg, g32 = rt.ptr(gb), C, rt.ptr(dout)
        ev = _probe_begin(ATTN_PROBE, "bwd", B, N, C)
        rt.check(bwd(kp, 4 * C, qp, 4 * C, rt.ptr(v16), gp, ldg, rt.ptr(v32), rt.ptr(out), g32, rt.ptr(lse), dkp, 4 * C, dqp, 4 * C,
                     rt.ptr(dv), rt.ptr(scr), B, N, C, 1 if residual else 0, 0 if residual else 1, rt.stream()))
        _probe_end(ev)


def _level_map_grads(need, maps, dY, Wc, dV):
    """Gradients of the two maps: dY . Wc (K = 4C) with the map's accumulated dV as the residual term."""
    B, _, H, W, C = maps[0].shape
    L = rt.lib()
    grads = [None, None]
    for i in range(2):
        if not need[i]:
            continue
        dx = grads[i] = torch.empty_like(maps[i])
        if PROJ_STREAM and L.hupr_mscsa_proj_dgrad_supported(B * H * W, C):
            rt.check(L.hupr_mscsa_proj_dgrad_f32(rt.ptr(dY[i]), rt.ptr(Wc[i]), rt.ptr(dV[i]), rt.ptr(dx), B * H * W, C, rt.stream()))
        else:
            rt.check(L.hupr_gemm_bf16(0, 0, rt.ptr(dY[i]), rt.ptr(Wc[i]), rt.ptr(dx), B * H * W, C, 4 * C, 4 * C, C, C, 1, 0, 0, 0,
                                      rt.ptr(dV[i]), C, 0, 0, rt.stream()))
    return grads


def _level_weight_grads(need, weights, maps, dY):
    """The eight projection weight gradients as backward() return values: per map one split-K product maps[i]^T dY[i] -> (4C, C), landed
    in the four parameters' gradients.  ``need``: needs_input_grad of the eight weights."""
    B, _, H, W, C = maps[0].shape
    L = rt.lib()
    wgrads = [None] * 8
    dsts, srcs, landed = [], [], []
    for i in range(2):
        if not any(need[4 * i:4 * i + 4]):
            continue
        ws4 = weights[4 * i:4 * i + 4]
        got = [_pgrad(w) if need[4 * i + j] else (None, False) for j, w in enumerate(ws4)]
        # the four gradient slots adjacent in their flat bucket, in this order (HuPRNet.gradient_groups -> GradientBuckets): the
        # GEMM writes them in place — no (4C, C) temporary, no copy launch
        inplace = all(g is not None and d for g, d in got) and all(
            got[j][0].is_contiguous() and got[j][0].data_ptr() == got[0][0].data_ptr() + j * C * C * 4 for j in range(4))
        dWc = None if inplace else torch.empty((4 * C, C), dtype=torch.float32, device=maps[i].device)
        ws = workspace(L.hupr_conv_wgrad_ws_bytes(B, 1, H, W, C, 4 * C, 1, 1, 1), maps[i].device)
        rt.check(L.hupr_conv_wgrad_bf16(rt.ptr(maps[i]), rt.ptr(dY[i]), got[0][0].data_ptr() if inplace else rt.ptr(dWc), B, 1, H, W, C, C,
                                        1, H, W, 4 * C, 4 * C, 1, 1, 1, 0, 0, 0, rt.ptr(ws), ws.numel(), rt.stream()))
        for j, (w, (g, direct)) in enumerate(zip(ws4, got)):
            if need[4 * i + j]:
                if not inplace:
                    dsts.append(g)
                    srcs.append(dWc[j * C:(j + 1) * C].view_as(w))
                landed.append((4 * i + j, w, g, direct))
    if dsts:
        torch._foreach_copy_(dsts, srcs)        # the eight row blocks of the two fused gradients in one launch
    for slot, w, g, direct in landed:
        wgrads[slot] = _pret(w, g, direct)
    return wgrads


@_math_scoped
class MSCSALevelFn(torch.autograd.Function):
    """One level of the multi-scale cross/self attention (models/layers.py:150-163 of the reference): eight 1x1
    projections of the two maps and the four attentions they feed, as one autograd node.

        ra . [phi_cross_hori | theta_cross_hori | phi_self_hori | theta_self_hori] -> Ya (B, N, 4C)
        re . [phi_cross_vert | theta_cross_vert | phi_self_vert | theta_self_vert] -> Ye
        out1 = attn(K=Ya[0], Q=Ye[1], V=ra) + ra      out2 = attn(K=Ya[2], Q=Ya[3], V=ra)
        out3 = attn(K=Ye[0], Q=Ya[1], V=re) + re      out4 = attn(K=Ye[2], Q=Ye[3], V=re)

    The four projections of a map are ONE GEMM; the backward writes dK / dQ into column blocks of dYa / dYe and
    accumulates both dV of a map in place, so each map's gradient is one GEMM (K = 4C) with dV as its residual term and
    each map's four weight gradients are one split-K GEMM — no gradient-accumulation kernels at all.
    Attention core: the fused kernels where they exist for (N, C) — the projection epilogue then stores the bf16
    operands those kernels read, no fp32 projections and no casts — else GEMM + row-softmax on the fp32 projections
    (the level-0 maps, C = 256), with the same strided operands / outputs.
    Weights: the eight (C, C, 1, 1) parameters in the order of the two lists above.
    cat_bf16 (fused attention kernels only): return ONE bf16 tensor (B,1,H,W,4C) = cat(out1..out4) — the kernels write
    the bf16 copy the decoder concatenates next straight from their accumulators, and the backward reads the four
    column blocks of the incoming (possibly strided: a slice of the concatenation's gradient) bf16 gradient in place: no
    cast or copy kernels on either side.  Otherwise: the four fp32 outputs.

    forward / backward build ONE operand table (a row per attention, SPEC order) and hand it to one attention core: the fused
    kernels (``_level_fwd_flash`` / ``_level_bwd_flash`` choose batched, split-key or per-attention launches) or ``_attn_gemm_*``."""

    #            K source/slot, Q source/slot, V map (0: ra, 1: re), residual
    SPEC = ((0, 0, 1, 1, 0, True), (0, 2, 0, 3, 0, False), (1, 0, 0, 1, 1, True), (1, 2, 1, 3, 1, False))

    @staticmethod
    def forward(ctx, ra, re, cat_bf16, *weights):
        assert len(weights) == 8
        ra, re = _c(ra), _c(re)
        B, _, H, W, C = ra.shape
        N = H * W
        L = rt.lib()
        dev = ra.device
        flash = USE_FLASH and bool(L.hupr_attn_flash_supported(N, C))
        ydt = torch.bfloat16 if flash else torch.float32
        maps = (ra, re)
        infer = bool(int(cat_bf16) & 2)                  # bit 1: the caller runs under no_grad (grad mode is always off in here)
        cat_bf16 = bool(int(cat_bf16) & 1) and flash
        # QS: the query projections leave the GEMM as log2(e) Q (rounded to bf16 once, like every projection), the attention kernels
        # take the exponent of 2 straight from the matrix pipe (csrc/attention_bf16.hip, kDeferBits)
        qscaled = flash and QS_ATTN
        pa, pe = _proj_cat(weights[:4], C), _proj_cat(weights[4:], C)
        Wc = (pa[0], pe[0])                              # plain: the backward GEMMs
        Wf = (pa[1], pe[1]) if qscaled else Wc                # what the forward projections multiply by
        Y = (torch.empty((B, N, 4 * C), dtype=ydt, device=dev), torch.empty((B, N, 4 * C), dtype=ydt, device=dev))
        for x, wc, y in zip(maps, Wf, Y):
            _level_project(x, wc, y, flash)
        outs = [torch.empty((B, 1, H, W, C), dtype=torch.float32, device=dev) for _ in range(4)]
        cat, ld16 = None, 4 * C
        if cat_bf16:
            cat = _level_cat_out.pop("out", None)      # output placement: a channel slice of the decoder stage's input buffer
            if cat is None:
                cat = torch.empty((B, 1, H, W, 4 * C), dtype=torch.bfloat16, device=dev)
            assert tuple(cat.shape) == (B, 1, H, W, 4 * C) and cat.dtype == torch.bfloat16 and _ld_view_ok(cat, 4 * C)
            ld16 = cat.stride(3)
        _level_cat_out.clear()
        vb = (_cast(ra, torch.bfloat16), _cast(re, torch.bfloat16)) if flash else maps
        # per attention: the log-sum-exp per query (fused kernels) or P[query][key]
        aux = [torch.empty((B, N) if flash else (B, N, N), dtype=torch.float32, device=dev) for _ in range(4)]
        tab = [(kp, qp, vb[vs], maps[vs] if residual else None, outs[i], aux[i], cat.data_ptr() + i * C * 2 if cat_bf16 else None)
               for i, ((kp, qp), (_, _, _, _, vs, residual)) in enumerate(zip(_level_blocks(Y, C), MSCSALevelFn.SPEC))]
        if flash:
            _level_fwd_flash(tab, ld16, qscaled, infer, B, N, C, dev)
        else:
            for kp, qp, v, vres, out, P, _ in tab:
                _attn_gemm_fwd(L.hupr_gemm_bf16, False, kp, qp, v, vres, P, out, B, N, C)
        ctx.save_for_backward(ra, re, Wc[0], Wc[1], Y[0], Y[1], vb[0], vb[1], *outs, *aux)
        ctx.weights = weights
        ctx.flash, ctx.cat_bf16, ctx.qscaled = flash, cat_bf16, qscaled
        return (cat,) if cat_bf16 else tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        t = ctx.saved_tensors
        maps, Wc, Y, vb, outs, aux = t[0:2], t[2:4], t[4:6], t[6:8], t[8:12], t[12:16]
        B, _, H, W, C = maps[0].shape
        N = H * W
        dev = maps[0].device
        f32 = torch.float32
        dY = (torch.empty((B, N, 4 * C), dtype=f32, device=dev), torch.empty((B, N, 4 * C), dtype=f32, device=dev))
        dV = (torch.empty((B, N, C), dtype=f32, device=dev), torch.empty((B, N, C), dtype=f32, device=dev))
        scr = torch.empty((B, N) if ctx.flash else (B, N, N), dtype=f32, device=dev)       # row sums / dS of one attention at a time
        dcat, ld = None, 0
        if ctx.cat_bf16:
            # one bf16 gradient (B,1,H,W,4C), typically a column slice of the decoder input's gradient: read in place
            dcat, douts = douts[0], (None,) * 4
            ld = dcat.stride(3)
            if not (dcat.dtype == torch.bfloat16 and dcat.stride(4) == 1 and dcat.stride(2) == W * ld and ld % 8 == 0
                    and (B == 1 or dcat.stride(0) == N * ld) and dcat.data_ptr() % 16 == 0):
                dcat, ld = _cast(dcat, torch.bfloat16), 4 * C
        # SPEC order: the residual attention of a map writes its dV, the other one adds to it
        tab = [(kp, qp, vb[vs], maps[vs], outs[i], aux[i], dkp, dqp, dV[vs], residual)
               for i, ((kp, qp), (dkp, dqp), (_, _, _, _, vs, residual))
               in enumerate(zip(_level_blocks(Y, C), _level_blocks(dY, C), MSCSALevelFn.SPEC))]
        if ctx.flash:
            _level_bwd_flash(tab, dcat, ld, douts, ctx.qscaled, scr, B, N, C)
        else:
            for (kp, qp, _, v, _, P, dkp, dqp, dv, residual), dout in zip(tab, douts):
                dout = _c(dout)
                _attn_gemm_bwd(rt.lib().hupr_gemm_bf16, False, kp, qp, v, P, rt.ptr(dout), residual, not residual, dv, scr, dkp, dqp,
                               B, N, C)
        grads = _level_map_grads(ctx.needs_input_grad, maps, dY, Wc, dV)
        wgrads = _level_weight_grads(ctx.needs_input_grad[3:], ctx.weights, maps, dY)
        return (grads[0], grads[1], None) + tuple(wgrads)


# The PRGCN head stays on the fp32 matrix pipe in bf16 runs.  It is 0.07 % of the model's flops (3 x 1024 x 1024 x 14 per
# sample) but its 1024-term dot products of un-normalised logits are where bf16 operand rounding hurt most: on trained
# (peaky) weights the decoded head went from 94.4 % to >= 99 % arg-max agreement with the fp32 path at B = 32
# (tests/test_trained_gpu.py), for a few tens of microseconds per step.
GCN_MATH = "f32"
GCN_PRODUCTS = True        # test aid: False = the generic fp32 engine instead of csrc/gcn_products.hip


def _gcn_products_ok(F, ld, weight_shape, dtype):
    """The dedicated PRGCN product kernels apply: fp32 pipe (the default of the head in every mode), 16-wide key-point slots."""
    return (GCN_PRODUCTS and (GCN_MATH == "f32" or _st.math == "f32") and dtype == torch.float32 and ld == 16
            and F % 64 == 0 and tuple(weight_shape) == (F, F))


def gcn_route(B, F, ld, weight_shape, dtype, backward=False):
    """Which kernels a PRGCN layer on x (B, F, ld) of ``dtype`` with a weight of ``weight_shape`` runs its products on (host logic
    only): "sliced" (forward of a single sample with F % 1024 == 0: eight K slices of a batched GEMM, summed by the adjacency kernel),
    "products" (csrc/gcn_products.hip) or "generic" (the fp32 / bf16 GEMM engine)."""
    products = _gcn_products_ok(F, ld, weight_shape, dtype)
    if backward:
        return "products" if products and B > 1 else "generic"
    if B == 1 and F % 1024 == 0:
        return "sliced"
    return "products" if products else "generic"


def head_route(region_switched, is_cuda, dtype, channels, weight_shape, num_keypoints):
    """Which kernels the 1x1 head runs on (host logic only): "head1x1" (Head1x1Fn, csrc/head.hip) inside a bf16 run whose "head" region
    is switched to fp32, else "generic" (the generic convolution)."""
    if region_switched and is_cuda and dtype == torch.float32 and channels == 32 and tuple(weight_shape) == (num_keypoints, 32, 1, 1):
        return "head1x1"
    return "generic"


@_math_scoped
class GCNLayerFn(torch.autograd.Function):
    """y = act( (W x) A + bias ) == W (x A) + bias  (models/gcn_networks.py:23-29); x, y: (B, F, ld=16)."""

    @staticmethod
    def forward(ctx, x, weight, bias, adj, relu):
        x = _c(x)
        B, F, ld = x.shape
        K = bias.shape[1]
        L = rt.lib()
        route = gcn_route(B, F, ld, weight.shape, x.dtype)
        if route == "sliced":
            # single-sample inference: F / 128 = 8 workgroups would each walk K = F alone (37 us of latency for 34 MFLOP);
            # eight K slices side by side as a batched GEMM; the adjacency kernel sums them
            S = 8
            t = gemm(0, 0, weight, x, F, ld, F // S, F, ld, S, F // S, (F // S) * ld, math=GCN_MATH)
        elif route == "products":
            S = 1
            t = torch.empty_like(x)
            rt.check(L.hupr_gcn_wx_f32(rt.ptr(_c(weight)), rt.ptr(x), rt.ptr(t), B, F, ld, 0, rt.stream()))
        else:
            S = 1
            t = gemm(0, 0, weight, x, F, ld, F, F, ld, B, 0, F * ld, math=GCN_MATH)
        y = torch.empty_like(x)
        if S > 1:
            rt.check(L.hupr_gcn_adj_fwd_sliced_f32(rt.ptr(t), S, rt.ptr(adj), rt.ptr(_c(bias)), rt.ptr(y), B, F, K, ld, 1 if relu else 0,
                                                   rt.stream()))
        else:
            rt.check(L.hupr_gcn_adj_fwd_f32(rt.ptr(t), rt.ptr(adj), rt.ptr(_c(bias)), rt.ptr(y), B, F, K, ld, 1 if relu else 0,
                                            rt.stream()))
        ctx.save_for_backward(x, weight, y, adj)
        ctx.bias_ref = bias
        ctx.relu, ctx.K = relu, K
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y, adj = ctx.saved_tensors
        B, F, ld = x.shape
        K = ctx.K
        L = rt.lib()
        dt = torch.empty_like(x)
        gm = torch.empty_like(x)
        # weight / bias gradients go straight into the flat-bucket views when a gradient sink is installed
        bias = ctx.bias_ref
        dbias, db_direct = _pgrad(bias) if tuple(bias.shape) == (F, K) and bias.is_contiguous() else (torch.empty((F, K), dtype=torch.float32, device=x.device), False)
        rt.check(L.hupr_gcn_adj_bwd_f32(rt.ptr(_c(dy)), rt.ptr(y), rt.ptr(adj), rt.ptr(dt), rt.ptr(gm), rt.ptr(dbias), B, F, K,
                                        ld, 1 if ctx.relu else 0, rt.stream()))
        if gcn_route(B, F, ld, weight.shape, x.dtype, backward=True) == "products":
            # the batch folded into the matrix pipe's column axis (dx) / reduction axis (dW) in place: csrc/gcn_products.hip
            dx = torch.empty_like(x)
            rt.check(L.hupr_gcn_wx_f32(rt.ptr(_c(weight)), rt.ptr(dt), rt.ptr(dx), B, F, ld, 1, rt.stream()))
            dw, dw_direct = _pgrad(weight)
            rt.check(L.hupr_gcn_dw_f32(rt.ptr(dt), rt.ptr(x), rt.ptr(dw), B, F, ld, rt.stream()))
            return dx, _pret(weight, dw, dw_direct), _pret(bias, dbias, db_direct), None, None
        dx = gemm(1, 0, weight, dt, F, ld, F, F, ld, B, 0, F * ld, math=GCN_MATH)              # W^T dt
        # dW[f][g] = sum_{b,k} dt[b][f][k] x[b][g][k]: fold the batch into the reduction axis
        dt2 = dt.permute(1, 0, 2).reshape(F, B * ld)
        x2 = x.permute(1, 0, 2).reshape(F, B * ld)
        dw = gemm(0, 1, _c(dt2), _c(x2), F, F, B * ld, B * ld, B * ld, 1, 0, 0, math=GCN_MATH)[0]
        return dx, dw, _pret(bias, dbias, db_direct), None, None


def _alloc_head(ws, kinds):
    buf = torch.zeros((16,) + tuple(ws[0].shape[1:]), dtype=torch.float32, device=ws[0].device)
    rows = buf[:ws[0].shape[0]]
    return buf, ((rows, rows),), False


_HEAD_KINDS = (wcache.COPY,)


def _head_w16_cached(weight):
    """The 14 head filters zero-padded to 16 as a PACK-TABLE entry (a plain copy into rows 0..K-1 of a persistent buffer whose other
    rows stay zero), refreshed by the one table launch after an optimiser step."""
    w16 = wcache.lookup((weight,), _HEAD_KINDS, _alloc_head) if tuple(weight.shape[1:]) == (32, 1, 1) else None
    if w16 is None:
        return torch.nn.functional.pad(weight.detach(), (0, 0, 0, 0, 0, 0, 0, 16 - weight.shape[0]))
    return w16


def head_weight16(weight, num_keypoints):
    """The 1x1 head's filters zero-padded to 16 output channels (later kernels stay float4-aligned).  Under no_grad the padded copy
    is the pack-table entry of ``_head_w16_cached`` (one pad launch less per inference forward)."""
    if torch.is_grad_enabled():                                 # training: an ordinary differentiable pad
        return torch.nn.functional.pad(weight, (0, 0, 0, 0, 0, 0, 0, 16 - num_keypoints))
    assert weight.shape[0] == num_keypoints
    return _head_w16_cached(weight)


@_math_scoped
class Head1x1Fn(torch.autograd.Function):
    """The 1x1 key-point head (reference models/layers.py:94) as plain fp32 FMAs: x (B,1,H,W,32) fp32, weight (K,32,1,1) the parameter,
    w16 (16,32,1,1) its zero-padded copy (``_head_w16_cached``) -> (B,1,H,W,16).  What the "head" precision region of a bf16 run uses
    (PRECISION["head"] = "f32"): the generic fp32 implicit-GEMM path costs 0.26 ms per training step on this 58-MFLOP product, these
    kernels ~0.03.  The weight gradient is written for the K real filters only, straight into the gradient sink."""

    @staticmethod
    def forward(ctx, x, weight, w16):
        x, w16 = _c(x), _c(w16)
        B, D, H, W, Ci = _vox(x)
        assert Ci == 32 and tuple(w16.shape) == (16, 32, 1, 1) and x.dtype == torch.float32
        y = torch.empty((B, D, H, W, 16), dtype=torch.float32, device=x.device)
        rt.check(rt.lib().hupr_head1x1_fwd_f32(rt.ptr(x), rt.ptr(w16), rt.ptr(y), B * D * H * W, rt.stream()))
        ctx.save_for_backward(x, w16, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w16, weight = ctx.saved_tensors
        dy = _c(dy)
        M = x.numel() // 32
        L = rt.lib()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw, direct = _pgrad(weight) if ctx.needs_input_grad[1] else (None, False)
        ws = workspace(L.hupr_head1x1_ws_bytes(), x.device)
        rt.check(L.hupr_head1x1_bwd_rows_f32(rt.ptr(x), rt.ptr(w16), rt.ptr(dy), rt.ptr(dx), rt.ptr(dw), weight.shape[0], M, rt.ptr(ws),
                                             ws.numel(), rt.stream()))
        return dx, _pret(weight, dw, direct) if dw is not None else None, None


def head_conv(x, weight, num_keypoints):
    """1x1 head: the dedicated fp32 kernels inside a bf16 run whose "head" region is switched to fp32 (32 -> 16 channels),
    the generic convolution otherwise (the pure fp32 parity path keeps the arithmetic its golden fixtures were pinned with)."""
    if head_route(_st.region_switched, x.is_cuda, x.dtype, x.shape[-1], weight.shape, num_keypoints) == "head1x1":
        return Head1x1Fn.apply(x, weight, _head_w16_cached(weight))
    return conv(x, head_weight16(weight, num_keypoints), None, None, (0, 0, 0))


@_math_scoped
class SigmoidHeadFn(torch.autograd.Function):
    """channels-last logits (B, HW, ld) -> probabilities (B, K, HW) in NCHW order."""

    @staticmethod
    def forward(ctx, x, K):
        x = _c(x)
        B, HW, ld = x.shape
        y = torch.empty((B, K, HW), dtype=torch.float32, device=x.device)
        rt.check(rt.lib().hupr_sigmoid_to_nchw_f32(rt.ptr(x), rt.ptr(y), B, HW, K, ld, rt.stream()))
        ctx.save_for_backward(y)
        ctx.ld = ld
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        B, K, HW = y.shape
        dx = torch.empty((B, HW, ctx.ld), dtype=torch.float32, device=y.device)
        rt.check(rt.lib().hupr_sigmoid_to_nchw_bwd_f32(rt.ptr(_c(dy)), rt.ptr(y), rt.ptr(dx), B, HW, K, ctx.ld, rt.stream()))
        return dx, None


@_math_scoped
class BCEFn(torch.autograd.Function):
    """nn.BCELoss(reduction='mean') on probabilities."""

    @staticmethod
    def forward(ctx, p, t):
        p, t = _c(p), _c(t)
        L = rt.lib()
        loss = torch.empty(1, dtype=torch.float32, device=p.device)
        ws = workspace(L.hupr_bce_ws_bytes(), p.device)
        rt.check(L.hupr_bce_fwd_f32(rt.ptr(p), rt.ptr(t), p.numel(), rt.ptr(loss), rt.ptr(ws), ws.numel(), rt.stream()))
        ctx.save_for_backward(p, t)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        p, t = ctx.saved_tensors
        dp = torch.empty_like(p)
        g = _c(g.reshape(1).to(torch.float32))
        rt.check(rt.lib().hupr_bce_bwd_f32(rt.ptr(p), rt.ptr(t), rt.ptr(g), rt.ptr(dp), p.numel(), rt.stream()))
        return dp, None


@_math_scoped
class PairBCEFn(torch.autograd.Function):
    """(alpha * BCE(p1, t) + beta * BCE(p2, t), BCE(p2, t)) — the two losses of a step and their weighted sum (reference
    misc/losses.py:24-33) as two launches forward and one backward instead of four, two and three torch-native ones; the same floats
    as two BCEFn nodes combined by torch (products and sum rounded separately)."""

    @staticmethod
    def forward(ctx, p1, p2, t, alpha, beta):
        p1, p2, t = _c(p1), _c(p2), _c(t)
        assert p1.shape == p2.shape == t.shape and p1.dtype == p2.dtype == t.dtype == torch.float32
        L = rt.lib()
        out = torch.empty(3, dtype=torch.float32, device=p1.device)
        ws = workspace(2 * L.hupr_bce_ws_bytes(), p1.device)
        rt.check(L.hupr_bce_pair_fwd_f32(rt.ptr(p1), rt.ptr(p2), rt.ptr(t), p1.numel(), float(alpha), float(beta), rt.ptr(out), rt.ptr(ws),
                                         ws.numel(), rt.stream()))
        ctx.save_for_backward(p1, p2, t)
        ctx.ab = (float(alpha), float(beta))
        ctx.set_materialize_grads(False)
        return out[0], out[2]

    @staticmethod
    def backward(ctx, g, g2):
        p1, p2, t = ctx.saved_tensors
        if g is None:
            g = torch.zeros(1, dtype=torch.float32, device=p1.device)
        dp1, dp2 = torch.empty_like(p1), torch.empty_like(p2)
        g = _c(g.reshape(1).to(torch.float32))
        g2 = _c(g2.reshape(1).to(torch.float32)) if g2 is not None else None
        rt.check(rt.lib().hupr_bce_pair_bwd_f32(rt.ptr(p1), rt.ptr(p2), rt.ptr(t), rt.ptr(g), rt.ptr(g2),
                                                ctx.ab[0], ctx.ab[1], rt.ptr(dp1), rt.ptr(dp2), p1.numel(), rt.stream()))
        return dp1, dp2, None, None, None


@_math_scoped
class MinedBCEFn(torch.autograd.Function):
    """PairBCEFn with online hard keypoint mining and per-joint weights (csrc/bce_mined.hip; the rule is stated beside
    hupr_bce_mined_fwd_f32 in include/hupr.h): per head and sample only the ``k`` joints with the largest weighted plane loss carry
    loss and gradient.  ``MinedBCEFn.apply(p1, p2, t, k, joint_w, alpha, beta, counts)`` -> (loss, loss2) with the launches of
    PairBCEFn, two forward and one backward.  p1, p2, t: fp32 GPU tensors of one shape (B, K, ...); ``joint_w``: None or K fp32
    weights on the device; ``counts``: None or a (2, K) int64 device tensor that accumulates how often each joint was selected by
    each head.  ``MinedBCEFn.last_plane_loss`` is the (2, B, K) unweighted plane losses of the latest forward, detached.  Anything
    else raises: there is no fallback to the plain loss."""

    last_plane_loss = None

    @staticmethod
    def forward(ctx, p1, p2, t, k, joint_w, alpha, beta, counts):
        for name, x in (("p1", p1), ("p2", p2), ("t", t)):
            if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
                raise ValueError("MinedBCEFn: %s must be an fp32 GPU tensor, got %s" % (
                    name, "%s on %s" % (x.dtype, x.device) if isinstance(x, torch.Tensor) else type(x).__name__))
        if not (p1.shape == p2.shape == t.shape) or p1.dim() < 2:
            raise ValueError("MinedBCEFn: p1, p2 and t must share one shape (B, K, ...), got %s, %s, %s" % (
                tuple(p1.shape), tuple(p2.shape), tuple(t.shape)))
        B, K = p1.shape[0], p1.shape[1]
        if B < 1 or K < 1 or p1.numel() == 0:
            raise ValueError("MinedBCEFn: empty input %s" % (tuple(p1.shape),))
        HW = p1.numel() // (B * K)
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= K <= 64:
            raise ValueError("MinedBCEFn: k must be an int with 1 <= k <= K <= 64, got k = %r, K = %d" % (k, K))
        if joint_w is not None and not (isinstance(joint_w, torch.Tensor) and joint_w.device == p1.device and joint_w.is_contiguous()
                                        and joint_w.dtype == torch.float32 and tuple(joint_w.shape) == (K,)):
            raise ValueError("MinedBCEFn: joint_w must be None or %d contiguous fp32 weights on %s" % (K, p1.device))
        if counts is not None and not (isinstance(counts, torch.Tensor) and counts.device == p1.device and counts.is_contiguous()
                                       and counts.dtype == torch.int64 and tuple(counts.shape) == (2, K)):
            raise ValueError("MinedBCEFn: counts must be None or a contiguous (2, %d) int64 tensor on %s" % (K, p1.device))
        p1, p2, t = _c(p1), _c(p2), _c(t)
        out = torch.empty(3, dtype=torch.float32, device=p1.device)
        plane_loss = torch.empty((2, B, K), dtype=torch.float32, device=p1.device)
        coef = torch.empty((2, B, K), dtype=torch.float32, device=p1.device)
        rt.check(rt.lib().hupr_bce_mined_fwd_f32(rt.ptr(p1), rt.ptr(p2), rt.ptr(t), B, K, HW, k, rt.ptr(joint_w), float(alpha), float(beta),
                                                 rt.ptr(out), rt.ptr(plane_loss), rt.ptr(coef), rt.ptr(counts), rt.stream()))
        ctx.save_for_backward(p1, p2, t, coef)
        ctx.ab = (float(alpha), float(beta))
        ctx.set_materialize_grads(False)
        MinedBCEFn.last_plane_loss = plane_loss
        return out[0], out[2]

    @staticmethod
    def backward(ctx, g, g2):
        p1, p2, t, coef = ctx.saved_tensors
        if g is None:
            g = torch.zeros(1, dtype=torch.float32, device=p1.device)
        dp1, dp2 = torch.empty_like(p1), torch.empty_like(p2)
        g = _c(g.reshape(1).to(torch.float32))
        g2 = _c(g2.reshape(1).to(torch.float32)) if g2 is not None else None
        B, K = p1.shape[0], p1.shape[1]
        rt.check(rt.lib().hupr_bce_mined_bwd_f32(rt.ptr(p1), rt.ptr(p2), rt.ptr(t), rt.ptr(coef), rt.ptr(g), rt.ptr(g2), ctx.ab[0], ctx.ab[1],
                                                 rt.ptr(dp1), rt.ptr(dp2), B, K, p1.numel() // (B * K), rt.stream()))
        return dp1, dp2, None, None, None, None, None, None


@_math_scoped
class CoordLossFn(torch.autograd.Function):
    """Integral (soft-arg-max) coordinate loss on both heads (csrc/coord_loss.hip; the rule is stated beside
    hupr_coord_loss_fwd_f32 in include/hupr.h): an L1 on the offset of each heat-map's mass centroid from its joint, in heat-map
    pixels.  ``CoordLossFn.apply(p1, p2, joints, stride, snap, joint_w, a0, a1, acc)`` -> (coord_loss, c_heads): coord_loss =
    a0 C_0 + a1 C_1, c_heads the detached (C_0, C_1); two launches forward, one backward.  p1, p2: fp32 GPU tensors of one shape
    (B, K, H, H); ``joints``: (B, K, 2) image pixels of any real dtype on that device; ``stride``: image pixels per heat-map pixel;
    ``snap``: the joints' target is the whole heat-map pixel ``gaussian_targets`` centres its patch on; ``joint_w``: None or K fp32
    weights on the device; ``acc``: None or 3 fp64 on the device, which accumulate (C_0, C_1, 1) per call.  The damping of the
    rule is ``CoordLossFn.eps``.  ``CoordLossFn.last_residual`` is the (2, B, K, 2) residuals of the latest forward, detached.  No
    gradient flows to the joints.  Anything else raises: there is no fallback."""

    eps = 1.0
    last_residual = None

    @staticmethod
    def forward(ctx, p1, p2, joints, stride, snap, joint_w, a0, a1, acc):
        for name, x in (("p1", p1), ("p2", p2)):
            if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
                raise ValueError("CoordLossFn: %s must be an fp32 GPU tensor, got %s" % (
                    name, "%s on %s" % (x.dtype, x.device) if isinstance(x, torch.Tensor) else type(x).__name__))
        if p1.shape != p2.shape or p1.device != p2.device or p1.dim() != 4 or p1.shape[2] != p1.shape[3] or p1.numel() == 0:
            raise ValueError("CoordLossFn: p1 and p2 must share one shape (B, K, H, H) and one device, got %s, %s" % (
                tuple(p1.shape), tuple(p2.shape)))
        B, K, H = p1.shape[0], p1.shape[1], p1.shape[2]
        if K > 64 or H > 4096:
            raise ValueError("CoordLossFn: K <= 64 and H <= 4096, got K = %d, H = %d" % (K, H))
        if not isinstance(joints, torch.Tensor) or joints.device != p1.device or tuple(joints.shape) != (B, K, 2) \
                or joints.dtype == torch.bool or joints.is_complex():
            raise ValueError("CoordLossFn: joints must be (%d, %d, 2) of a real dtype on %s, got %s" % (
                B, K, p1.device, "%s %s on %s" % (tuple(joints.shape), joints.dtype, joints.device)
                if isinstance(joints, torch.Tensor) else type(joints).__name__))
        if isinstance(stride, bool) or not isinstance(stride, (int, float)) or not (0 < stride < float("inf")):
            raise ValueError("CoordLossFn: stride must be a positive finite number, got %r" % (stride,))
        if joint_w is not None and not (isinstance(joint_w, torch.Tensor) and joint_w.device == p1.device and joint_w.is_contiguous()
                                        and joint_w.dtype == torch.float32 and tuple(joint_w.shape) == (K,)):
            raise ValueError("CoordLossFn: joint_w must be None or %d contiguous fp32 weights on %s" % (K, p1.device))
        if acc is not None and not (isinstance(acc, torch.Tensor) and acc.device == p1.device and acc.is_contiguous()
                                    and acc.dtype == torch.float64 and tuple(acc.shape) == (3,)):
            raise ValueError("CoordLossFn: acc must be None or 3 contiguous fp64 on %s" % (p1.device,))
        p1, p2, joints = _c(p1), _c(p2), _c(joints.to(torch.float32))
        out = torch.empty(3, dtype=torch.float32, device=p1.device)
        resid = torch.empty((2, B, K, 2), dtype=torch.float32, device=p1.device)
        scale = torch.empty((2, B, K), dtype=torch.float32, device=p1.device)
        rt.check(rt.lib().hupr_coord_loss_fwd_f32(rt.ptr(p1), rt.ptr(p2), rt.ptr(joints), B, K, H, float(stride), int(bool(snap)),
                                                  rt.ptr(joint_w), float(CoordLossFn.eps), float(a0), float(a1), rt.ptr(out),
                                                  rt.ptr(resid), rt.ptr(scale), rt.ptr(acc), rt.stream()))
        ctx.save_for_backward(resid, scale, joints)
        ctx.args = (B, K, H, float(stride), int(bool(snap)), float(a0), float(a1))
        ctx.set_materialize_grads(False)
        CoordLossFn.last_residual = resid
        c_heads = out[1:]
        ctx.mark_non_differentiable(c_heads)
        return out[0], c_heads

    @staticmethod
    def backward(ctx, g, _g_heads):
        resid, scale, joints = ctx.saved_tensors
        B, K, H, stride, snap, a0, a1 = ctx.args
        if g is None:
            g = torch.zeros(1, dtype=torch.float32, device=resid.device)
        dp1 = torch.empty((B, K, H, H), dtype=torch.float32, device=resid.device)
        dp2 = torch.empty_like(dp1)
        g = _c(g.reshape(1).to(torch.float32))
        rt.check(rt.lib().hupr_coord_loss_bwd_f32(rt.ptr(resid), rt.ptr(scale), rt.ptr(joints), rt.ptr(g), B, K, H, stride, snap, a0, a1,
                                                  rt.ptr(dp1), rt.ptr(dp2), rt.stream()))
        return dp1, dp2, None, None, None, None, None, None, None


def default_bones():
    """The bone table of the data set's skeleton (``datasets.base.SKELETON``, 13 edges over the 14 joints) with zero-based indices."""
    from .datasets.base import SKELETON
    return tuple((u - 1, v - 1) for u, v in SKELETON)


def bone_table(bones, K):
    """``bones`` (None = ``default_bones()``, else a sequence of (u, v) pairs of ints) -> a tuple of E pairs, checked as
    hupr_bone_loss_fwd_f32 checks them: 1 <= E <= 32, indices in [0, K), u != v."""
    if bones is None:
        bones = default_bones()
    try:
        table = tuple((u, v) for u, v in bones)
    except (TypeError, ValueError):
        raise ValueError("BoneLossFn: bones must be None or a sequence of (u, v) pairs, got %r" % (bones,))
    if not 1 <= len(table) <= 32:
        raise ValueError("BoneLossFn: 1 to 32 bones, got %d" % len(table))
    for u, v in table:
        if not all(isinstance(i, (int, np.integer)) and not isinstance(i, bool) and 0 <= i < K for i in (u, v)) or u == v:
            raise ValueError("BoneLossFn: a bone joins two different joints of [0, %d), got %r" % (K, (u, v)))
    return tuple((int(u), int(v)) for u, v in table)


@_math_scoped
class BoneLossFn(torch.autograd.Function):
    """Bone-vector loss on both heads (csrc/bone_loss.hip; the rule is stated beside hupr_bone_loss_fwd_f32 in include/hupr.h): an
    L1, in heat-map pixels, on the error of the vector between the mass centroids of the two maps at the ends of every bone.
    ``BoneLossFn.apply(p1, p2, joints, stride, snap, bones, bone_w, a0, a1, acc)`` -> (bone_loss, b_heads): bone_loss = a0 B_0 +
    a1 B_1, b_heads the detached (B_0, B_1); two launches forward, one backward.  p1, p2, joints, stride, snap: as in
    ``CoordLossFn``; ``bones``: None (``default_bones()``, which needs K = 14) or a sequence of 1 to 32 (u, v) pairs of different
    joints in [0, K); ``bone_w``: None or E fp32 weights on the device; ``acc``: None or 3 fp64 on the device, which accumulate
    (B_0, B_1, 1) per call.  The damping of the rule is ``BoneLossFn.eps``.  ``BoneLossFn.last_residual`` is the (2, B, E, 2) bone
    residuals of the latest forward, detached.  No gradient flows to the joints.  Anything else raises: there is no fallback."""

    eps = 1.0
    last_residual = None

    @staticmethod
    def forward(ctx, p1, p2, joints, stride, snap, bones, bone_w, a0, a1, acc):
        for name, x in (("p1", p1), ("p2", p2)):
            if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
                raise ValueError("BoneLossFn: %s must be an fp32 GPU tensor, got %s" % (
                    name, "%s on %s" % (x.dtype, x.device) if isinstance(x, torch.Tensor) else type(x).__name__))
        if p1.shape != p2.shape or p1.device != p2.device or p1.dim() != 4 or p1.shape[2] != p1.shape[3] or p1.numel() == 0:
            raise ValueError("BoneLossFn: p1 and p2 must share one shape (B, K, H, H) and one device, got %s, %s" % (
                tuple(p1.shape), tuple(p2.shape)))
        B, K, H = p1.shape[0], p1.shape[1], p1.shape[2]
        if K > 64 or H > 4096:
            raise ValueError("BoneLossFn: K <= 64 and H <= 4096, got K = %d, H = %d" % (K, H))
        if not isinstance(joints, torch.Tensor) or joints.device != p1.device or tuple(joints.shape) != (B, K, 2) \
                or joints.dtype == torch.bool or joints.is_complex():
            raise ValueError("BoneLossFn: joints must be (%d, %d, 2) of a real dtype on %s, got %s" % (
                B, K, p1.device, "%s %s on %s" % (tuple(joints.shape), joints.dtype, joints.device)
                if isinstance(joints, torch.Tensor) else type(joints).__name__))
        if isinstance(stride, bool) or not isinstance(stride, (int, float)) or not (0 < stride < float("inf")):
            raise ValueError("BoneLossFn: stride must be a positive finite number, got %r" % (stride,))
        table = bone_table(bones, K)
        E = len(table)
        if bone_w is not None and not (isinstance(bone_w, torch.Tensor) and bone_w.device == p1.device and bone_w.is_contiguous()
                                       and bone_w.dtype == torch.float32 and tuple(bone_w.shape) == (E,)):
            raise ValueError("BoneLossFn: bone_w must be None or %d contiguous fp32 weights on %s" % (E, p1.device))
        if acc is not None and not (isinstance(acc, torch.Tensor) and acc.device == p1.device and acc.is_contiguous()
                                    and acc.dtype == torch.float64 and tuple(acc.shape) == (3,)):
            raise ValueError("BoneLossFn: acc must be None or 3 contiguous fp64 on %s" % (p1.device,))
        p1, p2, joints = _c(p1), _c(p2), _c(joints.to(torch.float32))
        out = torch.empty(3, dtype=torch.float32, device=p1.device)
        resid = torch.empty((2, B, K, 2), dtype=torch.float32, device=p1.device)
        inv_den = torch.empty((2, B, K), dtype=torch.float32, device=p1.device)
        bone_resid = torch.empty((2, B, E, 2), dtype=torch.float32, device=p1.device)
        gcoef = torch.empty((2, B, K, 2), dtype=torch.float32, device=p1.device)
        host = (ctypes.c_int * (2 * E))(*[i for uv in table for i in uv])
        rt.check(rt.lib().hupr_bone_loss_fwd_f32(rt.ptr(p1), rt.ptr(p2), rt.ptr(joints), B, K, H, float(stride), int(bool(snap)), host, E,
                                                 rt.ptr(bone_w), float(BoneLossFn.eps), float(a0), float(a1), rt.ptr(out), rt.ptr(resid),
                                                 rt.ptr(inv_den), rt.ptr(bone_resid), rt.ptr(gcoef), rt.ptr(acc), rt.stream()))
        ctx.save_for_backward(resid, inv_den, gcoef, joints)
        ctx.args = (B, K, E, H, float(stride), int(bool(snap)), float(a0), float(a1))
        ctx.set_materialize_grads(False)
        BoneLossFn.last_residual = bone_resid
        b_heads = out[1:]
        ctx.mark_non_differentiable(b_heads)
        return out[0], b_heads

    @staticmethod
    def backward(ctx, g, _g_heads):
        resid, inv_den, gcoef, joints = ctx.saved_tensors
        B, K, E, H, stride, snap, a0, a1 = ctx.args
        if g is None:
            g = torch.zeros(1, dtype=torch.float32, device=resid.device)
        dp1 = torch.empty((B, K, H, H), dtype=torch.float32, device=resid.device)
        dp2 = torch.empty_like(dp1)
        g = _c(g.reshape(1).to(torch.float32))
        rt.check(rt.lib().hupr_bone_loss_bwd_f32(rt.ptr(resid), rt.ptr(inv_den), rt.ptr(gcoef), rt.ptr(joints), rt.ptr(g), B, K, E, H,
                                                 stride, snap, a0, a1, rt.ptr(dp1), rt.ptr(dp2), rt.stream()))
        return dp1, dp2, None, None, None, None, None, None, None, None


_PATCH_CACHE = {}


def gaussian_targets(joints, hsize=64, isize=256, sigma=2):
    """joints (B,K,2) int64 GPU tensor -> (B,K,H,W) fp32 targets (misc/utils.py:6-66)."""
    joints = _c(joints.to(torch.int64))
    B, K, _ = joints.shape
    rad = 3 * sigma
    key = (sigma, joints.device)
    if key not in _PATCH_CACHE:
        ax = np.arange(2 * rad + 1, dtype=np.float32)
        g = np.exp(-((ax[None, :] - rad) ** 2 + (ax[:, None] - rad) ** 2) / (2 * sigma ** 2))
        _PATCH_CACHE[key] = torch.from_numpy(g.astype(np.float32)).to(joints.device)
    t = torch.empty((B, K, hsize, hsize), dtype=torch.float32, device=joints.device)
    rt.check(rt.lib().hupr_gaussian_targets_f32(rt.ptr(joints), rt.ptr(_PATCH_CACHE[key]), rt.ptr(t), B * K, hsize, rad,
                                               float(isize) / float(hsize), rt.stream()))
    return t


def gaussian_targets_subpixel(joints, hsize=64, isize=256, sigma=2):
    """joints (B,K,2) GPU tensor of any real dtype, image pixels with their fractions -> (B,K,H,W) fp32 targets whose Gaussian is
    centred on the joint's real position inside the window ``gaussian_targets`` pastes (csrc/targets.hip; the rule is stated beside
    hupr_gaussian_targets_subpixel_f32 in include/hupr.h).  One launch, no host table; a joint that is not finite gives a zero plane."""
    if not isinstance(joints, torch.Tensor) or joints.dim() != 3 or joints.shape[-1] != 2:
        raise ValueError("gaussian_targets_subpixel needs (B, K, 2) joints, got %s" %
                         (tuple(joints.shape) if isinstance(joints, torch.Tensor) else type(joints).__name__,))
    if joints.dtype == torch.bool or joints.is_complex():
        raise ValueError("gaussian_targets_subpixel needs joints of a real dtype, got %s" % joints.dtype)
    if not joints.is_cuda:
        raise rt.HuprError("tensor is on %s; the HIP path needs a GPU tensor (no CPU fallback)" % joints.device)
    joints = _c(joints.to(torch.float32))
    B, K, _ = joints.shape
    t = torch.empty((B, K, hsize, hsize), dtype=torch.float32, device=joints.device)
    rt.check(rt.lib().hupr_gaussian_targets_subpixel_f32(rt.ptr(joints), rt.ptr(t), B * K, hsize, float(sigma), int(3 * sigma),
                                                        float(isize) / float(hsize), rt.stream()))
    return t


_I32, _F32 = torch.int32, torch.float32


def _outputs(name, out, lead, device, slots):
    """``name``'s outputs, one per slot — (tail shape, dtype), or None where the call returns None: new ``lead + tail`` tensors on
    ``device`` or, nothing allocated, the caller's own tuple ``out`` once each entry fits its slot (a ValueError before any launch)."""
    if out is None:
        return tuple(s and torch.empty(lead + s[0], dtype=s[1], device=device) for s in slots)
    if not isinstance(out, (tuple, list)) or len(out) != len(slots):
        raise ValueError("%s: out must be a tuple of %d entries, got %s" % (name, len(slots), type(out).__name__))
    for k, (t, s) in enumerate(zip(out, slots)):
        fits = t is None if s is None else (isinstance(t, torch.Tensor) and tuple(t.shape) == lead + s[0] and t.dtype == s[1]
                                            and t.device == device and t.is_contiguous())
        if not fits:
            want = "None" if s is None else "a contiguous %s tensor of shape %r on %s" % (s[1], lead + s[0], device)
            got = "%s %r with strides %r on %s" % (t.dtype, tuple(t.shape), t.stride(), t.device) if isinstance(t, torch.Tensor) else repr(t)
            raise ValueError("%s: out[%d] must be %s, got %s" % (name, k, want, got))
    return tuple(out)


def argmax_rows(p, out=None):
    """p (rows, n) GPU -> (idx int32 (rows,), maxval (rows,)) with first-max tie-break.  ``out``: that tuple, to write (``_outputs``)."""
    p = _c(p)
    rows, n = p.shape
    idx, mx = _outputs("argmax_rows", out, (rows,), p.device, (((), _I32), ((), _F32)))
    rt.check(rt.lib().hupr_argmax_rows_f32(rt.ptr(p), rows, n, rt.ptr(idx), rt.ptr(mx), rt.stream()))
    return idx, mx


def _pose_state(bytes_fn, rows, device):
    """A zero-filled ("never seen") per-row state of the size the library's ``bytes_fn(rows)`` gives, as (rows, floats) fp32."""
    n = int(bytes_fn(rows)) // 4
    return torch.zeros((rows, n // max(rows, 1)), dtype=torch.float32, device=device)


def _pose_heat(name, heat):
    """heat (..., H, W) fp32, checked in ``name``'s name -> (contiguous heat, lead shape, rows, H, W)."""
    if heat.dim() < 2:
        raise ValueError("%s needs (..., H, W) heat-maps, got shape %r" % (name, tuple(heat.shape)))
    if heat.dtype != torch.float32:
        raise ValueError("%s needs fp32 heat-maps, got %s" % (name, heat.dtype))
    heat = _c(heat)
    lead, (H, W) = tuple(heat.shape[:-2]), heat.shape[-2:]
    return heat, lead, int(np.prod(lead, dtype=np.int64)), H, W


def _pose_decode(name, checked, mode, ratio, filter_state, smoothing, out):
    """Launch for the two plain decodes: ``name`` is the function's and, as hupr_<name>_f32, its library entry's, ``checked`` what
    ``_pose_heat`` returned, ``mode`` the one argument in which the two differ (refine / radius), ``out`` see ``_outputs``."""
    if (filter_state is None) != (smoothing is None):
        raise ValueError("filter_state and smoothing go together")
    heat, lead, rows, H, W = checked
    params, xy = (0.0,) * 5, None                                     # without a filter: no filtered keypoints, no velocity
    if filter_state is not None:
        if filter_state.dtype != torch.float32 or filter_state.numel() * 4 != int(rt.lib().hupr_pose_filter_state_bytes(rows)):
            raise ValueError("filter_state must be the fp32 tensor pose_filter_state(%d, device) returns" % rows)
        params, xy = tuple(float(getattr(smoothing, k)) for k in ("rate_hz", "min_cutoff", "beta", "d_cutoff", "min_score")), ((2,), _F32)
    out = _outputs(name, out, lead, heat.device, (((), _I32), ((), _F32), ((2,), _F32), xy, xy))
    entry = getattr(rt.lib(), "hupr_%s_f32" % name)
    rt.check(entry(rt.ptr(heat), rows, H, W, float(ratio), mode, rt.ptr(filter_state), *params, *map(rt.ptr, out), rt.stream()))
    return out


def pose_filter_state(rows, device):
    """A zero-filled ("never seen") One-Euro filter state for ``rows`` (sample, joint) rows: (rows, 8) fp32."""
    return _pose_state(rt.lib().hupr_pose_filter_state_bytes, rows, device)


def pose_decode(heat, ratio, refine=True, filter_state=None, smoothing=None, out=None):
    """heat (..., H, W) fp32 GPU -> (idx int32 (...), maxval (...), raw keypoints (..., 2), filtered keypoints, velocity) in one launch
    (csrc/pose_decode.hip; the rule is stated beside hupr_pose_decode_f32 in include/hupr.h).  ``idx`` / ``maxval`` are
    ``argmax_rows``' bits; the keypoints are (x, y) in heat-map pixels times ``ratio``, refined to sub-pixel position unless
    ``refine`` is false.  ``filter_state`` (``pose_filter_state``, advanced in place) together with ``smoothing`` (an object with
    ``rate_hz``, ``min_cutoff``, ``beta``, ``d_cutoff``, ``min_score``: tools.stream.PoseSmoothing) adds the One-Euro filter: the
    filtered keypoints and the velocity in pixels per second, both None without it.  ``out``: that 5-tuple, to write
    (``_outputs``).  Device tensors, no sync."""
    checked = _pose_heat("pose_decode", heat)
    return _pose_decode("pose_decode", checked, int(bool(refine)), ratio, filter_state, smoothing, out)


def pose_decode_integral(heat, ratio, radius, filter_state=None, smoothing=None, out=None):
    """heat (..., H, W) fp32 GPU -> ``pose_decode``'s 5-tuple in one launch (csrc/pose_integral.hip; the rule is stated beside
    hupr_pose_decode_integral_f32 in include/hupr.h): the raw keypoint is the mass centroid of the weights max(h, 0) over the window
    of ``radius`` pixels around the arg-max, clipped to the map, times ``ratio``; ``radius`` 0 is the whole map, the centroid the
    integral coordinate loss trains.  ``idx`` / ``maxval`` are ``argmax_rows``' bits.  ``filter_state``, ``smoothing`` and ``out`` are
    ``pose_decode``'s: the same state tensor, the same One-Euro filter (csrc/pose_filter.h).  Device tensors, no sync."""
    checked = _pose_heat("pose_decode_integral", heat)
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius < 2 ** 31:
        raise ValueError("pose_decode_integral needs an integer radius >= 0 (0 = the whole map), got %r" % (radius,))
    return _pose_decode("pose_decode_integral", checked, int(radius), ratio, filter_state, smoothing, out)


TRACK_UPDATED, TRACK_COASTED_MISSING, TRACK_COASTED_GATED, TRACK_STARTED, TRACK_LOST = range(5)      # pose_track's status codes
_TRACK_PARAMS = ("rate_hz", "accel_psd", "meas_std", "heatmap_gain", "gate", "max_coast", "init_speed_std", "min_score", "horizon_s")


def pose_track_state(rows, device):
    """A zero-filled ("never seen") Kalman track state for ``rows`` (sample, joint) rows: (rows, 16) fp32 = x, y, vx, vy, the upper
    triangle of the 4 x 4 covariance row by row, live, coast."""
    return _pose_state(rt.lib().hupr_pose_track_state_bytes, rows, device)


def pose_imm_state(rows, device):
    """A zero-filled ("never seen") state of the two-model tracker (``pose_track`` with ``tracking.accel_psd_moving``) for ``rows``
    rows: (rows, 32) fp32 = the still model's x, y, vx, vy and covariance triangle, the moving model's same 14, the two mode
    probabilities, live, coast."""
    return _pose_state(rt.lib().hupr_pose_track_imm_state_bytes, rows, device)


MAX_CANDIDATES = 4                  # of pose_track's association and of pose_peaks


def check_peaks(K, min_separation, peak_ratio, name="pose_peaks"):
    """The three candidate parameters of ``pose_peaks`` and of the associating ``pose_track``, checked in ``name``'s name ->
    (int K in 1..4, int min_separation >= 0 in heat-map pixels, float peak_ratio in (0, 1])."""
    for what, v in (("K", K), ("min_separation", min_separation)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s needs an integer %s, got %r" % (name, what, v))
    if not 1 <= K <= MAX_CANDIDATES:
        raise ValueError("%s needs K in 1..%d, got %r" % (name, MAX_CANDIDATES, K))
    if not 0 <= min_separation < 2 ** 31:
        raise ValueError("%s needs min_separation >= 0, got %r" % (name, min_separation))
    if isinstance(peak_ratio, bool) or not isinstance(peak_ratio, (int, float, np.integer, np.floating)) or not 0 < peak_ratio <= 1:
        raise ValueError("%s needs peak_ratio in (0, 1], got %r" % (name, peak_ratio))
    return int(K), int(min_separation), float(peak_ratio)


MAX_GROUP_ROWS = 32                 # joints in a group of the pair tracker (hupr_pose_track_pairs_f32)


def check_pair_table(pairs, swap_cost, group, name="pose_track"):
    """The two pair-tracker settings, checked in ``name``'s name for groups of ``group`` rows -> (the partner table as a list of
    ``group`` ints: entry j the partner of joint j or j itself, its own inverse; float swap_cost >= 0, finite)."""
    if not 1 <= group <= MAX_GROUP_ROWS:
        raise ValueError("%s pairs joints inside groups of 1..%d rows (the last lead axis of the heat-maps), got %d"
                         % (name, MAX_GROUP_ROWS, group))
    try:
        table = list(pairs)
    except TypeError:
        raise ValueError("%s with pair_swap needs tracking.pairs, one partner per joint of the group of %d, got %r"
                         % (name, group, pairs)) from None
    if len(table) != group:
        raise ValueError("%s needs one tracking.pairs entry per joint of the group of %d, got %d" % (name, group, len(table)))
    for j, q in enumerate(table):
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 0 <= q < group or table[q] != j:
            raise ValueError("%s: tracking.pairs[%d] = %r: every entry is a joint of the group, and the partner's partner is the joint "
                             "itself" % (name, j, q))
    if (isinstance(swap_cost, bool) or not isinstance(swap_cost, (int, float, np.integer, np.floating))
            or not 0 <= swap_cost <= 3.0e38):                                           # finite as an fp32 launch argument
        raise ValueError("%s needs a finite swap_cost >= 0, got %r" % (name, swap_cost))
    return [int(q) for q in table], float(swap_cost)


def pose_peaks(heat, ratio, K, min_separation=3, peak_ratio=0.25, refine=True):
    """heat (..., H, W) fp32 GPU -> (positions (..., K, 2) in image pixels, scores (..., K), pixel indices int32 (..., K), count int32
    (...)): the up to ``K`` <= 4 peaks of every map that the associating tracker chooses among, in one launch and without a tracker
    (csrc/pose_assoc.hip; the rule is stated beside hupr_pose_track_assoc_f32 in include/hupr.h).  Peak 0 is ``pose_decode``'s
    arg-max; the others are the next 3 x 3 local maxima by value that are at least ``peak_ratio`` times as high and lie more than
    ``min_separation`` heat-map pixels (Chebyshev) from every peak taken; slots past the count hold zeros.  Device tensors, no sync."""
    heat, lead, rows, H, W = _pose_heat("pose_peaks", heat)
    K, min_separation, peak_ratio = check_peaks(K, min_separation, peak_ratio)
    xy, score, index, count = _outputs("pose_peaks", None, lead, heat.device, (((K, 2), _F32), ((K,), _F32), ((K,), _I32), ((), _I32)))
    rt.check(rt.lib().hupr_pose_peaks_f32(rt.ptr(heat), rows, H, W, float(ratio), int(bool(refine)), K, min_separation, peak_ratio,
                                          rt.ptr(xy), rt.ptr(score), rt.ptr(index), rt.ptr(count), rt.stream()))
    return xy, score, index, count


def _present_group(present, lead, device):
    """``pose_track``'s ``present`` flags checked against the lead shape of its heat-maps -> rows per flag (1 without flags)."""
    if present is None:
        return 1
    if (not isinstance(present, torch.Tensor) or present.dtype != torch.int32 or tuple(present.shape) != lead[:-1]
            or not present.is_contiguous()):
        raise ValueError("present must be a contiguous int32 tensor of shape %r (one flag per group of %d rows)"
                         % (lead[:-1], lead[-1] if lead else 1))
    if present.device != device:
        raise ValueError("present is on %s, the heat-maps on %s" % (present.device, device))
    return lead[-1] if lead else 1


def pose_track(heat, ratio, refine=True, track_state=None, tracking=None, present=None, out=None):
    """heat (..., H, W) fp32 GPU -> (idx int32 (...), maxval (...), raw keypoints (..., 2), filtered keypoints (..., 2), velocity
    (..., 2), position covariance (..., 3) = (Pxx, Pxy, Pyy), forecast (..., 2), status int32 (...)) in one launch
    (csrc/pose_track.hip; the rule is stated beside hupr_pose_track_f32 in include/hupr.h).  ``idx`` / ``maxval`` / raw keypoints are
    ``pose_decode``'s bits.  ``track_state`` (``pose_track_state``, advanced in place) and ``tracking`` (an object with ``rate_hz``,
    ``accel_psd``, ``meas_std``, ``heatmap_gain``, ``gate``, ``max_coast``, ``init_speed_std``, ``min_score``, ``horizon_s``:
    tools.stream.PoseTracking) are both required.  One call is one frame.  Device tensors, no sync.
    With ``tracking.candidates`` > 1, or with ``present`` (int32, the shape of ``heat`` without its last three axes: one flag per
    group of joints, 0 = nobody there, the group has no measurement in this frame), the launch is the associating tracker's
    (csrc/pose_assoc.hip, hupr_pose_track_assoc_f32): it reads ``tracking.candidates``, ``min_separation`` and ``peak_ratio`` too and
    returns the eight outputs plus (candidate positions (..., K, 2), candidate scores (..., K), candidate count int32 (...), chosen
    int32 (...), -1 where no measurement went into the state).  ``out``: the returned 8- or 12-tuple, to write (``_outputs``).
    With ``tracking.pair_swap`` the launch is the pair tracker's (csrc/pose_pairs.hip, hupr_pose_track_pairs_f32): the last lead axis
    of ``heat`` is the group of joints, ``tracking.pairs`` names every joint's partner in it (itself for a joint without one) and
    ``tracking.swap_cost`` prices a peak from the partner's map; partner rows share the peaks of both maps.  It returns those twelve
    plus source int32 (...): 0 the measurement came from the row's own map, 1 from its partner's, -1 none; ``out`` is that 13-tuple.
    With ``tracking.accel_psd_moving`` (not None) the launch is the two-model tracker's (csrc/pose_imm.hip, hupr_pose_track_imm_f32):
    a still filter with ``accel_psd`` and a moving one with ``accel_psd_moving`` run on the arg-max measurement, coupled by
    ``tracking.switch_prob`` and started with ``tracking.moving_prior``; ``track_state`` is ``pose_imm_state``'s, ``present`` is
    allowed, ``candidates`` > 1 and ``pair_swap`` are not.  It returns the eight outputs — the mixture of the two models — plus moving
    (...): the probability of the moving model, 0 without a live track; ``out`` is that 9-tuple."""
    heat, lead, rows, H, W = _pose_heat("pose_track", heat)
    if track_state is None or tracking is None:
        raise ValueError("pose_track needs its track_state and its tracking parameters")
    imm = getattr(tracking, "accel_psd_moving", None) is not None
    state_bytes, state_name = ((rt.lib().hupr_pose_track_imm_state_bytes, "pose_imm_state") if imm else
                               (rt.lib().hupr_pose_track_state_bytes, "pose_track_state"))
    if (not isinstance(track_state, torch.Tensor) or track_state.dtype != torch.float32 or not track_state.is_contiguous()
            or track_state.numel() * 4 != int(state_bytes(rows))):
        raise ValueError("track_state must be the fp32 tensor %s(%d, device) returns" % (state_name, rows))
    if track_state.device != heat.device:
        raise ValueError("track_state is on %s, the heat-maps on %s" % (track_state.device, heat.device))
    params = tuple(int(getattr(tracking, k)) if k == "max_coast" else float(getattr(tracking, k)) for k in _TRACK_PARAMS)
    slots = (((), _I32), ((), _F32)) + (((2,), _F32),) * 3 + (((3,), _F32), ((2,), _F32), ((), _I32))
    K = getattr(tracking, "candidates", 1)
    paired = getattr(tracking, "pair_swap", False)
    if imm:
        if K != 1 or paired:
            raise ValueError("pose_track: accel_psd_moving goes with the arg-max measurement only, not with candidates > 1 or pair_swap")
        group = _present_group(present, lead, heat.device)
        out = _outputs("pose_track", out, lead, heat.device, slots + (((), _F32),))
        rt.check(rt.lib().hupr_pose_track_imm_f32(rt.ptr(heat), rows, H, W, float(ratio), int(bool(refine)), rt.ptr(track_state), *params,
                                                  float(tracking.accel_psd_moving), float(getattr(tracking, "switch_prob", 0.05)),
                                                  float(getattr(tracking, "moving_prior", 0.5)), rt.ptr(present), group,
                                                  *map(rt.ptr, out), rt.stream()))
        return out
    if K == 1 and present is None and not paired:
        out = _outputs("pose_track", out, lead, heat.device, slots)
        rt.check(rt.lib().hupr_pose_track_f32(rt.ptr(heat), rows, H, W, float(ratio), int(bool(refine)), rt.ptr(track_state), *params,
                                              *map(rt.ptr, out), rt.stream()))
        return out
    K, sep, floor = check_peaks(K, getattr(tracking, "min_separation", 3), getattr(tracking, "peak_ratio", 0.25), "pose_track")
    group = _present_group(present, lead, heat.device)
    slots += (((K, 2), _F32), ((K,), _F32), ((), _I32), ((), _I32))
    if not paired:
        out = _outputs("pose_track", out, lead, heat.device, slots)
        rt.check(rt.lib().hupr_pose_track_assoc_f32(rt.ptr(heat), rows, H, W, float(ratio), int(bool(refine)), rt.ptr(track_state),
                                                    *params, K, sep, floor, rt.ptr(present), group, *map(rt.ptr, out), rt.stream()))
        return out
    group = lead[-1] if lead else 1
    table, swap_cost = check_pair_table(getattr(tracking, "pairs", None), getattr(tracking, "swap_cost", 0.0), group, "pose_track")
    out = _outputs("pose_track", out, lead, heat.device, slots + (((), _I32),))
    rt.check(rt.lib().hupr_pose_track_pairs_f32(rt.ptr(heat), rows, H, W, float(ratio), int(bool(refine)), rt.ptr(track_state), *params,
                                                K, sep, floor, rt.ptr(present), group, (ctypes.c_int * group)(*table), swap_cost,
                                                *map(rt.ptr, out), rt.stream()))
    return out


MEAS_FLOATS = 8                     # pose_measure's record of a row and frame: zx, zy, score, m, Sxx, Sxy, Syy, 0


def pose_measure(heat, ratio, refine=True, out=None):
    """heat (..., H, W) fp32 GPU -> (idx int32 (...), maxval (...), raw keypoints (..., 2), meas (..., 8)) in one launch
    (csrc/pose_fit.hip; the rule is stated beside hupr_pose_measure_f32 in include/hupr.h): the measurement half of ``pose_track``
    without a filter.  The first three are ``pose_decode``'s bits; ``meas`` = (zx, zy, score, m, Sxx, Sxy, Syy, 0) is the raw keypoint,
    the maximum and the mass and second central moments of the tracker's covariance window — everything the tracker reads of a
    frame, so that a recording of it can be run through the filter again under other parameters (``pose_track_nll``).  ``out``: that
    4-tuple, to write (``_outputs``).  Device tensors, no sync."""
    heat, lead, rows, H, W = _pose_heat("pose_measure", heat)
    out = _outputs("pose_measure", out, lead, heat.device, (((), _I32), ((), _F32), ((2,), _F32), ((MEAS_FLOATS,), _F32)))
    rt.check(rt.lib().hupr_pose_measure_f32(rt.ptr(heat), rows, H, W, float(ratio), int(bool(refine)), *map(rt.ptr, out), rt.stream()))
    return out


def check_track_candidates(params, name="pose_track_nll"):
    """Parameter candidates for ``pose_track_nll``: anything ``np.asarray`` turns into (G, 3) numbers = (accel_psd, meas_std,
    heatmap_gain) per candidate, or a tensor (copied to the host) -> a float32 (G, 3) array.  The tracker's rule for the three holds
    for every candidate — accel_psd and heatmap_gain >= 0, meas_std > 0, all finite as fp32 —, else a ValueError in ``name``'s name:
    the library entry takes them as device memory and cannot check."""
    if isinstance(params, torch.Tensor):
        params = params.detach().cpu().numpy()
    try:
        p = np.asarray(params, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s needs (G, 3) candidates (accel_psd, meas_std, heatmap_gain), got %r" % (name, params)) from None
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("%s needs (G, 3) candidates (accel_psd, meas_std, heatmap_gain), got shape %r" % (name, p.shape))
    with np.errstate(over="ignore"):
        p32 = p.astype(np.float32)
    ok = np.isfinite(p32).all(axis=1) & (p32[:, 0] >= 0) & (p32[:, 1] > 0) & (p32[:, 2] >= 0)
    if not ok.all():
        g = int(np.flatnonzero(~ok)[0])
        raise ValueError("%s: candidate %d = (accel_psd %r, meas_std %r, heatmap_gain %r): accel_psd and heatmap_gain must not be "
                         "negative, meas_std must be positive, all finite" % ((name, g) + tuple(p[g].tolist())))
    return p32


def outlier_cost(extent):
    """What a measurement costs the likelihood as an outlier uniform over an image of ``extent`` = (width, height) pixels, in the units
    of d2 + ln det S: 2 ln(width height / 2 pi) — 18.50 at 256 x 256."""
    try:
        w, h = (float(v) for v in extent)
    except (TypeError, ValueError):
        raise ValueError("extent must be (width, height) in image pixels, got %r" % (extent,)) from None
    if not (0 < w < float("inf") and 0 < h < float("inf")):
        raise ValueError("extent must be (width, height) in image pixels, positive and finite, got %r" % (extent,))
    return 2.0 * math.log(w * h / (2.0 * math.pi))


def pose_track_nll(meas, start, tracking, params, extent, ratio):
    """The likelihood of a recording under many tracker parameters, in one launch (csrc/pose_fit.hip; the rule is stated beside
    hupr_pose_track_nll_f32 in include/hupr.h).  ``meas`` (T, ..., 8) fp32 GPU: frame by frame what ``pose_measure`` gave; ``start``
    (T,) int32 or bool on the same device: non-zero where a frame begins a sequence (every track is zeroed in front of it);
    ``tracking`` the parameters all candidates share (``rate_hz``, ``gate``, ``max_coast``, ``init_speed_std``, ``min_score`` are
    read); ``params`` (G, 3) = (accel_psd, meas_std, heatmap_gain) per candidate (``check_track_candidates``: checked on the host,
    before the upload and any launch); ``extent`` = (width, height) of the image in pixels, which prices an outlier
    (``outlier_cost``); ``ratio`` image pixels per heat-map pixel, the one ``pose_measure`` was called with — the moments in ``meas``
    are heat-map pixels squared -> (nll float64 (G, ...): per candidate and row the sum of min(d2 + ln det S, outlier cost) over the
    frames scored; counts int32 (G, ..., 6): the frames per TRACK_* status in code order, then the frames scored; final_state
    (G, ..., 16): the track state after the last frame).  Every thread runs the plain ``pose_track`` frame, so a candidate that
    equals a ``pose_track`` run's parameters ends in that run's state bit for bit.  Device tensors, no sync."""
    if not isinstance(meas, torch.Tensor) or meas.dtype != _F32 or meas.dim() < 2 or meas.shape[-1] != MEAS_FLOATS:
        raise ValueError("pose_track_nll needs meas as a (T, ..., %d) fp32 tensor, got %s" % (MEAS_FLOATS, getattr(meas, "shape", type(meas).__name__)))
    if not meas.is_cuda:
        raise ValueError("pose_track_nll needs GPU tensors (no CPU fallback), got %s" % meas.device)
    if tracking is None:
        raise ValueError("pose_track_nll needs the tracking parameters the candidates share")
    T, lead = int(meas.shape[0]), tuple(meas.shape[1:-1])
    if not isinstance(start, torch.Tensor) or start.dtype not in (_I32, torch.bool) or tuple(start.shape) != (T,):
        raise ValueError("pose_track_nll needs start as a (%d,) int32 or bool tensor, got %s" % (T, getattr(start, "shape", type(start).__name__)))
    if start.device != meas.device:
        raise ValueError("start is on %s, meas on %s" % (start.device, meas.device))
    cand = check_track_candidates(params)
    cost = outlier_cost(extent)
    G, rows, dev = cand.shape[0], int(np.prod(lead, dtype=np.int64)), meas.device
    meas, start = _c(meas), _c(start.to(_I32))
    nll = torch.empty((G,) + lead, dtype=torch.float64, device=dev)
    counts = torch.empty((G,) + lead + (6,), dtype=_I32, device=dev)
    final = torch.empty((G,) + lead + (16,), dtype=_F32, device=dev)
    table = torch.from_numpy(cand).to(dev)
    rt.check(rt.lib().hupr_pose_track_nll_f32(rt.ptr(meas), rt.ptr(start), T, rows, float(ratio), float(tracking.rate_hz),
                                              float(tracking.gate), int(tracking.max_coast), float(tracking.init_speed_std),
                                              float(tracking.min_score), cost, rt.ptr(table), G, rt.ptr(nll), rt.ptr(counts),
                                              rt.ptr(final), rt.stream()))
    return nll, counts, final


SMOOTH_SMOOTHED, SMOOTH_END, SMOOTH_PASSTHROUGH, SMOOTH_DEGENERATE = range(4)                   # pose_smooth_rts's flags


def pose_smooth_rts(states, status, keypoints, tracking):
    """Rauch-Tung-Striebel smoothing of a recorded ``pose_track`` run in one launch (csrc/pose_smooth.hip; the rule is stated beside
    hupr_pose_smooth_rts_f32 in include/hupr.h).  ``states`` (T, ..., 16) fp32: entry k is a copy of the ``track_state`` right after
    the ``pose_track`` call of frame k; ``status`` int32 (T, ...) and ``keypoints`` (T, ..., 2) that call's status and filtered
    keypoints; ``tracking`` the parameters of the run (``rate_hz`` and ``accel_psd`` are read) -> (smoothed keypoints (T, ..., 2),
    velocity (T, ..., 2), position covariance (T, ..., 3) = (Pxx, Pxy, Pyy), flag int32 (T, ...), one of the SMOOTH_* codes).  Device
    tensors, no sync."""
    for name, t, dtype in (("states", states, torch.float32), ("status", status, torch.int32), ("keypoints", keypoints, torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise ValueError("pose_smooth_rts needs %s as a %s tensor, got %s" % (name, dtype, getattr(t, "dtype", type(t).__name__)))
    if tracking is None:
        raise ValueError("pose_smooth_rts needs the tracking parameters of the filter run")
    if status.dim() < 1 or status.shape[0] < 1:
        raise ValueError("pose_smooth_rts needs (T, ...) histories with T >= 1, got status of shape %r" % (tuple(status.shape),))
    lead = tuple(status.shape)
    if tuple(states.shape) != lead + (16,) or tuple(keypoints.shape) != lead + (2,):
        raise ValueError("pose_smooth_rts needs states %r and keypoints %r beside status %r, got %r and %r"
                         % (lead + (16,), lead + (2,), lead, tuple(states.shape), tuple(keypoints.shape)))
    if not (states.device == status.device == keypoints.device):
        raise ValueError("states, status and keypoints are on %s, %s and %s" % (states.device, status.device, keypoints.device))
    if not states.is_cuda:
        raise ValueError("pose_smooth_rts needs GPU tensors (no CPU fallback), got %s" % states.device)
    states, status, keypoints = _c(states), _c(status), _c(keypoints)
    T = lead[0]
    rows = int(np.prod(lead[1:], dtype=np.int64))
    dev = states.device
    smoothed, vel = (torch.empty(lead + (2,), dtype=torch.float32, device=dev) for _ in range(2))
    cov = torch.empty(lead + (3,), dtype=torch.float32, device=dev)
    flag = torch.empty(lead, dtype=torch.int32, device=dev)
    rt.check(rt.lib().hupr_pose_smooth_rts_f32(rt.ptr(states), rt.ptr(status), rt.ptr(keypoints), T, rows, float(tracking.rate_hz),
                                               float(tracking.accel_psd), rt.ptr(smoothed), rt.ptr(vel), rt.ptr(cov), rt.ptr(flag),
                                               rt.stream()))
    return smoothed, vel, cov, flag


SMOOTH_EMPTY = 4                    # pose_smooth_lag's flag of a tail slot whose frame does not exist yet
MAX_LAG = 64


def check_lag(lag, name="pose_smooth_lag"):
    """``lag`` as an int where it is an integer (no bool) in 1..MAX_LAG; otherwise a ValueError in ``name``'s name."""
    if isinstance(lag, bool) or not isinstance(lag, (int, np.integer)) or not 1 <= lag <= MAX_LAG:
        raise ValueError("%s needs an integer lag in 1..%d frames, got %r" % (name, MAX_LAG, lag))
    return int(lag)


def pose_lag_state(rows, lag, device):
    """A zero-filled ("new sequence") state of the fixed-lag smoother for ``rows`` (sample, joint) rows and ``lag`` frames, fp32 and
    opaque: the ring of the last ``lag + 1`` tracker states with their outputs, and a frame counter per row."""
    lag = check_lag(lag, "pose_lag_state")
    return _pose_state(lambda n: rt.lib().hupr_pose_lag_state_bytes(n, lag), rows, device)


def pose_smooth_lag(track_state, status, filtered, raw, scores, lag_state, tracking, lag, out=None):
    """One frame of the fixed-lag Rauch-Tung-Striebel smoother behind ``pose_track``, in one launch (csrc/pose_lag.hip; the rule is
    stated beside hupr_pose_smooth_lag_f32 in include/hupr.h).  ``track_state`` (..., 16) fp32: the tracker's state right after the
    ``pose_track`` call of the frame; ``status`` int32 (...), ``filtered`` (..., 2), ``raw`` (..., 2) and ``scores`` (...): that
    call's status, filtered keypoints, raw keypoints and maxima; ``lag_state`` (``pose_lag_state`` for the same rows and ``lag``,
    advanced in place); ``tracking`` the parameters of the run (``rate_hz`` and ``accel_psd`` are read).  The frame is filed in the
    ring, and the backward pass of ``pose_smooth_rts`` runs over the last ``lag + 1`` frames -> the tail, slot j = the frame j
    frames ago: (keypoints (lag + 1, ..., 2), velocity (lag + 1, ..., 2), position covariance (lag + 1, ..., 3), flag int32
    (lag + 1, ...), one of the SMOOTH_* codes; and the filter's record of the same frames: filtered (lag + 1, ..., 2), raw
    (lag + 1, ..., 2), status int32 (lag + 1, ...), scores (lag + 1, ...)).  Slot ``lag`` is the fixed-lag answer; a slot whose
    frame does not exist yet holds zeros and SMOOTH_EMPTY.  ``out``: that 8-tuple, to write (``_outputs``).  Device tensors, no
    sync."""
    lag = check_lag(lag)
    for name, t, dtype in (("track_state", track_state, _F32), ("status", status, _I32), ("filtered", filtered, _F32), ("raw", raw, _F32),
                           ("scores", scores, _F32), ("lag_state", lag_state, _F32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise ValueError("pose_smooth_lag needs %s as a %s tensor, got %s" % (name, dtype, getattr(t, "dtype", type(t).__name__)))
    if tracking is None:
        raise ValueError("pose_smooth_lag needs the tracking parameters of the filter run")
    lead = tuple(status.shape)
    rows = int(np.prod(lead, dtype=np.int64))
    if (track_state.numel() != rows * 16 or (rows and track_state.shape[-1] != 16) or tuple(filtered.shape) != lead + (2,)
            or tuple(raw.shape) != lead + (2,) or tuple(scores.shape) != lead):
        raise ValueError("pose_smooth_lag needs the %d x 16 track_state, filtered %r, raw %r and scores %r beside status %r, got %r, %r, "
                         "%r and %r" % (rows, lead + (2,), lead + (2,), lead, lead, tuple(track_state.shape), tuple(filtered.shape),
                                        tuple(raw.shape), tuple(scores.shape)))
    for name, t in (("track_state", track_state), ("filtered", filtered), ("raw", raw), ("scores", scores), ("lag_state", lag_state)):
        if t.device != status.device:
            raise ValueError("%s is on %s, status on %s" % (name, t.device, status.device))
    if not status.is_cuda:
        raise ValueError("pose_smooth_lag needs GPU tensors (no CPU fallback), got %s" % status.device)
    if not lag_state.is_contiguous() or lag_state.numel() * 4 != int(rt.lib().hupr_pose_lag_state_bytes(rows, lag)):
        raise ValueError("lag_state must be the fp32 tensor pose_lag_state(%d, %d, device) returns" % (rows, lag))
    track_state, status, filtered, raw, scores = _c(track_state), _c(status), _c(filtered), _c(raw), _c(scores)
    xy, scalar = ((2,), _F32), ((), _F32)
    out = _outputs("pose_smooth_lag", out, (lag + 1,) + lead, status.device, (xy, xy, ((3,), _F32), ((), _I32), xy, xy, ((), _I32), scalar))
    rt.check(rt.lib().hupr_pose_smooth_lag_f32(rt.ptr(track_state), rt.ptr(status), rt.ptr(filtered), rt.ptr(raw), rt.ptr(scores), rows, lag,
                                               float(tracking.rate_hz), float(tracking.accel_psd), rt.ptr(lag_state), *map(rt.ptr, out),
                                               rt.stream()))
    return out


# ---- scene occupancy: CA-CFAR detection on the mean planes, presence gate (csrc/cfar.hip) -----------------------------------------------
CFAR_SUMMARY = ("count", "peak_snr", "peak_f", "peak_r", "peak_a", "centroid_r", "centroid_a", "doppler")


class CfarResult:
    """What ``cfar_ra`` returns.  ``summary`` (..., 8) fp32, the fields of ``CFAR_SUMMARY`` (also as attributes: ``result.count`` is
    ``summary[..., 0]``); ``mask`` uint8 and ``snr`` fp32, (..., 8, 64, 64) each, None unless asked for; ``pfa``, ``guard``, ``train``
    the settings of the run.  Device tensors."""
    __slots__ = ("summary", "mask", "snr", "pfa", "guard", "train")

    def __init__(self, summary, mask, snr, pfa, guard, train):
        self.summary, self.mask, self.snr, self.pfa, self.guard, self.train = summary, mask, snr, pfa, guard, train

    def __getattr__(self, name):
        if name in CFAR_SUMMARY:
            return self.summary[..., CFAR_SUMMARY.index(name)]
        raise AttributeError(name)


_CFAR_TABLES = {}


def cfar_table(pfa, guard, train, device):
    """The fp32 device copy of ``preprocessing.cfar_alpha_table(pfa, guard, train)``, uploaded once per setting and device."""
    from .preprocessing.cfar import cfar_alpha_table, check_cfar
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = check_cfar(pfa, guard, train) + (device,)
    if key not in _CFAR_TABLES:
        _CFAR_TABLES[key] = torch.from_numpy(cfar_alpha_table(*key[:3]).astype(np.float32)).to(device)
    return _CFAR_TABLES[key]


def cfar_ra(planes, pfa=1e-5, guard=2, train=4, want_mask=True, want_snr=False):
    """CA-CFAR detection on the (range, azimuth) maps of the seven moving Doppler slots of ``planes`` (..., 16, 64, 64) fp32 GPU, the
    elevation-mean planes of ``preprocessing.fft_chain_loader_means`` -> ``CfarResult`` in one launch (csrc/cfar.hip; the rule is
    stated beside hupr_cfar_ra_f32 in include/hupr.h).  Device tensors, no sync."""
    from .preprocessing.cfar import check_cfar
    pfa, guard, train = check_cfar(pfa, guard, train)
    if not isinstance(planes, torch.Tensor) or planes.dtype != torch.float32 or planes.dim() < 3 or tuple(planes.shape[-3:]) != (16, 64, 64):
        raise ValueError("cfar_ra needs fp32 planes (..., 16, 64, 64), got %s %r" % (getattr(planes, "dtype", type(planes).__name__),
                                                                                   tuple(getattr(planes, "shape", ()))))
    if not planes.is_cuda:
        raise rt.HuprError("cfar_ra needs GPU planes (no CPU fallback), got %s" % planes.device)
    planes = _c(planes)
    lead = tuple(planes.shape[:-3])
    n = int(np.prod(lead, dtype=np.int64))
    dev = planes.device
    with torch.cuda.device(dev):
        table = cfar_table(pfa, guard, train, dev)
        summary = torch.empty(lead + (8,), dtype=torch.float32, device=dev)
        mask = torch.empty(lead + (8, 64, 64), dtype=torch.uint8, device=dev) if want_mask else None
        snr = torch.empty(lead + (8, 64, 64), dtype=torch.float32, device=dev) if want_snr else None
        rt.check(rt.lib().hupr_cfar_ra_f32(rt.ptr(planes), n, guard, train, rt.ptr(table), table.numel(), rt.ptr(mask), rt.ptr(snr),
                                           rt.ptr(summary), rt.stream()))
    return CfarResult(summary, mask, snr, pfa, guard, train)


def presence_state(lanes, device):
    """A zeroed presence-gate state: int32 (lanes, 4) = (present, hits, misses, frames)."""
    return torch.zeros((lanes, 4), dtype=torch.int32, device=device)


def presence_update(summary, gate_state, min_cells=3, confirm=2, hold=20, out=None):
    """One frame of the presence gate (hupr_presence_update in include/hupr.h): ``summary`` (lanes, 8) fp32 of ``cfar_ra``,
    ``gate_state`` (``presence_state``, advanced in place) -> present int32 (lanes,), ``out`` if given.  Device tensors, no sync."""
    if summary.dtype != torch.float32 or summary.dim() != 2 or summary.shape[1] != 8:
        raise ValueError("presence_update needs the (lanes, 8) fp32 summary of cfar_ra, got %s %r" % (summary.dtype, tuple(summary.shape)))
    lanes = summary.shape[0]
    if gate_state.dtype != torch.int32 or tuple(gate_state.shape) != (lanes, 4) or gate_state.device != summary.device:
        raise ValueError("gate_state must be the int32 tensor presence_state(%d, device) returns" % lanes)
    present, = _outputs("presence_update", None if out is None else (out,), (lanes,), summary.device, (((), _I32),))
    with torch.cuda.device(summary.device):
        rt.check(rt.lib().hupr_presence_update(rt.ptr(_c(summary)), lanes, int(min_cells), int(confirm), int(hold), rt.ptr(gate_state),
                                               rt.ptr(present), rt.stream()))
    return present


# ---- interference blanking of the raw ADC cube in front of the FFT chain (csrc/interference.hip) ----------------------------------------
class InterferenceStats:
    """The counts ``adc_interference`` returns: ``frames`` int32 (n, 2) = (samples replaced, chirps touched) per sensor-frame, the sums
    of ``groups`` int32 (n, 12, 2), the same pair per (rx, tx) group, index 3 rx + tx.  Device tensors."""
    __slots__ = ("frames", "groups")

    def __init__(self, frames, groups):
        self.frames, self.groups = frames, groups


def adc_interference(adc, K=32, guard=2, fill="clutter", out=None, want_mask=False, stats=None):
    """Time-domain interference detection and blanking on int16 GPU cubes ``adc`` (n, 4, 192, 256, 2), in two launches (the rule is
    stated beside hupr_adc_interference_i16 in include/hupr.h) -> ``(cube, stats, mask)``: the filtered cube (``out``: a tensor like
    ``adc`` to write, ``adc`` itself for in place, None for a new one), an ``InterferenceStats`` (``stats``: one to reuse) and the bit mask
    uint8 (n, 4, 192, 32) of the replaced samples (bit ``s % 8`` of byte ``s / 8``; None unless ``want_mask``).  Device tensors, no sync."""
    from .preprocessing.interference import FILLS, check_interference
    K, guard, fill = check_interference(K, guard, fill)
    if not isinstance(adc, torch.Tensor) or adc.dtype != torch.int16 or adc.dim() != 5 or tuple(adc.shape[1:]) != (4, 192, 256, 2):
        raise ValueError("adc must be int16 (n,4,192,256,2), got %s %r" % (getattr(adc, "dtype", type(adc).__name__),
                                                                           tuple(getattr(adc, "shape", ()))))
    if stats is not None and not isinstance(stats, InterferenceStats):
        raise ValueError("stats must be an InterferenceStats or None, got %s" % type(stats).__name__)
    n, dev = adc.shape[0], adc.device
    out, = _outputs("adc_interference", None if out is None else (out,), (n,), dev, (((4, 192, 256, 2), torch.int16),))
    frames, groups = _outputs("adc_interference: stats", stats and (stats.frames, stats.groups), (n,), dev, (((2,), _I32), ((12, 2), _I32)))
    if not adc.is_cuda:
        raise rt.HuprError("adc_interference needs GPU cubes (no CPU fallback), got %s" % adc.device)
    with torch.cuda.device(dev):
        mask = torch.empty((n, 4, 192, 32), dtype=torch.uint8, device=dev) if want_mask else None
        rt.check(rt.lib().hupr_adc_interference_i16(rt.ptr(adc), rt.ptr(out), n, K, guard, FILLS[fill], rt.ptr(mask), rt.ptr(groups), rt.stream()))
        rt.check(rt.lib().hupr_adc_interference_stats(rt.ptr(groups), n, rt.ptr(frames), rt.stream()))
    return out, stats or InterferenceStats(frames, groups), mask


# ---- radar scene simulator: moving scatterers -> the raw ADC cube of one sensor (csrc/radar_scene.hip) ------------------------------------
def _host_f64(name, a, shape):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    if a.shape != shape:
        raise ValueError("radar_scene: %s must have shape %r, got %r" % (name, shape, a.shape))
    return a


def radar_scene(pos, vel, amp, tx, rx, wavelength, range_bin_m, chirp_period_s, add=None, out_dtype=torch.int16):
    """The raw ADC cube of one sensor for ``frames`` frames of S moving point scatterers, in one launch (the model and its arithmetic
    are stated beside hupr_radar_scene_i16 in include/hupr.h).  ``pos``, ``vel``: fp64 GPU tensors (frames, S, 3), metres and metres
    per second at the start of each frame's burst; ``amp``: fp32 (frames, S), 0 or NaN hides a scatterer for that frame; ``tx`` (3, 3)
    and ``rx`` (4, 3): the antenna positions, anything ``np.asarray`` takes (they travel with the launch); ``add``: fp32
    (frames, 4, 192, 256, 2) added to the sums, or None.  -> (frames, 4, 192, 256, 2), int16 (rounded to nearest even, clipped) or, with
    ``out_dtype=torch.float32``, the fp32 sums.  Device tensor, no sync."""
    if out_dtype not in (torch.int16, torch.float32):
        raise ValueError("radar_scene: out_dtype must be torch.int16 or torch.float32, got %r" % (out_dtype,))
    for name, t, dt in (("pos", pos, torch.float64), ("vel", vel, torch.float64), ("amp", amp, torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError("radar_scene: %s must be a %s tensor, got %s" % (name, dt, getattr(t, "dtype", type(t).__name__)))
    if pos.dim() != 3 or pos.shape[2] != 3 or pos.shape[1] < 1 or vel.shape != pos.shape or tuple(amp.shape) != tuple(pos.shape[:2]):
        raise ValueError("radar_scene: pos and vel must be (frames, S >= 1, 3) and amp (frames, S), got %r, %r, %r"
                         % (tuple(pos.shape), tuple(vel.shape), tuple(amp.shape)))
    frames, S = int(pos.shape[0]), int(pos.shape[1])
    cube = (frames, 4, 192, 256, 2)
    if add is not None and (not isinstance(add, torch.Tensor) or add.dtype != torch.float32 or tuple(add.shape) != cube):
        raise ValueError("radar_scene: add must be an fp32 tensor %r or None, got %s %r"
                         % (cube, getattr(add, "dtype", type(add).__name__), tuple(getattr(add, "shape", ()))))
    txh, rxh = _host_f64("tx", tx, (3, 3)), _host_f64("rx", rx, (4, 3))
    if not pos.is_cuda:
        raise rt.HuprError("radar_scene needs GPU tensors (no CPU fallback), got %s" % pos.device)
    for name, t in (("vel", vel), ("amp", amp), ("add", add)):
        if t is not None and t.device != pos.device:
            raise ValueError("radar_scene: %s is on %s, pos on %s" % (name, t.device, pos.device))
    f64p = ctypes.POINTER(ctypes.c_double)
    with torch.cuda.device(pos.device):
        out = torch.empty(cube, dtype=out_dtype, device=pos.device)
        fn = rt.lib().hupr_radar_scene_i16 if out_dtype == torch.int16 else rt.lib().hupr_radar_scene_f32
        rt.check(fn(rt.ptr(_c(pos)), rt.ptr(_c(vel)), rt.ptr(_c(amp)), txh.ctypes.data_as(f64p), rxh.ctypes.data_as(f64p), frames, S,
                    float(wavelength), float(range_bin_m), float(chirp_period_s), rt.ptr(None if add is None else _c(add)), rt.ptr(out),
                    rt.stream()))
    return out


# ---- radar point cloud: CFAR peaks to sub-cell points, two sensors fused to metres (csrc/radar_points.hip) -------------------------------
PEAK_FIELDS = ("range", "azimuth", "doppler", "power", "snr", "cell")
CLOUD_FIELDS = ("x", "y", "z", "velocity", "snr_h", "snr_v", "row_h", "row_v")


class RadarPeaks:
    """What ``radar_peaks`` returns.  ``points`` (..., max_points, 6) fp32, the fields of ``PEAK_FIELDS`` (also as attributes:
    ``result.range`` is ``points[..., 0]``), sorted by descending power, unused rows (0, 0, 0, 0, 0, -1); ``counts`` int32 (..., 2) =
    (points written, peaks found), also ``result.count`` and ``result.found``; ``max_points``, ``sep_range``, ``sep_azimuth`` the
    settings of the run.  Device tensors."""
    __slots__ = ("points", "counts", "max_points", "sep_range", "sep_azimuth")

    def __init__(self, points, counts, max_points, sep_range, sep_azimuth):
        self.points, self.counts, self.max_points, self.sep_range, self.sep_azimuth = points, counts, max_points, sep_range, sep_azimuth

    def __getattr__(self, name):
        if name in PEAK_FIELDS:
            return self.points[..., PEAK_FIELDS.index(name)]
        if name in ("count", "found"):
            return self.counts[..., ("count", "found").index(name)]
        raise AttributeError(name)


class RadarCloud:
    """What ``radar_points_fuse`` returns.  ``cloud`` (..., max_points, 8) fp32, the fields of ``CLOUD_FIELDS`` (also as attributes;
    ``xyz`` is ``cloud[..., :3]``): metres, metres per second (receding positive), both sensors' SNR and the rows of the two points in
    their lists; unused rows (0, 0, 0, 0, 0, 0, -1, -1).  ``counts`` int32 (...,): the points of each frame.  ``peaks_h``, ``peaks_v``:
    the ``RadarPeaks`` it was made of.  Device tensors."""
    __slots__ = ("cloud", "counts", "peaks_h", "peaks_v")

    def __init__(self, cloud, counts, peaks_h, peaks_v):
        self.cloud, self.counts, self.peaks_h, self.peaks_v = cloud, counts, peaks_h, peaks_v

    def __getattr__(self, name):
        if name in CLOUD_FIELDS:
            return self.cloud[..., CLOUD_FIELDS.index(name)]
        if name == "xyz":
            return self.cloud[..., :3]
        raise AttributeError(name)


def radar_peaks(planes, mask, snr=None, max_points=64, sep_range=1, sep_azimuth=4):
    """The detections of ``cfar_ra`` thinned to local power maxima and refined to sub-cell points, one launch (csrc/radar_points.hip; the
    rule is stated beside hupr_radar_peaks_f32 in include/hupr.h).  ``planes`` (..., 16, 64, 64) fp32 GPU, ``mask`` uint8 and ``snr``
    fp32 or None, (..., 8, 64, 64) each -> ``RadarPeaks``.  Device tensors, no sync."""
    from .preprocessing.points import check_points
    s = check_points(max_points=max_points, sep_range=sep_range, sep_azimuth=sep_azimuth)
    max_points, sep_range, sep_azimuth = s["max_points"], s["sep_range"], s["sep_azimuth"]
    if not isinstance(planes, torch.Tensor) or planes.dtype != torch.float32 or planes.dim() < 3 or tuple(planes.shape[-3:]) != (16, 64, 64):
        raise ValueError("radar_peaks needs fp32 planes (..., 16, 64, 64), got %s %r" % (getattr(planes, "dtype", type(planes).__name__),
                                                                                       tuple(getattr(planes, "shape", ()))))
    lead = tuple(planes.shape[:-3])
    for name, t, dt in (("mask", mask, torch.uint8), ("snr", snr, torch.float32)):
        if t is None and name == "snr":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != lead + (8, 64, 64):
            raise ValueError("radar_peaks needs a %s %s %r, got %s %r" % (dt, name, lead + (8, 64, 64), getattr(t, "dtype", type(t).__name__),
                                                                          tuple(getattr(t, "shape", ()))))
    if not planes.is_cuda:
        raise rt.HuprError("radar_peaks needs GPU planes (no CPU fallback), got %s" % planes.device)
    for name, t in (("mask", mask), ("snr", snr)):
        if t is not None and t.device != planes.device:
            raise ValueError("radar_peaks: %s is on %s, planes on %s" % (name, t.device, planes.device))
    n, dev = int(np.prod(lead, dtype=np.int64)), planes.device
    with torch.cuda.device(dev):
        points = torch.empty(lead + (max_points, 6), dtype=torch.float32, device=dev)
        counts = torch.empty(lead + (2,), dtype=torch.int32, device=dev)
        rt.check(rt.lib().hupr_radar_peaks_f32(rt.ptr(_c(planes)), rt.ptr(_c(mask)), rt.ptr(None if snr is None else _c(snr)), n, max_points,
                                               sep_range, sep_azimuth, rt.ptr(points), rt.ptr(counts), rt.stream()))
    return RadarPeaks(points, counts, max_points, sep_range, sep_azimuth)


def radar_points_fuse(peaks_h, peaks_v, geometry, range_gate=1.5, doppler_gate=1):
    """The two sensors' points of the same frames paired and turned into metres, one launch (the rule is stated beside
    hupr_radar_points_fuse_f32 in include/hupr.h).  ``peaks_h``, ``peaks_v``: the ``RadarPeaks`` of the horizontal and the vertical sensor;
    ``geometry``: ``preprocessing.points.radar_geometry(model)`` = (range_bin_m, doppler_mps_per_bin, a_h, o_h, a_v, o_v) -> ``RadarCloud``
    with as many rows as ``peaks_h``.  Device tensors, no sync."""
    from .preprocessing.points import check_points, geometry_vector
    s = check_points(range_gate=range_gate, doppler_gate=doppler_gate)
    geo = geometry_vector(geometry)
    for name, p in (("peaks_h", peaks_h), ("peaks_v", peaks_v)):
        if not isinstance(p, RadarPeaks):
            raise ValueError("radar_points_fuse: %s must be a RadarPeaks, got %s" % (name, type(p).__name__))
    lead = tuple(peaks_h.counts.shape[:-1])
    if tuple(peaks_v.counts.shape[:-1]) != lead:
        raise ValueError("radar_points_fuse: the sensors' frames differ: %r and %r" % (lead, tuple(peaks_v.counts.shape[:-1])))
    if not peaks_h.points.is_cuda:
        raise rt.HuprError("radar_points_fuse needs GPU points (no CPU fallback), got %s" % peaks_h.points.device)
    dev = peaks_h.points.device
    if peaks_v.points.device != dev:
        raise ValueError("radar_points_fuse: peaks_v is on %s, peaks_h on %s" % (peaks_v.points.device, dev))
    n, mh, mv = int(np.prod(lead, dtype=np.int64)), int(peaks_h.points.shape[-2]), int(peaks_v.points.shape[-2])
    with torch.cuda.device(dev):
        cloud = torch.empty(lead + (mh, 8), dtype=torch.float32, device=dev)
        counts = torch.empty(lead, dtype=torch.int32, device=dev)
        rt.check(rt.lib().hupr_radar_points_fuse_f32(rt.ptr(_c(peaks_h.points)), rt.ptr(_c(peaks_h.counts)), mh, rt.ptr(_c(peaks_v.points)),
                                                     rt.ptr(_c(peaks_v.counts)), mv, n, geo.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                     s["range_gate"], s["doppler_gate"], rt.ptr(cloud), rt.ptr(counts), rt.stream()))
    return RadarCloud(cloud, counts, peaks_h, peaks_v)
