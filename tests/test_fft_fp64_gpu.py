"""GPU (-m gpu): every form of the FFT chain (csrc/fft_chain.hip: hupr_k_range_doppler<0..3>, hupr_k_doppler_range<0..3, HALF>,
hupr_k_angle<0..3> plain and TDM, hupr_k_loader_normalize — 21 instantiations) against the fp64 answer of that form
(tests/fft_ref.py), element by element, with its launches counted.  tests/test_fft_route.py holds the table below to the compiled
instantiations and proves on the CPU that the gate rejects subtly wrong results.

Gate, per element, no term relative to the output.  A = the L2 norm of the frame's raw int16 samples times the form's window weights
(fft_ref.frame_scale; at a dithered zero-Doppler index: the L2 norm of the dither's input), s = the fp64 unbiased std of the reference
plane:
  cube               |out - ref|       <= c A
  magnitude          ||out| - |ref||   <= c A + 2^-23 |ref|
  loader             |n - n_ref|       <= c_L (A / s) (1 + |n_ref|)
  means              |m - m_ref|       <= the loader bound averaged over the eight elevation planes
  loader_normalize   the loader bound, against the fp64 Normalize of the very complex64 cube the kernel reads
The zero-Doppler index takes the gate of its own reference (fft_ref.zero_rule): the dither against its restatement; "exact" as bound
0 (s = 0: the output must be exactly zero); range-first without the Doppler window against ref = 0 (some non-zero value), its loader
slot f = 4 only finite with unit variance (the normalised residue of another arithmetic is nothing to compare with).

Constants (GATE_C): per group and family the smallest power of two >= 8 x the worst ratio measured over this table on an MI355X
(8 x: room for another butterfly order), capped at 2^-15 — the largest power of two that keeps this gate tighter than the
2e-5 max|ref| of tests/test_fft_gpu.py (2^-14.0 A on seeds 0..2).  Measured worst err / bound-at-c-=-1, as log2:
  group              Doppler-first (df)                      range-first (rf)                      TDM (tdm)
  cube               -19.0024 (W 3, impulses)    c = 2^-16   -20.34 (W 1, noise)       c = 2^-17   -18.8976 (W 3, impulses)  c = 2^-15
  magnitude          -20.80 (W 3, noise)         c = 2^-17   -20.66 (W 3, noise)       c = 2^-17   -20.57 (W 3, noise)       c = 2^-17
  loader             -20.86 (W 0, coherent)      c = 2^-17   -20.98 (W 0, coherent)    c = 2^-17   -20.59 (W 0, coherent)    c = 2^-17
  means              -22.25 (W 1, noise)         c = 2^-19   -22.16 (W 3, noise)       c = 2^-19   -22.23 (W 3, noise)       c = 2^-19
  loader_normalize   -23.51                      c = 2^-20
On noise every cube form sits at -20.2 .. -20.6.  The windowed impulse frames are the worst cube inputs because A is not mean-removed:
the one sample has the weight hann64[5] hann256[37] = 0.012, while the mean that clutter removal spreads over the other 63 chirp loops
is windowed with weights up to 1 — the output, and its rounding, are several times A there.  ``clutter`` (20 000 LSB static, 50 LSB
target): Doppler-first -23.61 under W = 3 and -21.35 under W = 1 against the range-first order's -20.40 under W = 3 — the exact
cancellation the Doppler-first design claims; with W = 0 the range-first order reaches -22.83.

Every call: the output is a view 16-byte aligned inside a NaN-pattern buffer with guards on both sides; the workspace is exactly
hupr_fft_chain_ws_bytes(n_sf) bytes, NaN-filled before every call (the HALF form of K1 leaves rows 0..3 and 12..15 unwritten: a
K2 that read them would show it), guards on both sides; the ADC cube sits between two full-scale int16 tails; afterwards every
guard and the ADC buffer are bit-identical, no output element holds the pattern or a non-finite value, the unwritten rows of a HALF
workspace still hold the pattern, and a second launch into fresh buffers gives the same bits.  hupr_launch_count rises by exactly 2
per chain call, 1 per hupr_loader_normalize_c64, 0 for n_sf = 0 and for every refused call.

The zero-Doppler rule under a window (include/hupr.h).  These cases found hupr_k_doppler_range applying both conventions under
WIN == 0 only: with HUPR_FFT_HANN_RANGE alone index 8 held the fp32 residue of sum_c fl((x_c - mean) w) — on the noise frames up to
6.7e-2 where the dither is 4.5e-10, and under HUPR_FFT_ZERO_DOPPLER_EXACT a normalised noise channel (|n| up to 4.5) in loader slot 4
where the header promises zeros.  The kernel now gives bin 0 the W = 0 treatment whenever the Doppler window is off (64 * mean is the
exact chirp sum); against the build before it, every W = 0, 2, 3 form and every other index of the W = 1 forms kept its bits.  The
W = 1 cases below (dither: bit-identical with W = 0's index 8; exact: zeros) pin the rule."""
import collections
import functools

import numpy as np
import pytest
import torch

import fft_ref
from fft_ref import Form
from test_conv_halo_fp64_gpu import GUARD, NAN32, bits, nan_buffer

pytestmark = pytest.mark.gpu

HUPR_ERR_ARG, HUPR_ERR_WORKSPACE = -1, -2
HANN_RANGE, HANN_DOPPLER, MAGNITUDE, ZERO_DOPPLER_EXACT, RANGE_FIRST = 1, 2, 4, 8, 16      # include/hupr.h HUPR_FFT_*
CAP = 2.0 ** -15


# ---- the case table ------------------------------------------------------------------------------------------------------------------
def DR(W, half):
    return ("doppler_range", W, half)


def RD(W):
    return ("range_doppler", W)


def AN(mode, tdm=False):
    return ("angle", mode, tdm)


LN = ("loader_normalize",)
# conv: the order / zero-Doppler convention; out: cube / magnitude / loader / means; inputs: names of INPUTS; k1, k2: the two
# instantiations the call launches (tests/test_fft_route.py holds them to the dispatch and to the build)
Case = collections.namedtuple("Case", "conv window out tdm inputs k1 k2")
CASES = [
    # Doppler-first, the default convention: W 0..3 x cube / magnitude / loader / means
    Case("dither", 0, "cube", False, "noise impulses clutter full_scale", DR(0, False), AN(0)),
    Case("dither", 1, "cube", False, "noise clutter", DR(1, False), AN(0)),
    Case("dither", 2, "cube", False, "noise", DR(2, False), AN(0)),
    Case("dither", 3, "cube", False, "noise impulses clutter full_scale", DR(3, False), AN(0)),
    Case("dither", 0, "magnitude", False, "noise impulses", DR(0, False), AN(2)),
    Case("dither", 1, "magnitude", False, "noise", DR(1, False), AN(2)),
    Case("dither", 2, "magnitude", False, "noise", DR(2, False), AN(2)),
    Case("dither", 3, "magnitude", False, "noise", DR(3, False), AN(2)),
    Case("dither", 0, "loader", False, "noise impulses clutter coherent", DR(0, True), AN(1)),
    Case("dither", 1, "loader", False, "noise", DR(1, True), AN(1)),
    Case("dither", 2, "loader", False, "noise", DR(2, True), AN(1)),
    Case("dither", 3, "loader", False, "noise coherent", DR(3, True), AN(1)),
    Case("dither", 0, "means", False, "noise impulses coherent", DR(0, True), AN(3)),
    Case("dither", 1, "means", False, "noise", DR(1, True), AN(3)),
    Case("dither", 2, "means", False, "noise", DR(2, True), AN(3)),
    Case("dither", 3, "means", False, "noise", DR(3, True), AN(3)),
    # HUPR_FFT_ZERO_DOPPLER_EXACT: W 0, 1 x cube / loader / means
    Case("exact", 0, "cube", False, "noise", DR(0, False), AN(0)),
    Case("exact", 1, "cube", False, "noise", DR(1, False), AN(0)),
    Case("exact", 0, "loader", False, "noise", DR(0, True), AN(1)),
    Case("exact", 1, "loader", False, "noise", DR(1, True), AN(1)),
    Case("exact", 0, "means", False, "noise", DR(0, True), AN(3)),
    Case("exact", 1, "means", False, "noise", DR(1, True), AN(3)),
    # the range-first order: W 0..3 x cube, W 0, 3 x magnitude / loader / means
    Case("range_first", 0, "cube", False, "noise impulses clutter", RD(0), AN(0)),
    Case("range_first", 1, "cube", False, "noise", RD(1), AN(0)),
    Case("range_first", 2, "cube", False, "noise", RD(2), AN(0)),
    Case("range_first", 3, "cube", False, "noise clutter", RD(3), AN(0)),
    Case("range_first", 0, "magnitude", False, "noise", RD(0), AN(2)),
    Case("range_first", 3, "magnitude", False, "noise", RD(3), AN(2)),
    Case("range_first", 0, "loader", False, "noise clutter coherent", RD(0), AN(1)),
    Case("range_first", 3, "loader", False, "noise", RD(3), AN(1)),
    Case("range_first", 0, "means", False, "noise", RD(0), AN(3)),
    Case("range_first", 3, "means", False, "noise", RD(3), AN(3)),
    # TDM compensation with the swap table [1, 0]: W 0..3 x cube, W 0, 3 x magnitude / loader / means
    Case("dither", 0, "cube", True, "noise impulses", DR(0, False), AN(0, True)),
    Case("dither", 1, "cube", True, "noise", DR(1, False), AN(0, True)),
    Case("dither", 2, "cube", True, "noise", DR(2, False), AN(0, True)),
    Case("dither", 3, "cube", True, "noise impulses", DR(3, False), AN(0, True)),
    Case("dither", 0, "magnitude", True, "noise", DR(0, False), AN(2, True)),
    Case("dither", 3, "magnitude", True, "noise", DR(3, False), AN(2, True)),
    Case("dither", 0, "loader", True, "noise impulses coherent", DR(0, True), AN(1, True)),
    Case("dither", 3, "loader", True, "noise", DR(3, True), AN(1, True)),
    Case("dither", 0, "means", True, "noise coherent", DR(0, True), AN(3, True)),
    Case("dither", 3, "means", True, "noise", DR(3, True), AN(3, True)),
]
LOADER_CODE = {"cube": 0, "magnitude": 0, "loader": 1, "means": 2}
SWAP_FLAGS = (1, 0)                          # the table of tests/test_tdm_gpu.py


def case_id(c):
    return "%s%s-W%d-%s" % ("tdm-" if c.tdm else "", c.conv, c.window, c.out)


def form_of(c):
    return Form(c.window, c.conv, LOADER_CODE[c.out], c.out == "magnitude", c.tdm)


def flags_of(c):
    return c.window | (MAGNITUDE if c.out == "magnitude" else 0) | {"dither": 0, "exact": ZERO_DOPPLER_EXACT, "range_first": RANGE_FIRST}[c.conv]


def family(c):
    return "tdm" if c.tdm else "rf" if c.conv == "range_first" else "df"


def frames_per_flag(n):
    """noise: frames 0, 1 swapped, 2 not; impulses: the receivers 0, 1 swapped, 2, 3 not; a single frame: swapped."""
    return {1: 1, 3: 2, 12: 6}[n]


def swapped(c, n, k):
    g = k // frames_per_flag(n)
    return bool(c.tdm and g < len(SWAP_FLAGS) and SWAP_FLAGS[g])


# ---- the gate (CPU, numpy) -----------------------------------------------------------------------------------------------------------
# group -> family -> c: the smallest power of two >= 8 x the measured worst ratio (the module docstring), at most CAP
GATE_C = {
    "cube": {"df": 2.0 ** -16, "rf": 2.0 ** -17, "tdm": 2.0 ** -15},
    "magnitude": {"df": 2.0 ** -17, "rf": 2.0 ** -17, "tdm": 2.0 ** -17},
    "loader": {"df": 2.0 ** -17, "rf": 2.0 ** -17, "tdm": 2.0 ** -17},
    "means": {"df": 2.0 ** -19, "rf": 2.0 ** -19, "tdm": 2.0 ** -19},
    "loader_normalize": {"df": 2.0 ** -20},
}
assert all(v <= CAP for g in GATE_C.values() for v in g.values())


def residue_slot(form):
    """True where loader slot f = 4 is the normalised rounding residue of the range-first order: nothing to compare it with."""
    return bool(form.loader) and form.convention == "range_first" and not form.window & 2


def loader_bound(ans, c):
    """(8, 2, 64, 64, 8): c (A / s) (1 + |n_ref|); an exactly-zero reference plane (s = 0) has the bound 0."""
    s = ans.std
    ratio = np.divide(ans.scale[4:12, None, None], s, out=np.zeros_like(s), where=s > 0)
    return c * ratio[:, :, None, None, :] * (1.0 + np.abs(ans.ld))


def bound(ans, form, c):
    """The gate's right-hand side, in the layout of ans.ref."""
    if form.loader == 0:
        b = c * np.broadcast_to(ans.scale[:, None, None, None], ans.ref.shape)
        return b + 2.0 ** -23 * ans.ref if form.magnitude else b
    lb = loader_bound(ans, c)
    return lb if form.loader == 1 else lb.mean(axis=-1).reshape(16, 64, 64)


def gated(ans, form):
    """Boolean mask in the layout of ans.ref: every element but the residue slot."""
    m = np.ones(ans.ref.shape, dtype=bool)
    if residue_slot(form):
        if form.loader == 1:
            m[4] = False
        else:
            m[8:10] = False
    return m


def error(out, ans, form):
    out = np.asarray(out)
    return np.abs(out.astype(np.complex128 if np.iscomplexobj(out) else np.float64) - ans.ref)


def within(out, ans, form, c):
    """True where ``out`` meets the gate of ``form`` (a NaN never does; the residue slot always does)."""
    return (error(out, ans, form) <= bound(ans, form, c)) | ~gated(ans, form)


def measured(out, ans, form):
    """The smallest c at which ``out`` would pass: the worst err / bound-at-c-=-1 over the gated elements whose bound is not 0."""
    err, m = error(out, ans, form), gated(ans, form)
    if form.magnitude:
        err = np.maximum(err - 2.0 ** -23 * ans.ref, 0.0)
    b1 = bound(ans, Form(form.window, form.convention, form.loader, False, form.tdm), 1.0)
    m = m & (b1 > 0)
    return float((err[m] / b1[m]).max()) if m.any() else 0.0


def group_of(c):
    return c.out


def assert_within(out, ans, form, c, what):
    ok = within(out, ans, form, c)
    if not bool(ok.all()):
        bad = np.argwhere(~ok)
        raise AssertionError("%s: %d of %d outside the gate, first at %s (out %r, ref %r), measured c = 2^%.2f against 2^%.2f"
                             % (what, len(bad), ok.size, tuple(bad[0]), np.asarray(out)[tuple(bad[0])], ans.ref[tuple(bad[0])],
                                np.log2(max(measured(out, ans, form), 1e-300)), np.log2(c)))


# ---- inputs (host, int16 (n, 4, 192, 256, 2), made once) --------------------------------------------------------------------------------
IMPULSE = (5, 37, 1000, 700)                 # chirp loop, sample, I, Q


def _noise():
    from hupr_amd import synth
    return np.concatenate([synth.adc_cube_int16(s) for s in (0, 1, 2)])


def _impulses():
    """Twelve frames, frame k = 3 rx + tx: one non-zero sample, on receiver rx in the chirp of transmitter tx of loop 5."""
    loop, s, i, q = IMPULSE
    out = np.zeros((12, 4, 192, 256, 2), dtype=np.int16)
    for k in range(12):
        out[k, k // 3, 3 * loop + k % 3, s] = (i, q)
    return out


def _clutter():
    from hupr_amd import synth
    tg = [dict(range_bin=60, doppler_bin=3, az_bin=10, el_bin=2, amp=50.0)]
    x = synth.point_target_cube(tg, noise=5.0, seed=7).astype(np.int64)
    static = np.array([[20000, 0], [-18000, 9000], [15000, -12000], [-7000, -19000]], dtype=np.int64)      # per receiver, constant over chirps
    return np.clip(x + static[None, :, None, None, :], -32768, 32767).astype(np.int16)


def _full_scale():
    iq = np.full((1, 4, 192, 256, 2), 32767, dtype=np.int16)
    iq[:, :, ::2] = -32768
    return iq


def _coherent():
    from hupr_amd import synth
    x = synth.adc_cube_int16(3).astype(np.int64)
    c = np.arange(64)
    v = 20000.0 * np.exp(2j * np.pi * 3 * c / 64.0)
    x[0, 0, 3 * c, 0, 0] += np.rint(v.real).astype(np.int64)
    x[0, 0, 3 * c, 0, 1] += np.rint(v.imag).astype(np.int64)
    return np.clip(x, -32768, 32767).astype(np.int16)


_MAKERS = {"noise": _noise, "impulses": _impulses, "clutter": _clutter, "full_scale": _full_scale, "coherent": _coherent}


@functools.lru_cache(maxsize=None)
def frames(name):
    x = _MAKERS[name]()
    x.setflags(write=False)
    return x


# ---- buffers and the call (GPU) --------------------------------------------------------------------------------------------------------
TAIL = 4096                                  # int16 values in front of and behind the ADC cube


def out_floats(c):
    return {"cube": 2 * 16 * 64 * 64 * 8, "magnitude": 16 * 64 * 64 * 8, "loader": 8 * 2 * 64 * 64 * 8, "means": 16 * 64 * 64}[c.out]


def out_array(c, flat, n):
    a = flat.cpu().numpy()
    if c.out == "cube":
        return a.view(np.complex64).reshape(n, 16, 64, 64, 8)
    return a.reshape((n,) + {"magnitude": (16, 64, 64, 8), "loader": (8, 2, 64, 64, 8), "means": (16, 64, 64)}[c.out])


def adc_buffer(host):
    """-> (the whole int16 buffer on the device, its host copy, the cube's view): [full-scale tail | cube | full-scale tail]."""
    n = host.size
    buf = np.empty(TAIL + n + TAIL, dtype=np.int16)
    buf[:TAIL] = 32767
    buf[:TAIL:2] = -32768
    buf[TAIL + n:] = buf[:TAIL]
    buf[TAIL:TAIL + n] = host.reshape(-1)
    dev = torch.from_numpy(buf).cuda()
    return dev, buf, dev[TAIL:TAIL + n]


def guarded(n):
    """n fp32 words inside a NaN-pattern buffer: (buffer, the view); GUARD words = 1 KiB keep the view 16-byte aligned."""
    buf = nan_buffer(GUARD + n + GUARD, torch.float32)
    return buf, buf[GUARD:GUARD + n]


def assert_guards(buf, n, what):
    assert bool((bits(buf[:GUARD]) == NAN32).all()), "%s: the guard in front was written" % what
    assert bool((bits(buf[GUARD + n:]) == NAN32).all()), "%s: the guard behind was written" % what


def chain_call(L, rt, c, adc, n, out, ws, nbytes, table=None, n_swapped=0, fpf=1):
    flags, loader = flags_of(c), LOADER_CODE[c.out]
    head, tail = (rt.ptr(adc), n, rt.ptr(out)), (rt.ptr(ws), nbytes, rt.stream())
    if c.tdm:
        return L.hupr_fft_chain_tdm(*head, flags, loader, rt.ptr(table), n_swapped, fpf, *tail)
    if flags == 0:
        entry = (L.hupr_fft_chain_c64, L.hupr_fft_chain_loader_f32, L.hupr_fft_chain_loader_means_f32)[loader]
        return entry(*head, *tail)
    return L.hupr_fft_chain_opts(*head, flags, loader, *tail)


def launch(L, c, host, flags=SWAP_FLAGS, fpf=None):
    """One chain call of case ``c`` on the frames ``host`` in fresh guarded buffers, every buffer promise checked -> the output array."""
    from hupr_amd import runtime as rt
    n, what = host.shape[0], case_id(c)
    adc_dev, adc_host, adc = adc_buffer(host)
    obuf, out = guarded(n * out_floats(c))
    nbytes = L.hupr_fft_chain_ws_bytes(n)
    assert nbytes == n * 16 * 64 * 12 * 8
    wbuf, ws = guarded(nbytes // 4)
    table = torch.tensor(flags, dtype=torch.uint8, device="cuda") if c.tdm else None
    torch.cuda.synchronize()
    n0 = L.hupr_launch_count()
    rc = chain_call(L, rt, c, adc, n, out, ws, nbytes, table, len(flags), fpf or frames_per_flag(n))
    torch.cuda.synchronize()
    assert rc == 0, (what, L.hupr_last_error())
    assert L.hupr_launch_count() - n0 == 2, what
    assert_guards(obuf, out.numel(), what + " output")
    assert_guards(wbuf, ws.numel(), what + " workspace")
    assert np.array_equal(adc_dev.cpu().numpy(), adc_host), "%s: the ADC buffer was written" % what
    ob = bits(out)
    assert not bool((ob == NAN32).any()), "%s: an output element was never written, or a NaN-pattern workspace row was read" % what
    assert bool(torch.isfinite(out).all()), what
    if c.k1[0] == "doppler_range" and c.k1[2]:           # HALF: rows 0..3 and 12..15 of RD[sf][12][16][64] stay as they were
        rd = bits(ws).view(n, 12, 16, 64 * 2)
        assert bool((rd[:, :, :4] == NAN32).all()) and bool((rd[:, :, 12:] == NAN32).all()), what
        assert not bool((rd[:, :, 4:12] == NAN32).any()), what
    return out_array(c, out, n)


@pytest.fixture(scope="module", autouse=True)
def _reference_cache():
    yield
    fft_ref.drop_cache()


@pytest.fixture(scope="module")
def lib():
    from hupr_amd import runtime as rt
    return rt.lib()


def check_frames(c, name, got):
    """Every frame of ``got`` against the fp64 answer of its form, the measured ratio printed first."""
    host, form, grp, fam = frames(name), form_of(c), group_of(c), family(c)
    n = host.shape[0]
    worst = 0.0
    answers = [fft_ref.answer(host[k], form, swapped(c, n, k)) for k in range(n)]
    for k, ans in enumerate(answers):
        worst = max(worst, measured(got[k], ans, form))
    print("FFT64 %s %s %s %s log2(c) = %.4f" % (grp, fam, case_id(c), name, np.log2(max(worst, 1e-300))))
    for k, ans in enumerate(answers):
        assert_within(got[k], ans, form, GATE_C[grp][fam], "%s on %s, frame %d" % (case_id(c), name, k))
    return answers


def check_zero_doppler(c, name, got, answers):
    """What the gate does not say about Doppler index 8 / loader slot 4 / mean planes 8, 9."""
    form = form_of(c)
    rule = fft_ref.zero_rule(form.window, form.convention)
    z = {0: lambda a: a[:, 8], 1: lambda a: a[:, 4], 2: lambda a: a[:, 8:10]}[form.loader](got)
    what = "%s on %s" % (case_id(c), name)
    if rule == "exact":
        assert np.abs(z).max() == 0, what
    elif rule == "dither":
        assert np.abs(z).max() > 0, what
    elif not form.window & 2:                        # range-first: the order's own residue
        assert np.abs(z).max() > 0, what
        if form.loader == 1 and name != "impulses":
            p = z.reshape(-1, 2, 4096, 8).astype(np.float64)
            assert np.abs(p.std(axis=2, ddof=1) - 1).max() < 1e-3 and np.abs(p.mean(axis=2)).max() < 1e-3, what


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_fft_chain_form_matches_fp64(c, lib):
    for name in c.inputs.split():
        host = frames(name)
        n = host.shape[0]
        got = launch(lib, c, host)
        answers = check_frames(c, name, got)
        check_zero_doppler(c, name, got, answers)
        again = launch(lib, c, host)
        assert np.array_equal(got.view(np.uint32) if got.dtype != np.complex64 else got.view(np.uint64),
                              again.view(np.uint32) if again.dtype != np.complex64 else again.view(np.uint64)), "two launches differ"
        if name == "noise":                          # odd grids 3 * 12, 3 * 8, 3 * 16; a frame's bits do not depend on its place
            for k in range(n):
                one = launch(lib, c, host[k:k + 1], flags=(int(swapped(c, n, k)),), fpf=1)
                assert np.array_equal(one[0].view(np.uint8), np.ascontiguousarray(got[k]).view(np.uint8)), (case_id(c), k)


def test_coherent_input_has_a_plane_whose_mean_matters():
    """From the reference alone: at least one kept (Doppler 4..11, re / im, elevation) plane of ``coherent`` has |mean| / std in
    [1, 4] — the S * mean terms of both Normalize implementations carry weight there (noise cubes: at most 0.09)."""
    c = fft_ref.cube(frames("coherent")[0], 0, "dither")[4:12]
    ratio = np.stack([np.abs(c.real.mean(axis=(1, 2))) / c.real.std(axis=(1, 2), ddof=1),
                      np.abs(c.imag.mean(axis=(1, 2))) / c.imag.std(axis=(1, 2), ddof=1)])
    print("coherent: worst |mean| / std = %.3f" % ratio.max())
    assert ((ratio >= 1.0) & (ratio <= 4.0)).any(), ratio.max()


# ---- hupr_k_loader_normalize on cubes of its own ------------------------------------------------------------------------------------------
def normalize_inputs():
    """Three complex64 cubes (the fp64 answers rounded once) and their frames' scales: noise W = 0, noise W = 3, coherent W = 0."""
    picks = ((frames("noise")[0], 0), (frames("noise")[1], 3), (frames("coherent")[0], 0))
    cubes = np.stack([fft_ref.cube(iq, w, "dither").astype(np.complex64) for iq, w in picks])
    scales = []
    for iq, w in picks:
        a = fft_ref.answer(iq, Form(w, "dither", 0, False, False))
        scales.append(a.scale)
    return cubes, scales


def normalize_answer(cube_c64, scale):
    c = cube_c64.astype(np.complex128)
    ld = fft_ref.loader(c)
    return fft_ref.Answer(ld, float(scale[0]), scale, fft_ref.plane_std(c), c, ld)


def test_loader_normalize_matches_fp64(lib):
    from hupr_amd import runtime as rt
    cubes, scales = normalize_inputs()
    n = cubes.shape[0]
    form = Form(0, "dither", 1, False, False)

    def once():
        cbuf, cv = guarded(cubes.size * 2)
        cv.copy_(torch.from_numpy(cubes.view(np.float32).reshape(-1)))
        before = bits(cbuf).clone()
        obuf, out = guarded(n * 8 * 2 * 64 * 64 * 8)
        torch.cuda.synchronize()
        n0 = lib.hupr_launch_count()
        rc = lib.hupr_loader_normalize_c64(rt.ptr(cv), n, rt.ptr(out), rt.stream())
        torch.cuda.synchronize()
        assert rc == 0 and lib.hupr_launch_count() - n0 == 1
        assert_guards(obuf, out.numel(), "loader_normalize output")
        assert torch.equal(bits(cbuf), before), "the cube was written"
        assert not bool((bits(out) == NAN32).any()) and bool(torch.isfinite(out).all())
        return out.cpu().numpy().reshape(n, 8, 2, 64, 64, 8)

    got, again = once(), once()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    worst = 0.0
    answers = [normalize_answer(cubes[k], scales[k]) for k in range(n)]
    for k, ans in enumerate(answers):
        worst = max(worst, measured(got[k], ans, form))
    print("FFT64 loader_normalize df loader_normalize all log2(c) = %.4f" % np.log2(worst))
    for k, ans in enumerate(answers):
        assert_within(got[k], ans, form, GATE_C["loader_normalize"]["df"], "loader_normalize, cube %d" % k)
    n0 = lib.hupr_launch_count()
    assert lib.hupr_loader_normalize_c64(None, 0, None, None) == 0 and lib.hupr_launch_count() == n0


# ---- the zero-Doppler rule under a window (include/hupr.h) ------------------------------------------------------------------------------
def _case(conv, window, out, tdm=False):
    (c,) = [c for c in CASES if (c.conv, c.window, c.out, c.tdm) == (conv, window, out, tdm)]
    return c


@pytest.mark.parametrize("out", ["cube", "loader", "means"])
def test_range_window_keeps_the_zero_doppler_convention(out, lib):
    """HUPR_FFT_HANN_RANGE alone: index 8 carries the SAME unwindowed dither as W = 0, bit for bit (the dither row goes through the
    same range FFT), and exactly zero under HUPR_FFT_ZERO_DOPPLER_EXACT; every other index differs from W = 0 (the window is on)."""
    host = frames("noise")
    z = {"cube": lambda a: a[:, 8], "loader": lambda a: a[:, 4], "means": lambda a: a[:, 8:10]}[out]
    rest = {"cube": lambda a: a[:, 9], "loader": lambda a: a[:, 5], "means": lambda a: a[:, 10:12]}[out]
    w0, w1 = launch(lib, _case("dither", 0, out), host), launch(lib, _case("dither", 1, out), host)
    assert np.array_equal(np.ascontiguousarray(z(w0)).view(np.uint8), np.ascontiguousarray(z(w1)).view(np.uint8))
    assert np.abs(z(w1)).max() > 0 and not np.array_equal(rest(w0), rest(w1))
    e1 = launch(lib, _case("exact", 1, out), host)
    assert np.abs(z(e1)).max() == 0
    keep = np.ones(w1.shape[1], dtype=bool)
    keep[{"cube": [8], "loader": [4], "means": [8, 9]}[out]] = False
    assert np.array_equal(e1[:, keep].view(np.uint8), w1[:, keep].view(np.uint8))      # the two conventions agree on every other index


@pytest.mark.parametrize("window", [2, 3])
@pytest.mark.parametrize("out", ["cube", "loader"])
def test_doppler_window_makes_the_conventions_a_no_op(window, out, lib):
    """With HUPR_FFT_HANN_DOPPLER index 8 is ordinary leakage (gated against fp64 by the table like every other index);
    HUPR_FFT_ZERO_DOPPLER_EXACT stays accepted and changes no bit."""
    host = frames("noise")[:1]
    c = _case("dither", window, out)
    plain = launch(lib, c, host)
    exact = launch(lib, c._replace(conv="exact"), host)
    assert np.array_equal(plain.view(np.uint8), exact.view(np.uint8))
    z = plain[:, 8] if out == "cube" else plain[:, 4]
    assert np.abs(z).max() > 0
    if out == "cube":                                    # leakage, not residue: of the order of the neighbouring bins
        assert np.abs(plain[:, 8]).max() > 1e-3 * np.abs(plain[:, 7]).max()


# ---- n_sf = 0 and the refused calls ------------------------------------------------------------------------------------------------------
# name, what differs from a good call of n_sf = 1 (hupr_fft_chain_opts, or hupr_fft_chain_tdm with ``tdm``), the return code
REFUSED = [
    ("out-at-8-mod-16", dict(out_off=8), HUPR_ERR_ARG),
    ("ws-at-8-mod-16", dict(ws_off=8), HUPR_ERR_ARG),
    ("adc-at-2-mod-4", dict(adc_off=2), HUPR_ERR_ARG),
    ("ws_bytes-one-short", dict(short=1), HUPR_ERR_WORKSPACE),
    ("n_sf-2^20+1", dict(n_sf=(1 << 20) + 1), HUPR_ERR_ARG),
    ("n_sf-negative", dict(n_sf=-1), HUPR_ERR_ARG),
    ("loader-3", dict(loader=3), HUPR_ERR_ARG),
    ("loader-3-tdm", dict(loader=3, tdm=True), HUPR_ERR_ARG),
    ("flag-bit-32", dict(flags=32), HUPR_ERR_ARG),
    ("flag-bit-64-tdm", dict(flags=64 | 1, tdm=True), HUPR_ERR_ARG),
    ("loader-with-magnitude", dict(loader=1, flags=MAGNITUDE), HUPR_ERR_ARG),
    ("means-with-magnitude", dict(loader=2, flags=MAGNITUDE | 3), HUPR_ERR_ARG),
    ("exact-with-range-first", dict(flags=ZERO_DOPPLER_EXACT | RANGE_FIRST), HUPR_ERR_ARG),
    ("exact-with-range-first-tdm", dict(flags=ZERO_DOPPLER_EXACT | RANGE_FIRST, tdm=True), HUPR_ERR_ARG),
    ("tdm-frames_per_flag-0", dict(tdm=True, table=True, n_swapped=2, fpf=0), HUPR_ERR_ARG),
    ("tdm-n_swapped-negative", dict(tdm=True, table=True, n_swapped=-1, fpf=2), HUPR_ERR_ARG),
    ("tdm-table-with-n_swapped-0", dict(tdm=True, table=True, n_swapped=0, fpf=2), HUPR_ERR_ARG),
]


def refused_call(L, r, adc, out, ws, table, nbytes, stream):
    """The call of REFUSED row ``r`` on the addresses given (integers)."""
    k = dict(n_sf=1, flags=0, loader=0, tdm=False, table=False, n_swapped=0, fpf=1, out_off=0, ws_off=0, adc_off=0, short=0)
    k.update(r[1])
    head, tail = (adc + k["adc_off"], k["n_sf"], out + k["out_off"]), (ws + k["ws_off"], nbytes - k["short"], stream)
    if k["tdm"]:
        return L.hupr_fft_chain_tdm(*head, k["flags"], k["loader"], table if k["table"] else None, k["n_swapped"], k["fpf"], *tail)
    return L.hupr_fft_chain_opts(*head, k["flags"], k["loader"], *tail)


@pytest.mark.parametrize("r", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_calls_leave_everything_untouched(r, lib):
    from hupr_amd import runtime as rt
    adc_dev, adc_host, adc = adc_buffer(frames("noise")[:1])
    obuf, out = guarded(2 * 16 * 64 * 64 * 8)
    nbytes = lib.hupr_fft_chain_ws_bytes(1)
    wbuf, ws = guarded(nbytes // 4)
    table = torch.tensor(SWAP_FLAGS, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n0 = lib.hupr_launch_count()
    rc = refused_call(lib, r, rt.ptr(adc), rt.ptr(out), rt.ptr(ws), rt.ptr(table), nbytes, rt.stream())
    torch.cuda.synchronize()
    assert rc == r[2] and lib.hupr_last_error(), (r[0], rc)
    assert lib.hupr_launch_count() == n0
    assert bool((bits(obuf) == NAN32).all()) and bool((bits(wbuf) == NAN32).all()), r[0]
    assert np.array_equal(adc_dev.cpu().numpy(), adc_host)


def test_empty_batch_launches_nothing(lib):
    from hupr_amd import runtime as rt
    obuf, out = guarded(64)
    wbuf, ws = guarded(64)
    adc = torch.zeros(16, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    n0 = lib.hupr_launch_count()
    assert lib.hupr_fft_chain_ws_bytes(0) == 0
    for loader in (0, 1, 2):
        for flags in (0, 3, ZERO_DOPPLER_EXACT, RANGE_FIRST | 1):
            assert lib.hupr_fft_chain_opts(rt.ptr(adc), 0, rt.ptr(out), flags, loader, rt.ptr(ws), 0, rt.stream()) == 0
            assert lib.hupr_fft_chain_tdm(rt.ptr(adc), 0, rt.ptr(out), flags, loader, None, 0, 1, rt.ptr(ws), 0, rt.stream()) == 0
    assert lib.hupr_fft_chain_c64(None, 0, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert lib.hupr_launch_count() == n0
    assert bool((bits(obuf) == NAN32).all()) and bool((bits(wbuf) == NAN32).all())
