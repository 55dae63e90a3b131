"""CPU (no GPU needed): the case table of tests/test_fft_fp64_gpu.py against the build and against its own gate.

Routes.  The compiled instantiations of hupr_k_range_doppler, hupr_k_doppler_range, hupr_k_angle and hupr_k_loader_normalize are read
from the device listing the build keeps, by their mangled template arguments: 21.  A Python mirror of fft_chain_common's dispatch
((flags, loader, tdm) -> the two kernels) sends the table onto EXACTLY that set (hupr_k_loader_normalize is the one kernel of
hupr_loader_normalize_c64): an instantiation added later without a case fails here, and so does a case whose line names another
kernel than the dispatch launches.  The refused calls are refused on made-up addresses without a device, by host checks alone.

The gate, on outputs synthesised from the fp64 reference (oracle/fft_chain.py and tests/tdm_ref.py, staged).  It ACCEPTS the reference
rounded to fp32 after each stage (range-Doppler, angle, Normalize with fp32 mean and 1 / std).  It REJECTS, with the constants committed
in the GPU module (FAULTS: the inputs named reject the fault; "impulses" frames are pure exponentials in every cell, so an index slip
is an error of O(A) nearly everywhere):
  two virtual antennas exchanged           noise, impulses        the TX1 / TX2 demux exchanged          noise, impulses
  the range crop off by one                noise, impulses        the azimuth flip off by one            noise, impulses
  the elevation map (3 - e) as (e - 3)     noise, impulses        one sign error in w8^1 Q               noise, impulses (elevated antennas)
  the Doppler window left out              noise, impulses        the Doppler window before the mean     noise, impulses
  a TDM factor of the wrong slot           noise, impulses        biased variance (n for n - 1)          noise (loader), where |n| > ~0.5
  a missing mean subtraction               coherent (loader)      one Doppler row of the HALF range = 0  noise (loader)"""
import re

import numpy as np
import pytest

import fft_ref
import tdm_ref
import test_fft_fp64_gpu as T
from fft_ref import Form
from oracle import fft_chain as offt


@pytest.fixture(scope="module", autouse=True)
def _reference_cache():
    yield
    fft_ref.drop_cache()


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from hupr_amd import runtime
    return runtime.lib()


# ---- routes ------------------------------------------------------------------------------------------------------------------------
def kernels_of(flags, loader, tdm):
    """The mirror of fft_chain_common (csrc/fft_chain.hip): the two kernels a call that is not refused launches."""
    W = flags & 3
    k1 = ("range_doppler", W) if flags & T.RANGE_FIRST else ("doppler_range", W, loader != 0)
    mode = 3 if loader == 2 else 1 if loader == 1 else 2 if flags & T.MAGNITUDE else 0
    return k1, ("angle", mode, bool(tdm))


def refused(flags, loader):
    """The mirror of the flag rules: True where hupr_fft_chain_opts / _tdm answer HUPR_ERR_ARG whatever the buffers."""
    return bool(loader not in (0, 1, 2) or (flags & ~31) != 0 or (flags & T.ZERO_DOPPLER_EXACT and flags & T.RANGE_FIRST)
                or (loader != 0 and flags & T.MAGNITUDE))


def compiled():
    """The instantiations in the listing of csrc/fft_chain.hip, as the table names them."""
    from listing import kernel_metadata
    out = []
    for name in kernel_metadata("fft_chain"):
        m = re.search(r"hupr_k_range_dopplerILi(\d)EE", name)
        if m:
            out.append(("range_doppler", int(m.group(1))))
        m = re.search(r"hupr_k_doppler_rangeILi(\d)ELb([01])ELi\d+EE", name)
        if m:
            out.append(("doppler_range", int(m.group(1)), m.group(2) == "1"))
        m = re.search(r"hupr_k_angleILi(\d)ELb([01])E", name)
        if m:
            out.append(("angle", int(m.group(1)), m.group(2) == "1"))
        if "hupr_k_loader_normalize" in name:
            out.append(T.LN)
    return out


def test_the_table_reaches_exactly_the_compiled_instantiations():
    have = compiled()
    assert len(have) == len(set(have)) == 21, sorted(have)
    reached = {c.k1 for c in T.CASES} | {c.k2 for c in T.CASES} | {T.LN}
    assert reached == set(have), (sorted(reached - set(have)), sorted(set(have) - reached))


@pytest.mark.parametrize("c", T.CASES, ids=[T.case_id(c) for c in T.CASES])
def test_fp64_case_table_routes(c):
    flags, loader = T.flags_of(c), T.LOADER_CODE[c.out]
    assert not refused(flags, loader)
    assert kernels_of(flags, loader, c.tdm) == (c.k1, c.k2)
    assert set(c.inputs.split()) <= set(T._MAKERS) and "noise" in c.inputs.split()


def test_the_table_feeds_every_kernel_as_asked():
    """Every K1 is consumed by a cube-form K2 (the HALF forms, which write eight rows, by a loader-form K2); every K2 is fed by W = 0
    and by W = 3; the minimum list of forms is there."""
    for k1 in {c.k1 for c in T.CASES}:
        half = k1[0] == "doppler_range" and k1[2]
        assert any(c.k1 == k1 and (c.out in ("loader", "means") if half else c.out == "cube") for c in T.CASES), k1
    for k2 in {c.k2 for c in T.CASES}:
        assert {c.window for c in T.CASES if c.k2 == k2} >= {0, 3}, k2
    have = {(c.conv, c.window, c.out, c.tdm) for c in T.CASES}
    assert len(have) == len(T.CASES)
    want = {("dither", W, o, False) for W in range(4) for o in ("cube", "magnitude", "loader", "means")}
    want |= {("exact", W, o, False) for W in (0, 1) for o in ("cube", "loader", "means")}
    want |= {("range_first", W, "cube", False) for W in range(4)} | {("range_first", W, o, False) for W in (0, 3) for o in ("magnitude", "loader", "means")}
    want |= {("dither", W, "cube", True) for W in range(4)} | {("dither", W, o, True) for W in (0, 3) for o in ("magnitude", "loader", "means")}
    assert have >= want, sorted(want - have)
    for name in T._MAKERS:
        assert any(name in c.inputs.split() for c in T.CASES), name


@pytest.mark.parametrize("r", T.REFUSED, ids=[r[0] for r in T.REFUSED])
def test_refused_calls_are_refused_by_host_checks(r, L):
    """On made-up addresses and without a device: the error comes back before anything is launched or dereferenced."""
    base = 1 << 24
    n0 = L.hupr_launch_count()
    rc = T.refused_call(L, r, base, 2 * base, 3 * base, 4 * base, L.hupr_fft_chain_ws_bytes(1), None)
    assert rc == r[2], (r[0], rc, L.hupr_last_error())
    assert L.hupr_last_error()
    assert L.hupr_launch_count() == n0
    k = dict(flags=0, loader=0)
    k.update(r[1])
    if refused(k["flags"], k["loader"]):
        assert r[2] == T.HUPR_ERR_ARG


def test_flag_rules_and_workspace_bytes_on_the_host(L):
    """Every (flags, loader) pair: with n_sf = 0 the call answers HUPR_OK exactly where the mirror accepts the pair (the flag rules come
    before the empty batch); nothing is launched.  hupr_fft_chain_ws_bytes is n_sf * 16 * 64 * 12 complex64."""
    n0 = L.hupr_launch_count()
    for flags in range(0, 72):
        for loader in (-1, 0, 1, 2, 3):
            want = T.HUPR_ERR_ARG if refused(flags, loader) else 0
            assert L.hupr_fft_chain_opts(None, 0, None, flags, loader, None, 0, None) == want, (flags, loader)
            assert L.hupr_fft_chain_tdm(None, 0, None, flags, loader, None, 0, 1, None, 0, None) == want, (flags, loader)
    assert L.hupr_launch_count() == n0
    for n in (-5, -1, 0):
        assert L.hupr_fft_chain_ws_bytes(n) == 0
    for n in (1, 3, 12, 256, 1 << 20):
        assert L.hupr_fft_chain_ws_bytes(n) == n * 16 * 64 * 12 * 8


def test_gate_constants_respect_the_cap():
    assert set(T.GATE_C) == {"cube", "magnitude", "loader", "means", "loader_normalize"}
    for grp, fams in T.GATE_C.items():
        assert set(fams) == ({"df"} if grp == "loader_normalize" else {"df", "rf", "tdm"}), grp
        for fam, c in fams.items():
            assert 0 < c <= 2.0 ** -15 and np.log2(c) == int(np.log2(c)), (grp, fam, c)


# ---- the staged reference, with one fault or with fp32 roundings ---------------------------------------------------------------------------
def c64(x):
    return x.astype(np.complex64).astype(np.complex128)


def index_map(M5, r_hi=94, a0=31, emap=lambda e: (3 - e) % 8):
    """tdm_ref.index_map with its three constants open, for the faults only."""
    e = emap(np.arange(8)) % 8
    a = (a0 - np.arange(64)) % 64
    d = (56 + np.arange(16)) % 64
    r = r_hi - np.arange(64)
    return np.ascontiguousarray(M5[e[None, None, None, :], a[None, None, :, None], d[:, None, None, None], r[None, :, None, None]])


def staged(iq, window=0, rule="dither", tdm=False, swapped=False, fault=None, r32=False):
    """The chain of tdm_ref.cube stage by stage -> complex128 (16, 64, 64, 8); ``r32``: every stage's result rounded to complex64;
    ``fault``: one of FAULTS's cube faults."""
    frame = iq[..., 0].astype(np.float64) + 1j * iq[..., 1].astype(np.float64)
    az, el = offt.demux(frame)
    if fault == "demux":                                 # the chirps of TX1 (3 c + 1) and TX2 (3 c + 2) exchanged
        az, el = np.concatenate([frame[:, 0::3], frame[:, 1::3]], axis=0), frame[:, 2::3].copy()
    if fault == "no_doppler_window":
        window &= 1
    if fault == "window_before_mean":
        h = np.hanning(64)[None, :, None]
        az, el = offt.range_doppler(az * h, el * h, window & 1)
    else:
        az, el = offt.range_doppler(az, el, window)
    if rule == "dither":
        dz = np.fft.fft(offt.zero_doppler_dither(iq), axis=1)
        az[:, 0, :], el[:, 0, :] = dz[:8], dz[8:]
    elif rule == "exact":
        az[:, 0, :], el[:, 0, :] = 0.0, 0.0
    if r32:
        az, el = c64(az), c64(el)
    if fault == "half_row":                              # Doppler bin 62 = index 6 = loader slot 2
        az[:, 62, :], el[:, 62, :] = 0.0, 0.0
    if fault == "antennas":
        az[[2, 3]] = az[[3, 2]]
    if tdm:
        if fault == "tdm_slot":                          # the second azimuth half with the elevated row's slot
            d = np.arange(64)
            d = np.where(d < 32, d, d - 64).astype(np.float64)
            k = tdm_ref.slots(swapped).astype(np.float64).copy()
            k[k == 2] = 1
            f = np.exp(-2j * np.pi * d[None, :] * k[:, None] / 192.0)
            az, el = az * f[:8, :, None], el * f[8:, :, None]
        else:
            az, el = tdm_ref.compensate(az, el, swapped)
        if r32:
            az, el = c64(az), c64(el)
    M = offt.angle_cube(az, el)
    if fault == "w8_sign":                               # U = h (1 + i) Q for h (1 - i) Q: the odd e' see i U
        MQ = offt.angle_cube(np.zeros_like(az), el)
        M[1::2] += (1j - 1.0) * MQ[1::2]
    if fault == "crop":
        out = index_map(M, r_hi=95)
    elif fault == "flip":
        out = index_map(M, a0=30)
    elif fault == "elevation":
        out = index_map(M, emap=lambda e: (e - 3) % 8)
    else:
        out = tdm_ref.index_map(M)
    return c64(out) if r32 else out


def normalized(c, fault=None, r32=False):
    """The loader tensor (8, 2, 64, 64, 8) of cube ``c``; ``r32``: fp32 mean, fp32 1 / std and fp32 arithmetic on the fp32 cube."""
    out = np.zeros((8, 2, 64, 64, 8), dtype=np.float64)
    for f in range(8):
        for e in range(8):
            for k, p in enumerate((c[4 + f, :, :, e].real, c[4 + f, :, :, e].imag)):
                if not p.any():
                    continue
                mean, std = p.mean(), p.std(ddof=0 if fault == "biased" else 1)
                if fault == "no_mean":
                    mean = 0.0
                if r32:
                    m32, r = np.float32(mean), np.float32(1.0 / std)
                    out[f, k, :, :, e] = p.astype(np.float32) * r + (-(m32 * r))
                else:
                    out[f, k, :, :, e] = (p - mean) / std
    return out


def in_form(c, form, fault=None, r32=False):
    if form.loader == 0:
        return np.abs(c).astype(np.float32) if form.magnitude and r32 else np.abs(c) if form.magnitude else c
    ld = normalized(c, fault, r32)
    if form.loader == 1:
        return ld
    m = tdm_ref.means(ld)
    return m.astype(np.float32).astype(np.float64) if r32 else m


def frame_of(name, k=0):
    return T.frames(name)[k]


ACCEPT = [c for c in T.CASES if c.window in (0, 3) and c.conv != "exact"] + [c for c in T.CASES if c.conv == "exact" and c.window == 1]


@pytest.mark.parametrize("c", ACCEPT, ids=[T.case_id(c) for c in ACCEPT])
def test_gate_accepts_the_reference_rounded_to_fp32_at_each_stage(c):
    form = T.form_of(c)
    names = [n for n in ("noise", "coherent") if n in c.inputs.split()]
    for name in names:
        iq = frame_of(name)
        sw = T.swapped(c, 1, 0)
        ans = fft_ref.answer(iq, form, sw)
        got = in_form(staged(iq, form.window, fft_ref.zero_rule(form.window, form.convention), form.tdm, sw, r32=True), form, r32=True)
        ok = T.within(got, ans, form, T.GATE_C[T.group_of(c)][T.family(c)])
        assert bool(ok.all()), (T.case_id(c), name, np.log2(T.measured(got, ans, form)))
        assert form.magnitude or T.measured(got, ans, form) > 0          # (it is another result than the reference's)


def test_gate_accepts_an_fp32_normalize_of_the_given_cube():
    cubes, scales = T.normalize_inputs()
    form = Form(0, "dither", 1, False, False)
    for k in range(cubes.shape[0]):
        ans = T.normalize_answer(cubes[k], scales[k])
        got = normalized(cubes[k].astype(np.complex128), r32=True)
        assert bool(T.within(got, ans, form, T.GATE_C["loader_normalize"]["df"]).all()), k


# fault -> (the output form it is judged in, window, tdm, {input: least fraction of the elements that must fail the gate})
FAULTS = {
    "antennas": ("cube", 0, False, {"noise": 0.9, "impulses": 0.9}),
    "demux": ("cube", 0, False, {"noise": 0.9, "impulses": 0.9}),
    "crop": ("cube", 0, False, {"noise": 0.9, "impulses": 0.9}),
    "flip": ("cube", 0, False, {"noise": 0.9, "impulses": 0.9}),
    "elevation": ("cube", 0, False, {"noise": 0.5, "impulses": 0.5}),
    "w8_sign": ("cube", 0, False, {"noise": 0.4, "impulses": 0.4}),
    "no_doppler_window": ("cube", 3, False, {"noise": 0.9, "impulses": 0.9}),
    "window_before_mean": ("cube", 3, False, {"noise": 0.9, "impulses": 0.9}),
    "tdm_slot": ("cube", 0, True, {"noise": 0.5, "impulses": 0.5}),
    "half_row": ("loader", 0, False, {"noise": 0.9}),
    "biased": ("loader", 0, False, {"noise": 0.3}),
    "no_mean": ("loader", 0, False, {"coherent": 0.005}),
}
# the impulse frame a fault shows on: frame k = 3 rx + tx.  Antenna 2 <-> 3: rx 2, TX0; demux: TX1; w8 and elevation: an elevated antenna
# (TX1); the TDM slot: TX2 (second azimuth half); the crop, the flip and the windows: antenna 3 (rx 3, TX0), which reaches every elevation bin
IMPULSE_FRAME = {"antennas": 6, "demux": 1, "w8_sign": 1, "elevation": 1, "tdm_slot": 2, "crop": 9, "flip": 9, "no_doppler_window": 9,
                 "window_before_mean": 9}


@pytest.mark.parametrize("fault,name", [(f, n) for f, v in FAULTS.items() for n in v[3]])
def test_gate_rejects(fault, name):
    out, window, tdm, need = FAULTS[fault]
    (c,) = [c for c in T.CASES if (c.conv, c.window, c.out, c.tdm) == ("dither", window, out, tdm)]
    form = T.form_of(c)
    iq = frame_of(name, IMPULSE_FRAME.get(fault, 0) if name == "impulses" else 0)
    ans = fft_ref.answer(iq, form, False)
    cube_fault = fault if fault not in ("biased", "no_mean") else None
    got = in_form(staged(iq, window, "dither", tdm, False, fault=cube_fault), form, fault)
    # (touched: beyond the fp64 noise of another order of operations, on the scale of the element's own Doppler index)
    touched = T.error(got, ans, form) > 1e-10 * (1.0 if form.loader else ans.scale[:, None, None, None])
    ok = T.within(got, ans, form, T.GATE_C[T.group_of(c)][T.family(c)])
    frac = float((~ok & touched).sum()) / max(int(touched.sum()), 1)
    print("%s on %s: %.3f of the %d touched elements fail the gate" % (fault, name, frac, int(touched.sum())))
    assert touched.any() and frac >= need[name], (fault, name, frac)
    assert not bool((~ok & ~touched).any())


def test_the_staged_reference_without_a_fault_is_the_reference():
    iq = frame_of("noise")
    for window, rule, tdm, sw in ((0, "dither", False, False), (3, None, True, True), (1, "exact", False, False)):
        conv = "range_first" if rule is None and not window & 2 else rule or "dither"
        assert np.array_equal(staged(iq, window, rule, tdm, sw), fft_ref.cube(iq, window, conv, tdm, sw))
    c = fft_ref.cube(iq, 0, "dither")
    assert np.allclose(normalized(c), fft_ref.loader(c), rtol=0, atol=1e-12)
    M = np.arange(8 * 64 * 64 * 256, dtype=np.float64).reshape(8, 64, 64, 256)
    assert np.array_equal(index_map(M), tdm_ref.index_map(M))          # the open-constant map of the faults, at its defaults
