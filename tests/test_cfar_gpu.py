"""GPU (-m gpu): hupr_cfar_ra_f32 and hupr_presence_update (csrc/cfar.hip) against the fp64 statement of their rule in
tests/cfar_ref.py.  n in {1, 3} frames, the four (guard, train) pairs, three inputs: seeded noise, noise plus one cell at 1e4 times the
noise power (what a difference of box sums gets wrong), noise plus strong cells in the corners and on the edges.  The references are
computed once per case and shared.  The one test without the gpu mark checks the inputs themselves on the CPU."""
import functools

import numpy as np
import pytest
import torch

import cfar_ref as ref

gpu = pytest.mark.gpu
PFA = 1e-3                       # noise alone then leaves some tens of detections per frame: the summary has something to sum
U = 2.0 ** -24
NS = (1, 3)
CASES = [(name, n, g, t) for name in ref.INPUTS for n in NS for g, t in ref.PAIRS]
IDS = ["%s-n%d-g%dt%d" % c for c in CASES]
RATIO_BAND = 1e-4                # cells whose fp64 p / (alpha noise) is closer to 1 than this may fall either way in fp32
LEFT_OUT_CAP = 0.0005            # ... and may be at most 0.05 % of the examined cells of a case


def snr_tol(g, t):
    """Twice the bound of the kernel's summation order (include/hupr.h): the power's two roundings, at most 2 w additions along the
    row and 2 w down the rows, the division by N and the division p / noise: (4 w + 6) 2^-24, 4.5e-6 at w = 8 — tighter than the
    4e-5 of a running sum over 288 cells."""
    return 2.0 * (4 * (g + t) + 6) * U


@functools.lru_cache(maxsize=None)
def planes(name, n):
    return ref.INPUTS[name](n, 31 + n)


@functools.lru_cache(maxsize=None)
def reference(name, n, g, t):
    out = ref.ref_cfar(planes(name, n), PFA, g, t)
    examined = np.zeros(out["mask"].shape, bool)
    examined[:, list(ref.SLOTS)] = True
    with np.errstate(invalid="ignore"):
        out["left_out"] = examined & (np.abs(out["ratio"] - 1.0) <= RATIO_BAND)
    out["examined"] = examined
    return out


@pytest.mark.parametrize("name,n,g,t", CASES, ids=IDS)
def test_inputs_keep_the_reference_clear_of_the_threshold(name, n, g, t):
    """On the CPU: the seeds leave at most 0.05 % of a case's examined cells within 1e-4 of the threshold, the two largest SNRs among
    the detections of every frame differ by more than 1e-4 relative, and every case has detections."""
    out = reference(name, n, g, t)
    assert out["left_out"].sum() <= LEFT_OUT_CAP * out["examined"].sum()
    for i in range(n):
        s = np.sort(out["snr"][i][out["mask"][i].astype(bool)])
        assert s.size >= 2 and s[-1] > s[-2] * (1 + 1e-4)
    if name == "spike":                  # the strong cell is a detection, at 1e4 times the mean noise power
        assert out["summary"][:, 1].min() > 3e3
    if name == "border":                 # the corner and edge cells are detections
        m = out["mask"].any(axis=1)
        assert m[:, 0, 0].all() and m[:, 0, 63].all() and m[:, 63, 0].all() and m[:, 63, 63].all() and m[:, 0, 29].all() and m[:, 45, 63].all()


def run(x, g, t, want_mask=True, want_snr=True, pfa=PFA):
    from hupr_amd import functional as F_
    res = F_.cfar_ra(torch.from_numpy(np.ascontiguousarray(x)).cuda(), pfa, g, t, want_mask=want_mask, want_snr=want_snr)
    return (res.summary.cpu().numpy(), None if res.mask is None else res.mask.cpu().numpy(), None if res.snr is None else res.snr.cpu().numpy())


@gpu
@pytest.mark.parametrize("name,n,g,t", CASES, ids=IDS)
def test_detector_matches_the_fp64_rule(name, n, g, t):
    want = reference(name, n, g, t)
    summary, mask, snr = run(planes(name, n), g, t)
    assert summary.shape == (n, 8) and mask.shape == snr.shape == (n, 8, 64, 64) and mask.dtype == np.uint8
    # slot 4 is never examined
    assert not mask[:, ref.DEAD_SLOT].any() and not snr[:, ref.DEAD_SLOT].any()
    # SNR = p / noise, and through it the noise estimate (the kernel writes no other trace of it; p itself carries 2 of the roundings)
    ex = want["examined"]
    err = np.abs(snr[ex].astype(np.float64) - want["snr"][ex]) / want["snr"][ex]
    print("%s n=%d g=%d t=%d: snr rel err max %.3g (tol %.3g), left out %d" % (name, n, g, t, err.max(), snr_tol(g, t), want["left_out"].sum()))
    assert err.max() <= snr_tol(g, t)
    # the mask, wherever fp64 is clear of the threshold
    firm = ex & ~want["left_out"]
    assert np.array_equal(mask[firm], want["mask"][firm])
    assert set(np.unique(mask)) <= {0, 1}
    # the summary
    for i in range(n):
        loose = int(want["left_out"][i].sum())
        got, w = summary[i].astype(np.float64), want["summary"][i]
        assert got[0] == mask[i].sum() and abs(got[0] - w[0]) <= loose
        assert tuple(got[2:5]) == tuple(w[2:5])
        assert abs(got[1] - w[1]) <= snr_tol(g, t) * w[1]
        if loose == 0:
            assert abs(got[5] - w[5]) <= 5e-3 and abs(got[6] - w[6]) <= 5e-3          # 2 * 4e-5 * 63: the weights' error
            assert abs(got[7] - w[7]) <= 3.2e-4                                      # likewise over d = -4 .. 3


@gpu
def test_summary_does_not_depend_on_the_optional_outputs():
    x = planes("border", 3)
    full = run(x, 2, 4)
    for want_mask, want_snr in ((False, False), (True, False), (False, True)):
        s, m, q = run(x, 2, 4, want_mask, want_snr)
        assert np.array_equal(s.view(np.int32), full[0].view(np.int32))
        assert (m is None) == (not want_mask) and (q is None) == (not want_snr)
        assert m is None or np.array_equal(m, full[1])
        assert q is None or np.array_equal(q.view(np.int32), full[2].view(np.int32))


@gpu
@pytest.mark.parametrize("g,t", ref.PAIRS)
def test_slot_four_is_ignored_and_runs_repeat(g, t):
    x = planes("spike", 3).copy()
    a = run(x, g, t)
    b = run(x, g, t)
    y = x.copy()
    y[:, 8] = ref.noise_planes(3, 99)[:, 0] * 1e6
    y[:, 9] = np.nan
    y[1, 8, 5, 5] = np.inf
    c = run(y, g, t)
    for other in (b, c):
        for u, v in zip(a, other):
            assert np.array_equal(u.view(np.int32) if u.dtype == np.float32 else u, v.view(np.int32) if v.dtype == np.float32 else v)


@gpu
@pytest.mark.parametrize("g,t", ref.PAIRS)
@pytest.mark.parametrize("r,a", [(30, 33), (0, 0), (63, 20)])
def test_a_nan_detects_nothing_around_it_and_changes_nothing_else(g, t, r, a):
    w = g + t
    x = planes("noise", 1).copy()
    clean = run(x, g, t)
    f = 2
    x[0, 2 * f + 1, r, a] = np.nan
    summary, mask, snr = run(x, g, t)
    rr, aa = np.mgrid[0:64, 0:64]
    cheb = np.maximum(np.abs(rr - r), np.abs(aa - a))
    trains = (cheb > g) & (cheb <= w)                       # the cells whose training ring holds the NaN
    touched = np.zeros((1, 8, 64, 64), bool)
    touched[0, f] = trains
    touched[0, f, r, a] = True
    assert not mask[touched].any() and np.isnan(snr[touched]).all()
    assert np.array_equal(mask[~touched], clean[1][~touched])
    assert np.array_equal(snr[~touched].view(np.int32), clean[2][~touched].view(np.int32))
    assert np.isfinite(summary).all() and summary[0, 0] == mask.sum()


@gpu
def test_no_detection_and_all_zero_planes():
    s, m, q = run(np.zeros((2, 16, 64, 64), np.float32), 2, 4)
    assert not m.any() and not q.any()                       # 0 / 0 is 0
    assert np.array_equal(s, np.tile(np.float32([0, 0, -1, -1, -1, 0, 0, 0]), (2, 1)))


@gpu
def test_offline_entry_takes_planes_and_adc_cubes():
    from hupr_amd import functional as F_, preprocessing, synth
    x = torch.from_numpy(planes("border", 3)).cuda()
    a, b = preprocessing.cfar_detect(x.view(3, 1, 16, 64, 64), PFA, 1, 2, want_snr=True), F_.cfar_ra(x, PFA, 1, 2, want_snr=True)
    assert a.summary.shape == (3, 1, 8) and a.mask.shape == (3, 1, 8, 64, 64)
    assert torch.equal(a.summary.view(3, 8), b.summary) and torch.equal(a.mask.view(-1), b.mask.view(-1)) and torch.equal(a.snr.view(-1), b.snr.view(-1))
    assert torch.equal(b.count, b.summary[:, 0]) and torch.equal(b.doppler, b.summary[:, 7])
    iq = torch.from_numpy(synth.adc_cube_int16(3)).cuda()
    c = preprocessing.cfar_detect(iq)
    d = F_.cfar_ra(preprocessing.fft_chain_loader_means(iq))
    assert c.summary.shape == (1, 8) and torch.equal(c.summary, d.summary) and torch.equal(c.mask, d.mask) and c.snr is None


@gpu
def test_presence_gate_follows_the_rule():
    from hupr_amd import functional as F_
    counts = np.array([[0, 5], [3, 5], [4, 0], [2, 0], [0, 0], [0, 7], [0, 0], [9, 0], [3, 0], [0, 0], [0, 0], [0, 0], [0, 0]], np.float32)
    min_cells, confirm, hold = 3, 2, 2
    want = np.stack([ref.ref_gate(counts[:, l], min_cells, confirm, hold)[0] for l in range(2)], axis=1)
    state = F_.presence_state(2, "cuda")
    got = []
    for c in counts:
        summary = torch.zeros((2, 8), device="cuda")
        summary[:, 0] = torch.from_numpy(c).cuda()
        got.append(F_.presence_update(summary, state, min_cells, confirm, hold).cpu().numpy())
    assert np.array_equal(np.stack(got), want) and want.any() and not want[-1].any()
    finals = [ref.ref_gate(counts[:, l], min_cells, confirm, hold)[1] for l in range(2)]
    assert state.cpu().numpy().tolist() == [list(f) for f in finals]
