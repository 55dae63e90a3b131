"""GPU (-m gpu): hupr_pose_decode_f32 (csrc/pose_decode.hip) — arg-max, sub-pixel refinement, One-Euro filter — against an fp64 NumPy
statement of the rule in include/hupr.h, written here (the reference project has no such decode), and the host-decode path built on
it (misc.metrics.get_final_preds, TEST.decode).  Section 8: every wrapper that takes ``out=`` (the decodes, the tracker, arg-max, the
presence gate) writes the allocating call's bits into the caller's buffers, in one launch and without an allocation.

Bounds.  Positions: 1e-3 heat-map pixel.  With inputs >= 1e-3 the logs are below 8 in magnitude, so a 2-ulp logf error is <= 1e-6;
the gradient error is then <= 1e-6, the Hessian error <= 4e-6, and with the smallest Hessian eigenvalue >= 0.02 the offset error is
<= 1.5e-4: the bound is about 7 x that, and any indexing or sign error costs >= 0.05.  Filter: 2e-3 image pixel — a step rounds by
<= ~6e-5 at coordinates below 256, the recurrence contracts by alpha >= 0.386 (10 Hz, 1 Hz cut-off), so the error stays <= 2e-4; the
bound is 10 x that.  Velocity: it is the filtered difference of positions times rate_hz, so its error is rate_hz times a position
error: the bound is rate_hz x 2e-3 = 2e-2 pixel / s at 10 Hz."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL_PX = 1e-3
TOL_FILTER = 2e-3


# ---- the rule in fp64 ----------------------------------------------------------------------------------------------------------------
def ref_decode(h32, refine=True):
    """h32 (rows, H, W) float32 -> dict of (rows, ...) fp64 arrays: idx, maxval, pos (x, y in heat-map pixels), off, and per row whether
    it took the Taylor branch and whether it is borderline (|dxx| or |det| < 1e-4, or an unclamped Taylor offset within 1e-3 of
    +-0.5: the fp32 kernel may legitimately take the other branch there)."""
    h = np.asarray(h32, dtype=np.float64)
    rows, H, W = h.shape
    out = dict(idx=np.zeros(rows, np.int64), maxval=np.zeros(rows), pos=np.zeros((rows, 2)), off=np.zeros((rows, 2)),
               taylor=np.zeros(rows, bool), borderline=np.zeros(rows, bool))
    for r in range(rows):
        flat = h[r].reshape(-1)
        i = int(np.argmax(np.where(np.isnan(flat), -np.inf, flat)))      # first maximum wins; a NaN is never the maximum
        mx = flat[i]
        px, py = i % W, i // W
        out["idx"][r], out["maxval"][r] = i, mx
        if not mx > 0:
            continue                                          # (0, 0)
        off = np.zeros(2)
        if refine and 0 < px < W - 1 and 0 < py < H - 1:
            n = h[r, py - 1:py + 2, px - 1:px + 2]            # n[y, x]
            with np.errstate(all="ignore"):
                l = np.log(np.maximum(n, 1e-10))              # np.maximum hands a NaN on
            if np.isfinite(l).all():
                dx, dy = 0.5 * (l[1, 2] - l[1, 0]), 0.5 * (l[2, 1] - l[0, 1])
                dxx, dyy = l[1, 2] - 2 * l[1, 1] + l[1, 0], l[2, 1] - 2 * l[1, 1] + l[0, 1]
                dxy = 0.25 * (l[2, 2] - l[2, 0] - l[0, 2] + l[0, 0])
                det = dxx * dyy - dxy * dxy
                out["borderline"][r] = abs(dxx) < 1e-4 or abs(det) < 1e-4
                with np.errstate(all="ignore"):
                    if dxx < 0 and det > 0:
                        t = np.array([-(dyy * dx - dxy * dy) / det, -(dxx * dy - dxy * dx) / det])
                        out["taylor"][r] = True
                        out["borderline"][r] |= bool((np.abs(np.abs(t) - 0.5) < 1e-3).any())
                    else:
                        t = 0.25 * np.array([np.sign(n[1, 2] - n[1, 0]), np.sign(n[2, 1] - n[0, 1])])
                if np.isfinite(t).all():
                    off = np.clip(t, -0.5, 0.5)
        out["off"][r] = off
        out["pos"][r] = (px + off[0], py + off[1])
    return out


def ref_one_euro(raw, maxval, sm, state=None):
    """fp64 One-Euro filter over raw (T, rows, 2) keypoints and (T, rows) maxima -> (filtered, velocity), both (T, rows, 2)."""
    T, rows, _ = raw.shape
    alpha = lambda fc: 1.0 / (1.0 + sm.rate_hz / (2.0 * np.pi * fc))
    x = np.zeros((rows, 2))
    v = np.zeros((rows, 2))
    valid = np.zeros(rows, bool)
    filt, vel = np.zeros((T, rows, 2)), np.zeros((T, rows, 2))
    for t in range(T):
        for r in range(rows):
            p = raw[t, r].astype(np.float64)
            if maxval[t, r] <= sm.min_score or not np.isfinite(p).all():
                filt[t, r] = x[r] if valid[r] else p
                continue
            if not valid[r]:
                x[r], v[r], valid[r] = p, 0.0, True
            else:
                d = (p - x[r]) * sm.rate_hz
                v[r] = alpha(sm.d_cutoff) * d + (1 - alpha(sm.d_cutoff)) * v[r]
                a = alpha(sm.min_cutoff + sm.beta * np.abs(v[r]))
                x[r] = a * p + (1 - a) * x[r]
            filt[t, r], vel[t, r] = x[r], v[r]
    return filt, vel


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def gaussians(rows, H, W, sigma, seed):
    """A exp(-r^2 / 2 sigma^2), centres uniform in [2, W-3] x [2, H-3], A in [0.02, 0.98] -> (float32 maps, fp64 centres (x, y))."""
    rng = np.random.RandomState(seed)
    cx, cy = rng.uniform(2, W - 3, rows), rng.uniform(2, H - 3, rows)
    A = rng.uniform(0.02, 0.98, rows)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    r2 = (xx[None] - cx[:, None, None]) ** 2 + (yy[None] - cy[:, None, None]) ** 2
    return (A[:, None, None] * np.exp(-r2 / (2.0 * sigma ** 2))).astype(np.float32), np.stack([cx, cy], axis=1)


@functools.lru_cache(maxsize=None)
def smooth_maps(rows=112):
    """Random smooth maps with several competing peaks: a standard-normal 64 x 64 field per row (NumPy seed 0), blurred separably
    with the normalised Gaussian taps -6..6 of sigma 2 (zeros outside the map), then sigmoid(12 z - 4).  With its fp64 decode."""
    z = np.random.RandomState(0).standard_normal((rows, 64, 64))
    taps = np.exp(-np.arange(-6, 7) ** 2 / (2.0 * 2.0 ** 2))
    taps /= taps.sum()
    z = np.apply_along_axis(lambda a: np.convolve(a, taps, mode="same"), 2, z)
    z = np.apply_along_axis(lambda a: np.convolve(a, taps, mode="same"), 1, z)
    maps = (1.0 / (1.0 + np.exp(-(12.0 * z - 4.0)))).astype(np.float32)
    maps.setflags(write=False)
    return maps, ref_decode(maps)


def decode(maps, ratio, refine=True, **kw):
    from hupr_amd import functional as F_
    return F_.pose_decode(torch.from_numpy(np.array(maps)).cuda(), ratio, refine=refine, **kw)


# ---- 1: bit anchor ----------------------------------------------------------------------------------------------------------------------
def test_without_refinement_it_is_argmax_rows_and_stream_keypoints_bit_for_bit():
    from hupr_amd import functional as F_, runtime as rt
    rows, H, W, ratio = 28, 64, 64, 4.0
    maps = np.random.RandomState(3).uniform(-0.2, 1.0, (rows, H, W)).astype(np.float32)
    maps[5].reshape(-1)[[77, 1300, 4000]] = 2.0                # tied maxima: the first wins
    maps[9] = -np.abs(maps[9])                                 # all <= 0 -> (0, 0)
    maps[10] = 0.0
    heat = torch.from_numpy(maps).cuda()
    idx, mx = F_.argmax_rows(heat.reshape(rows, H * W))
    kp = torch.empty((rows, 2), dtype=torch.float32, device="cuda")
    rt.check(rt.lib().hupr_stream_keypoints_f32(rt.ptr(idx), rt.ptr(mx), rt.ptr(kp), rows, W, ratio, rt.stream()))
    got_idx, got_mx, got_kp, filt, vel = F_.pose_decode(heat, ratio, refine=False)
    assert filt is None and vel is None
    assert got_idx.dtype == torch.int32 and torch.equal(got_idx, idx) and torch.equal(got_mx, mx) and torch.equal(got_kp, kp)
    assert idx[5].item() == 77 and kp[9].tolist() == [0.0, 0.0] and kp[10].tolist() == [0.0, 0.0]
    assert kp.abs().sum().item() > 0
    # the arg-max half is the same with refinement on
    r_idx, r_mx, r_kp, _, _ = F_.pose_decode(heat, ratio, refine=True)
    assert torch.equal(r_idx, idx) and torch.equal(r_mx, mx)
    assert (r_kp - kp).abs().max().item() <= 0.5 * ratio


# ---- 2: known answer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(64, 64), (8, 12)], ids=["64x64", "8x12"])
@pytest.mark.parametrize("sigma", [1, 2, 3])
def test_gaussian_centres_are_recovered(sigma, H, W):
    """The Taylor step is exact on a Gaussian: the decoded position is the centre, to 1e-3 heat-map pixel.  8 x 12: 96 elements (no
    multiple of the wave) and not square (an x / y or stride mix-up shows)."""
    maps, centres = gaussians(56, H, W, sigma, seed=10 * sigma + H)
    ratio = 4.0
    _, mx, kp, _, _ = decode(maps, ratio)
    got = kp.cpu().numpy().astype(np.float64) / ratio
    err = np.abs(got - centres).max()
    ref = ref_decode(maps)
    print("sigma %d, %d x %d: max |decoded - centre| %.3e px, |fp64 rule - centre| %.3e px" % (sigma, H, W, err, np.abs(ref["pos"] - centres).max()))
    assert ref["taylor"].all()
    assert err <= TOL_PX
    assert np.abs(got - np.round(got)).max() > 0.1              # sub-pixel positions indeed


# ---- 3: against fp64 on random maps --------------------------------------------------------------------------------------------------------
def test_random_smooth_maps_match_the_fp64_rule():
    maps, ref = smooth_maps()
    ratio = 4.0
    idx, mx, kp, _, _ = decode(maps, ratio)
    assert np.array_equal(idx.cpu().numpy(), ref["idx"]) and np.array_equal(mx.cpu().numpy().astype(np.float64), ref["maxval"])
    got = kp.cpu().numpy().astype(np.float64) / ratio
    keep = ~ref["borderline"]
    excluded = int((~keep).sum())
    err = np.abs(got - ref["pos"])[keep].max()
    print("%d rows: %d excluded as borderline, %d Taylor / %d quarter or zero; max |fp32 - fp64| %.3e px"
          % (len(keep), excluded, int(ref["taylor"].sum()), int((~ref["taylor"]).sum()), err))
    assert excluded <= 0.05 * len(keep)
    assert err <= TOL_PX
    assert ref["taylor"].sum() >= len(keep) // 2                 # the maps exercise the refinement
    assert np.abs(got - ref["pos"]).max() <= 1.0                 # an excluded row is still a neighbour of its peak


# ---- 4: every branch, constructed ------------------------------------------------------------------------------------------------------------
def _patch(m, px, py, n):
    m[py - 1:py + 2, px - 1:px + 2] = np.asarray(n, dtype=np.float32)


def constructed_maps():
    """8 x 8 maps, one per branch -> (maps, expected (x, y) in heat-map pixels, names).  Peak value 0.9 at (x, y) = (3, 4) unless said."""
    maps, want, names = [], [], []

    def add(name, m, xy):
        maps.append(m.astype(np.float32))
        want.append(xy)
        names.append(name)

    bg = lambda: np.full((8, 8), 0.1, dtype=np.float32)
    m = bg(); m[7, 7] = 0.9; add("corner", m, (7.0, 7.0))
    m = bg(); m[0, 0] = 0.9; add("corner at the origin", m, (0.0, 0.0))
    m = bg(); m[0, 3] = 0.9; m[1, 3] = 0.5; m[0, 2] = 0.8; add("edge y = 0", m, (3.0, 0.0))
    m = bg(); m[4, 7] = 0.9; m[4, 6] = 0.8; add("edge x = W - 1", m, (7.0, 4.0))
    # saddle: both axes concave, the cross term dominates (det < 0) -> quarter rule.  The four axis neighbours all equal: sign(0) = 0
    m = bg(); _patch(m, 3, 4, [[0.89, 0.89, 1e-6], [0.89, 0.9, 0.89], [1e-6, 0.89, 0.89]]); add("saddle, equal neighbours", m, (3.0, 4.0))
    # the same saddle with the axis neighbours apart: +-0.25
    m = bg(); _patch(m, 3, 4, [[0.89, 0.89, 1e-6], [0.88, 0.9, 0.89], [1e-6, 0.88, 0.89]]); add("saddle, quarter rule", m, (3.25, 3.75))
    m = bg(); _patch(m, 3, 4, [[0.89, 0.88, 1e-6], [0.89, 0.9, 0.88], [1e-6, 0.89, 0.89]]); add("saddle, quarter rule mirrored", m, (2.75, 4.25))
    # plateau tie on the x axis only
    m = bg(); _patch(m, 3, 4, [[0.89, 0.88, 1e-6], [0.89, 0.9, 0.89], [1e-6, 0.89, 0.89]]); add("plateau on x", m, (3.0, 4.25))
    # steep one-sided peak: the right neighbour ties the peak (the first maximum wins), the left one is far down: the 1-D Taylor step
    # is 0.5 (l[x+1] - l[x-1]) / (l[x] - l[x-1]) = exactly +0.5, on either axis.  (A neighbour that ties the peak on the low side
    # would be the peak itself, so -0.5 is reached through the clamp only: below.)
    m = bg(); _patch(m, 3, 4, [[0.1, 0.5, 0.1], [1e-6, 0.9, 0.9], [0.1, 0.5, 0.1]]); add("one-sided +0.5 on x", m, (3.5, 4.0))
    m = bg(); _patch(m, 3, 4, [[0.1, 1e-6, 0.1], [0.5, 0.9, 0.5], [0.1, 0.9, 0.1]]); add("one-sided +0.5 on y", m, (3.0, 4.5))
    # Taylor step far outside the pixel (dxx = dyy = -1, dxy = +-0.9, gradient 0.4): clamped to +-0.5
    e = lambda v: 0.9 * np.exp(v)
    m = bg() * 0.01; _patch(m, 3, 4, [[e(-0.2), e(-0.9), e(-2.0)], [e(-0.9), 0.9, e(-0.1)], [e(-2.0), e(-0.1), e(-0.2)]]); add("clamped ++", m, (3.5, 4.5))
    m = bg() * 0.01; _patch(m, 3, 4, [[e(-2.0), e(-0.9), e(-0.2)], [e(-0.1), 0.9, e(-0.9)], [e(-0.2), e(-0.1), e(-2.0)]]); add("clamped -+", m, (2.5, 4.5))
    m = bg() * 0.01; _patch(m, 3, 4, [[e(-0.2), e(-0.1), e(-2.0)], [e(-0.1), 0.9, e(-0.9)], [e(-2.0), e(-0.9), e(-0.2)]]); add("clamped --", m, (2.5, 3.5))
    m = bg(); _patch(m, 3, 4, [[0.5, 0.5, 0.5], [0.5, 0.9, np.nan], [0.5, 0.5, 0.5]]); add("NaN neighbour", m, (3.0, 4.0))
    m = bg(); _patch(m, 3, 4, [[np.nan, 0.5, 0.5], [0.4, 0.9, 0.6], [0.5, 0.5, 0.5]]); add("NaN corner", m, (3.0, 4.0))
    add("all zero", np.zeros((8, 8)), (0.0, 0.0))
    m = -bg(); m[4, 3] = -0.01; add("all negative", m, (0.0, 0.0))
    return np.stack(maps), np.asarray(want, dtype=np.float64), names


def test_every_branch_on_constructed_maps():
    maps, want, names = constructed_maps()
    ratio = 4.0
    ref = ref_decode(maps)
    idx, mx, kp, _, _ = decode(maps, ratio)
    got = kp.cpu().numpy().astype(np.float64) / ratio
    for r, name in enumerate(names):
        print("%-32s idx %2d  got (%.4f, %.4f)  want (%.4f, %.4f)  fp64 rule (%.4f, %.4f)" % ((name, idx[r].item()) + tuple(got[r]) + tuple(want[r]) + tuple(ref["pos"][r])))
    for r, name in enumerate(names):
        assert np.array_equal(ref["pos"][r], want[r]), (name, "the fp64 rule and the hand-worked answer differ")
        assert np.array_equal(got[r], want[r]), name               # offsets 0, +-0.25, +-0.5: exact in fp32
    assert np.array_equal(idx.cpu().numpy(), ref["idx"])


# ---- 5: filter -------------------------------------------------------------------------------------------------------------------------------
T, FROWS, DROP, NEVER = 24, 28, 5, 9


@functools.lru_cache(maxsize=None)
def moving_maps():
    """(T, 2 x 14 rows, 16, 16): a Gaussian of sigma 1.5 and amplitude 0.8 per row on a curved path; row DROP falls to 0.05 in frames
    8-10, row NEVER stays there throughout."""
    yy, xx = np.mgrid[0:16, 0:16].astype(np.float64)
    maps = np.zeros((T, FROWS, 16, 16), dtype=np.float32)
    for t in range(T):
        for r in range(FROWS):
            cx, cy = 7.5 + 4.0 * np.cos(0.2 * t + 0.5 * r), 7.5 + 3.0 * np.sin(0.15 * t + 0.3 * r)
            A = 0.05 if (r == NEVER or (r == DROP and 8 <= t <= 10)) else 0.8
            maps[t, r] = A * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * 1.5 ** 2))
    maps.setflags(write=False)
    return maps


def run_filter(sm, state):
    from hupr_amd import functional as F_
    heat = torch.from_numpy(np.array(moving_maps())).cuda().view(T, 2, 14, 16, 16)
    seq = []
    for t in range(T):
        idx, mx, raw, kp, vel = F_.pose_decode(heat[t], 4.0, refine=True, filter_state=state, smoothing=sm)
        seq.append(tuple(a.reshape(FROWS, -1).clone() for a in (mx, raw, kp, vel)) + (state.clone(),))
    return seq


def test_one_euro_filter_follows_the_fp64_recurrence():
    from hupr_amd import functional as F_
    from hupr_amd.tools import PoseSmoothing
    sm = PoseSmoothing(10.0, min_cutoff=1.0, beta=0.01, d_cutoff=1.0, min_score=0.1)
    state = F_.pose_filter_state(FROWS, "cuda")
    assert state.shape == (FROWS, 8) and not state.any().item()
    seq = run_filter(sm, state)
    mx = np.stack([s[0].cpu().numpy()[:, 0] for s in seq])
    raw = np.stack([s[1].cpu().numpy() for s in seq])
    kp = np.stack([s[2].cpu().numpy() for s in seq])
    vel = np.stack([s[3].cpu().numpy() for s in seq])
    filt64, vel64 = ref_one_euro(raw, mx, sm)
    e_pos, e_vel = np.abs(kp - filt64).max(), np.abs(vel - vel64).max()
    print("One-Euro over %d frames x %d rows: max |filtered - fp64| %.3e px, max |velocity - fp64| %.3e px/s (speeds up to %.1f px/s)"
          % (T, FROWS, e_pos, e_vel, np.abs(vel64).max()))
    assert e_pos <= TOL_FILTER
    assert e_vel <= sm.rate_hz * TOL_FILTER
    assert np.abs(vel64).max() > 5.0 and np.abs(kp - raw).max() > 0.5           # the joints move and the filter lags: a real test
    # first sample: the raw keypoint, no velocity
    assert torch.equal(seq[0][2], seq[0][1]) and not seq[0][3].any().item()
    # drop-out of row DROP in frames 8-10: it holds the last filtered value bit for bit, reports no velocity, keeps its state
    for t in (8, 9, 10):
        assert mx[t, DROP] <= sm.min_score < mx[7, DROP]
        assert torch.equal(seq[t][2][DROP], seq[7][2][DROP]) and not seq[t][3][DROP].any().item()
        assert torch.equal(seq[t][4][DROP], seq[7][4][DROP])
        assert not torch.equal(seq[t][1][DROP], seq[7][1][DROP])                # the raw keypoint goes on moving
        others = [r for r in range(FROWS) if r not in (DROP, NEVER)]
        assert not torch.equal(seq[t][4][others], seq[t - 1][4][others])        # every other row advances
    assert not torch.equal(seq[11][2][DROP], seq[7][2][DROP])                   # and it resumes from the held state
    # a joint that was never seen: raw keypoints out, state still zero
    for t in range(T):
        assert torch.equal(seq[t][2][NEVER], seq[t][1][NEVER]) and not seq[t][3][NEVER].any().item()
        assert not seq[t][4][NEVER].any().item()
    # state layout: (x^, y^, dx^, dy^, valid, pad)
    last = seq[-1]
    assert torch.equal(last[4][:, 0:2], torch.where(last[4][:, 4:5] != 0, last[2], torch.zeros_like(last[2])))
    assert torch.equal(last[4][DROP, 2:4], last[3][DROP]) and last[4][DROP, 4].item() == 1.0
    # after zero-filling the state the first output is the raw keypoint again
    state.zero_()
    idx, _, raw0, kp0, vel0 = F_.pose_decode(torch.from_numpy(np.array(moving_maps()[12])).cuda(), 4.0, filter_state=state, smoothing=sm)
    assert torch.equal(kp0, raw0) and not vel0.any().item()


# ---- 6: run to run ----------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_identical():
    from hupr_amd import functional as F_
    from hupr_amd.tools import PoseSmoothing
    maps, _ = smooth_maps()
    a, b = decode(maps, 4.0), decode(maps, 4.0)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    sm = PoseSmoothing(10.0, min_score=0.1)
    s1, s2 = run_filter(sm, F_.pose_filter_state(FROWS, "cuda")), run_filter(sm, F_.pose_filter_state(FROWS, "cuda"))
    for t in range(T):
        for x, y in zip(s1[t], s2[t]):
            assert torch.equal(x, y), t


# ---- 7: host-decode path ------------------------------------------------------------------------------------------------------------------------
def test_get_final_preds_and_test_decode():
    from hupr_amd import functional as F_, synth
    from hupr_amd.config_tree import load_config
    from hupr_amd.misc.losses import LossComputer
    from hupr_amd.misc.metrics import get_final_preds, get_max_preds
    maps, ref = smooth_maps()
    heat = torch.from_numpy(maps[:28].copy()).cuda().view(2, 14, 64, 64)
    preds, maxvals = get_final_preds(heat)
    coarse, coarse_max = get_max_preds(heat)
    _, mx, raw, _, _ = F_.pose_decode(heat, 1.0)
    assert preds.dtype == np.float32 and preds.shape == (2, 14, 2) and maxvals.shape == (2, 14, 1)
    assert np.array_equal(preds, raw.cpu().numpy()) and np.array_equal(maxvals, coarse_max)
    assert np.abs(preds - coarse).max() <= 0.5 and not np.array_equal(preds, coarse)
    assert np.abs(preds.reshape(28, 2) - ref["pos"][:28])[~ref["borderline"][:28]].max() <= TOL_PX

    cfg = load_config()
    sub = copy.deepcopy(cfg)
    sub.TEST.decode = "subpixel"
    gt = torch.from_numpy(synth.keypoints(2, 7))
    p1, p2 = heat.view(2, 14, 1, 64, 64).flip(0).contiguous(), heat.view(2, 1, 14, 64, 64)
    _, _, pred_default, gt_default = LossComputer(cfg, "cuda").computeLoss((p1, p2), gt)
    _, _, pred_sub, gt_sub = LossComputer(sub, "cuda").computeLoss((p1, p2), gt)
    assert np.array_equal(pred_default, coarse) and pred_default.dtype == coarse.dtype
    assert np.array_equal(pred_sub, preds)
    assert np.array_equal(gt_sub, gt_default)                    # the targets' decode is the arg-max either way
    # the device branch of the training step is the arg-max either way
    dev = LossComputer(sub, "cuda").computeLoss((p1, p2), gt, decode="device")[2]
    idx, mxs = F_.argmax_rows(heat.reshape(28, 64 * 64))
    assert torch.equal(dev[0], idx) and torch.equal(dev[1], mxs)


# ---- 8: out= — the wrappers write into buffers the caller owns --------------------------------------------------------------------------------
def _out_cases():
    """name -> (state factory or None, call(heat, state, out)) for every wrapper that takes ``out``: the two decodes with and without
    a filter, the tracker on its two entries, the row arg-max, the presence gate.  No call allocates an input of its own."""
    from hupr_amd import functional as F_
    from hupr_amd.tools import PoseSmoothing, PoseTracking
    sm = PoseSmoothing(10.0, min_score=0.1)
    track = lambda **kw: PoseTracking(10.0, min_score=0.1, horizon_s=0.2, **kw)
    present = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    summary = torch.zeros((2, 8), dtype=torch.float32, device="cuda")           # the gate reads column 0, the detection count
    summary[0, 0] = 5.0                                                          # lane 0 is a hit, lane 1 a miss
    cases = {}
    for refine in (0, 1):
        cases["pose_decode refine=%d" % refine] = (None, lambda h, s, out, r=refine: F_.pose_decode(h, 4.0, refine=bool(r), out=out))
        cases["pose_decode refine=%d filter" % refine] = (F_.pose_filter_state, lambda h, s, out, r=refine: F_.pose_decode(
            h, 4.0, refine=bool(r), filter_state=s, smoothing=sm, out=out))
    for radius in (2, 0):
        cases["pose_decode_integral radius=%d" % radius] = (None, lambda h, s, out, r=radius: F_.pose_decode_integral(h, 4.0, r, out=out))
        cases["pose_decode_integral radius=%d filter" % radius] = (F_.pose_filter_state, lambda h, s, out, r=radius: F_.pose_decode_integral(
            h, 4.0, r, filter_state=s, smoothing=sm, out=out))
    cases["pose_track"] = (F_.pose_track_state, lambda h, s, out: F_.pose_track(h, 4.0, track_state=s, tracking=track(), out=out))
    cases["pose_track candidates=2"] = (F_.pose_track_state, lambda h, s, out: F_.pose_track(h, 4.0, track_state=s,
                                                                                           tracking=track(candidates=2), out=out))
    cases["pose_track present"] = (F_.pose_track_state, lambda h, s, out: F_.pose_track(h, 4.0, track_state=s, tracking=track(),
                                                                                      present=present, out=out))
    cases["argmax_rows"] = (None, lambda h, s, out: F_.argmax_rows(h.view(6, 64), out=out))
    cases["presence_update"] = (lambda rows, dev: F_.presence_state(2, dev), lambda h, s, out: F_.presence_update(
        summary, s, min_cells=3, confirm=1, hold=0, out=out))
    return cases


@pytest.mark.parametrize("name", ["pose_decode refine=0", "pose_decode refine=0 filter", "pose_decode refine=1", "pose_decode refine=1 filter",
                                  "pose_decode_integral radius=2", "pose_decode_integral radius=2 filter", "pose_decode_integral radius=0",
                                  "pose_decode_integral radius=0 filter", "pose_track", "pose_track candidates=2", "pose_track present",
                                  "argmax_rows", "presence_update"])
def test_out_buffers_get_the_allocating_call_s_bits_in_one_launch_and_no_allocation(name):
    """Once allocating, once into sentinel-filled buffers with a clone of the same (already advanced) state: the same bits, the same
    advanced state, the caller's own tensors back, one launch, and not a byte allocated on the device."""
    from hupr_amd import runtime as rt
    new_state, call = _out_cases()[name]
    rng = np.random.RandomState(11)
    warm, heat = (torch.from_numpy(rng.uniform(0.0, 1.0, (2, 3, 8, 8)).astype(np.float32)).cuda() for _ in range(2))
    s1 = s2 = None
    if new_state is not None:
        s1 = new_state(6, "cuda")
        call(warm, s1, None)                                                     # a state that has seen a frame
        s2 = s1.clone()
    want = call(heat, s1, None)
    single = isinstance(want, torch.Tensor)                                      # presence_update returns its one tensor bare
    want = (want,) if single else want
    assert any(t is not None and t.any().item() for t in want)
    bufs = tuple(None if t is None else torch.full_like(t, 77) for t in want)
    torch.cuda.synchronize()
    L = rt.lib()
    n0, m0 = L.hupr_launch_count(), torch.cuda.memory_allocated()
    got = call(heat, s2, bufs[0] if single else bufs)
    assert L.hupr_launch_count() - n0 == 1 and torch.cuda.memory_allocated() == m0
    got = (got,) if single else got
    assert len(got) == len(want)
    for k, (g, b, w) in enumerate(zip(got, bufs, want)):
        assert g is b, k
        assert (g is None and w is None) or (g.dtype == w.dtype and torch.equal(g, w)), k
    if s1 is not None:
        assert torch.equal(s1, s2) and s1.any().item()
