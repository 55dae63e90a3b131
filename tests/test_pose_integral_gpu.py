"""GPU (-m gpu): hupr_pose_decode_integral_f32 (csrc/pose_integral.hip) — arg-max, windowed mass centroid, One-Euro filter — against the
fp64 NumPy statement of the rule in include/hupr.h (tests/pose_integral_ref.py; the reference project has no such decode), and every
layer built on it: ``functional.pose_decode_integral``, ``misc.metrics.get_integral_preds``, ``PoseStream(decode="integral")`` and
``Runner.eval`` with ``TEST.decode: integral``.

Bounds.  Offsets (``pose_integral_ref.offset_bound``): a lane adds at most ceil(cells / 64) window cells in sequence, one rounding each
(an addition for m, a fused multiply-add for Mx and My; x - px is an exact integer), then the 6 additions of the wave butterfly:
D = ceil(cells / 64) + 6 roundings of U = 2^-24 (D = 9 at radius 6, 12 at radius 9, 70 for a whole 64 x 64 plane).  The weights are
>= 0, so m errs by at most D U m and a moment by at most D U sum w |x - px|; the quotient adds one rounding.  The offset o = M / m
therefore errs by at most (D + 1) U (sum w |x - px| / m + |o|) to first order; the bound is twice that.  The raw keypoint adds the two
roundings of (px + ox) * ratio: 2 U |position|.  At radius 6 on a 64 x 64 map this is about 3e-6 heat-map px; an indexing, clipping or
ordering error costs 1e-2 or more.  Filter: tests/test_pose_decode_gpu.py's bounds (2e-3 image px on positions, rate_hz times that on
velocities), derived there for 10 Hz, a 1 Hz cut-off and coordinates below 256 — the same filter at the same settings here."""
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import pose_integral_ref as ref
from test_pose_decode_gpu import TOL_FILTER, ref_one_euro
from test_stream_decode_gpu import N as STREAM_FRAMES, _Ctx, _same

pytestmark = pytest.mark.gpu
RATIO = 4.0
NAN = float("nan")


def dev(x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).cuda()              # a copy: the shared inputs are read-only


def decode(maps, radius, ratio=RATIO, **kw):
    from hupr_amd import functional as F_
    return F_.pose_decode_integral(dev(maps), ratio, radius, **kw)


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ---- 1: against the restatement ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bumpy_maps(rows, H, W, radius):
    """A background uniform in [-0.02, 0.03] (negative pixels weigh nothing) and, per row, a Gaussian bump of amplitude 1 and sigma
    max(1, radius / 3): rows 0-3 on the four corner pixels, rows 4-7 on the middle pixel of the four edges, row 8 on the middle of the
    map (a whole window), the rest anywhere with a fraction, edges included — so the window is clipped on every side.  Every third row
    carries a NaN next to its peak.  With the pixels of the placed bumps and the fp64 decode."""
    rng = np.random.RandomState(1000 * H + W)
    maps = rng.uniform(-0.02, 0.03, (rows, H, W))
    special = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2), (W // 2, H // 2)]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    s = max(1.0, radius / 3.0)
    peaks = []
    for r in range(rows):
        cx, cy = special[r] if r < len(special) else (rng.randint(0, W), rng.randint(0, H))
        fx, fy = (0.0, 0.0) if r < len(special) else rng.uniform(-0.4, 0.4, 2)
        maps[r] += np.exp(-((xx - cx - fx) ** 2 + (yy - cy - fy) ** 2) / (2 * s * s))
        if r % 3 == 2:
            maps[r, min(max(cy + (1 if cy < H - 1 else -1), 0), H - 1), cx] = np.nan
        peaks.append((cx, cy))
    maps = maps.astype(np.float32)
    maps.setflags(write=False)
    return maps, np.array(peaks), ref.ref_integral(maps, radius)


@pytest.mark.parametrize("rows,H,W,radius", [(28, 64, 64, 6), (28, 128, 128, 9), (10, 5, 7, 1), (10, 9, 11, 3)],
                         ids=["28x64x64-r6", "28x128x128-r9", "10x5x7-r1", "10x9x11-r3"])
def test_kernel_against_the_fp64_rule(rows, H, W, radius):
    from hupr_amd import functional as F_
    maps, peaks, want = bumpy_maps(rows, H, W, radius)
    heat = dev(maps)
    a_idx, a_mx = F_.argmax_rows(heat.reshape(rows, H * W))
    idx, mx, raw, kp, vel = F_.pose_decode_integral(heat, RATIO, radius)
    assert kp is None and vel is None and idx.dtype == torch.int32 and raw.shape == (rows, 2)
    assert torch.equal(idx, a_idx) and torch.equal(mx, a_mx)
    assert np.array_equal(idx.cpu().numpy(), want["idx"]) and np.array_equal(mx.cpu().numpy(), want["maxval"])
    assert np.array_equal(want["idx"][:9], (peaks[:, 1] * W + peaks[:, 0])[:9])           # the placed peaks sit where they were put
    full = (2 * radius + 1) ** 2
    assert (want["cells"][:8] < full).all() and (want["cells"][:4] == (radius + 1) ** 2).all()      # clipped windows, corners twice
    assert want["cells"][8] == full                                                      # and a whole one
    err, bound = np.abs(f64(raw) - RATIO * want["pos"]), ref.position_bound(want, RATIO)
    print("%d x %d x %d, r = %d: max |fp32 - fp64| %.3e image px, worst err / bound %.3f, largest bound %.3e; offsets up to %.3f px"
          % (rows, H, W, radius, err.max(), (err / bound).max(), bound.max(), np.abs(want["off"]).max()))
    assert (err <= bound).all()
    assert np.abs(want["off"]).max() > 0.3 and bound.max() < 1e-3                        # a real test: the offsets dwarf the bound
    assert (np.abs(want["off"]) <= radius).all()


# ---- 2: edge planes ------------------------------------------------------------------------------------------------------------------------
def test_empty_and_negative_planes_decode_to_the_origin():
    maps = np.zeros((4, 9, 11), dtype=np.float32)
    maps[1] = -np.random.RandomState(0).uniform(0.1, 1.0, (9, 11))
    maps[2] = NAN
    maps[3, 4, 5] = 0.5
    for radius in (0, 1, 3):
        idx, mx, raw, _, _ = decode(maps, radius)
        assert raw[:3].eq(0).all().item() and raw[3].tolist() == [5 * RATIO, 4 * RATIO]
        assert idx[0].item() == 0 and mx[0].item() == 0.0 and mx[1].item() < 0 and idx[3].item() == 4 * 11 + 5
        assert idx[2].item() == 0x7fffffff and mx[2].item() == -float("inf")              # hupr_argmax_rows_f32's bits for an all-NaN row


def test_a_nan_or_a_negative_pixel_in_the_window_weighs_nothing():
    rng = np.random.RandomState(4)
    base = rng.uniform(0.05, 0.3, (6, 9, 11)).astype(np.float32)
    base[:, 4, 5] = 1.0
    holes = [(4, 6), (3, 5), (5, 4), (3, 4), (5, 6), (4, 4)]
    zeroed, nans, negs = base.copy(), base.copy(), base.copy()
    for r, (y, x) in enumerate(holes):
        zeroed[r, y, x], nans[r, y, x], negs[r, y, x] = 0.0, NAN, -7.0
    for radius in (1, 3, 0):
        z, n, g, b = decode(zeroed, radius), decode(nans, radius), decode(negs, radius), decode(base, radius)
        for k in range(3):
            assert torch.equal(z[k], n[k]) and torch.equal(z[k], g[k]), (radius, k)
        assert not torch.equal(z[2], b[2])                                                # the pixel did weigh something
    # an infinite peak: the mass is not finite, the offset (0, 0)
    inf = base.copy()
    inf[:, 4, 5] = float("inf")
    assert torch.equal(decode(inf, 3)[2], torch.tensor([[5 * RATIO, 4 * RATIO]] * 6, device="cuda"))


def test_a_tie_takes_the_first_maximum():
    maps = np.full((2, 9, 11), 0.01, dtype=np.float32)
    maps[0, 2, 3] = maps[0, 6, 8] = 0.9
    maps[0, 2, 4], maps[0, 6, 7] = 0.3, 0.6
    maps[1, 6, 8] = 0.9
    maps[1, 6, 7] = 0.6
    want = ref.ref_integral(maps, 1)
    idx, mx, raw, _, _ = decode(maps, 1)
    assert idx.tolist() == [2 * 11 + 3, 6 * 11 + 8] and want["idx"].tolist() == idx.tolist()
    assert (np.abs(f64(raw) - RATIO * want["pos"]) <= ref.position_bound(want, RATIO)).all()
    assert raw[0, 0].item() > 3 * RATIO and raw[0, 0].item() < 4 * RATIO and raw[1, 0].item() < 8 * RATIO


@pytest.mark.parametrize("H,W", [(64, 64), (9, 11), (5, 7)], ids=["64x64", "9x11", "5x7"])
def test_radius_zero_is_the_whole_plane_and_runs_repeat(H, W):
    maps = np.random.RandomState(H).uniform(-0.1, 1.0, (20, H, W)).astype(np.float32)
    whole = decode(maps, 0)
    for radius in (max(H, W) - 1, max(H, W), 1000, 2 ** 31 - 1):
        for a, b in zip(whole[:3], decode(maps, radius)[:3]):
            assert torch.equal(a, b), radius
    assert not torch.equal(whole[2], decode(maps, 2)[2])                                 # a window is not the plane
    want = ref.ref_integral(maps, 0)
    assert (want["cells"] == H * W).all()
    assert (np.abs(f64(whole[2]) - RATIO * want["pos"]) <= ref.position_bound(want, RATIO)).all()
    # three launches on the same input
    for radius in (0, 2):
        runs = [decode(maps, radius) for _ in range(3)]
        for other in runs[1:]:
            for a, b in zip(runs[0][:3], other[:3]):
                assert torch.equal(a, b)


# ---- 3: it inverts the targets ----------------------------------------------------------------------------------------------------------------
def test_it_returns_the_joints_the_targets_encode():
    """functional.gaussian_targets_subpixel targets decoded at the default radius: the joint, to 0.01 heat-map px (the truncation of the
    Gaussian's tails by its patch; tests/test_pose_integral_cpu.py), for joints whose patch is unclipped: 6 <= joint / 4 <= 57."""
    from hupr_amd import functional as F_
    from hupr_amd.misc.metrics import default_decode_radius, get_integral_preds, get_max_preds
    joints = np.random.RandomState(13).uniform(24.0, 228.0, (8, 14, 2)).astype(np.float32)
    t = F_.gaussian_targets_subpixel(torch.from_numpy(joints).cuda())
    radius = default_decode_radius(64)
    assert radius == 6 and default_decode_radius(128) == 9
    _, mx, raw, _, _ = F_.pose_decode_integral(t, RATIO, radius)
    err = np.sqrt(((f64(raw) - joints.astype(np.float64)) ** 2).sum(axis=-1)) / RATIO
    print("encode -> integral decode: max |error| %.4f heat-map px, mean %.4f" % (err.max(), err.mean()))
    assert err.max() <= 0.01
    assert (mx.cpu().numpy() > 0.93).all()
    # the host decode built on it
    preds, maxvals = get_integral_preds(t, radius)
    coarse, coarse_max = get_max_preds(t)
    assert preds.dtype == np.float32 and preds.shape == (8, 14, 2) and maxvals.shape == (8, 14, 1) and np.array_equal(maxvals, coarse_max)
    assert np.array_equal(preds, F_.pose_decode_integral(t, 1.0, radius)[2].cpu().numpy())
    assert np.abs(preds - coarse).max() <= 0.51 and np.abs(preds.astype(np.float64) - joints / RATIO).max() <= 0.01


# ---- 4: the loss's centroid ---------------------------------------------------------------------------------------------------------------------
def test_whole_plane_decode_is_the_centroid_of_the_coordinate_loss():
    """Strictly positive planes, radius 0: decoded / stride - a = resid (S + eps) / S with resid and scale = 1 / (S + eps) from
    hupr_coord_loss_fwd_f32, a = joint / stride.  Tolerance: this kernel's bound plus the loss kernel's (tests/test_coord_loss_gpu.py:
    resid to 5e-6 (A + |r|) + 1e-7 with A = sum p |x - a| / (S + eps), scale to 5e-6 relative), carried through the right-hand side:
    with T = S + eps, d(r T / (T - eps)) <= dr T / S + |r| dT eps / S^2."""
    from hupr_amd import runtime as rt
    B, K, H, stride, eps = 2, 14, 64, 4.0, 1.0
    rng = np.random.RandomState(5)
    yy, xx = np.mgrid[0:H, 0:H].astype(np.float64)
    planes = rng.uniform(0.01, 0.2, (2, B, K, H, H))
    for p in planes.reshape(-1, H, H):
        cx, cy = rng.uniform(3, H - 4, 2)
        p += 0.8 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 8.0)
    planes = planes.astype(np.float32)
    joints = (stride * rng.uniform(0, H - 1, (B, K, 2))).astype(np.float32)
    p1, p2, dj = dev(planes[0]), dev(planes[1]), dev(joints)
    loss3 = torch.full((3,), NAN, dtype=torch.float32, device="cuda")
    resid = torch.full((2, B, K, 2), NAN, dtype=torch.float32, device="cuda")
    scale = torch.full((2, B, K), NAN, dtype=torch.float32, device="cuda")
    rt.check(rt.lib().hupr_coord_loss_fwd_f32(rt.ptr(p1), rt.ptr(p2), rt.ptr(dj), B, K, H, stride, 0, None, eps, 1.0, 1.0, rt.ptr(loss3),
                                              rt.ptr(resid), rt.ptr(scale), None, rt.stream()))
    _, _, raw, _, _ = decode(planes, 0, ratio=stride)
    assert raw.shape == (2, B, K, 2)
    a = joints.astype(np.float64) / stride
    lhs = f64(raw) / stride - a[None]
    r, T = f64(resid), 1.0 / f64(scale)[..., None]
    S = T - eps
    rhs = r * T / S
    want = ref.ref_integral(planes.reshape(-1, H, H), 0)
    mine = (ref.position_bound(want, stride) / stride).reshape(2, B, K, 2)
    p64 = planes.astype(np.float64)
    g = np.arange(H, dtype=np.float64)
    A = np.stack([(p64.sum(axis=-2) * np.abs(g - a[None, ..., 0:1])).sum(axis=-1), (p64.sum(axis=-1) * np.abs(g - a[None, ..., 1:2])).sum(axis=-1)],
                 axis=-1) / T
    theirs = (5e-6 * (A + np.abs(r)) + 1e-7) * T / S + np.abs(r) * 5e-6 * T * eps / (S * S)
    err = np.abs(lhs - rhs)
    print("decode vs loss centroid: max |difference| %.3e px, worst / bound %.3f (bounds up to %.3e + %.3e); residuals up to %.1f px"
          % (err.max(), (err / (mine + theirs)).max(), mine.max(), theirs.max(), np.abs(r).max()))
    assert np.isfinite(err).all() and (err <= mine + theirs).all()
    assert np.abs(r).max() > 5.0 and (mine + theirs).max() < 1e-2


# ---- 5: noise ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", ref.NOISE_LEVELS)
def test_the_kernel_beats_the_taylor_kernel_under_noise(level):
    """The planes of tests/test_pose_integral_cpu.py through both kernels: the same strict ordering of mean and 99th percentile."""
    from hupr_amd import functional as F_
    planes, centres = ref.noise_case(level)
    heat = dev(planes)
    integral = ref.error_stats(f64(F_.pose_decode_integral(heat, 1.0, 6)[2]), centres)
    taylor = ref.error_stats(f64(F_.pose_decode(heat, 1.0, refine=True)[2]), centres)
    print("noise %.2f on the device: mean (p99) error in heat-map px: Taylor %.3f (%.3f), centroid r = 6 %.3f (%.3f)"
          % ((level,) + taylor + integral))
    assert integral[0] < taylor[0] and integral[1] < taylor[1]


# ---- 6: filter ---------------------------------------------------------------------------------------------------------------------------------
T, FROWS, DROP = 20, 28, 5


@functools.lru_cache(maxsize=None)
def moving_maps():
    """(T, 2 x 14 rows, 16, 16): a Gaussian of sigma 1.5 and amplitude 0.8 per row on a curved path over a floor of 0.01; row DROP
    falls to 0.05 in frames 8-10."""
    yy, xx = np.mgrid[0:16, 0:16].astype(np.float64)
    maps = np.zeros((T, FROWS, 16, 16), dtype=np.float32)
    for t in range(T):
        for r in range(FROWS):
            cx, cy = 7.5 + 4.0 * np.cos(0.2 * t + 0.5 * r), 7.5 + 3.0 * np.sin(0.15 * t + 0.3 * r)
            A = 0.05 if (r == DROP and 8 <= t <= 10) else 0.8
            maps[t, r] = 0.01 + A * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * 1.5 ** 2))
    maps.setflags(write=False)
    return maps


def test_one_euro_filter_follows_the_fp64_recurrence_and_a_lost_joint_holds_its_place():
    from hupr_amd import functional as F_
    from hupr_amd.tools import PoseSmoothing
    sm = PoseSmoothing(10.0, min_cutoff=1.0, beta=0.01, d_cutoff=1.0, min_score=0.1)
    state = F_.pose_filter_state(FROWS, "cuda")
    heat = dev(moving_maps()).view(T, 2, 14, 16, 16)
    seq = []
    for t in range(T):
        idx, mx, raw, kp, vel = F_.pose_decode_integral(heat[t], RATIO, 4, filter_state=state, smoothing=sm)
        plain = F_.pose_decode_integral(heat[t], RATIO, 4)
        assert kp.shape == (2, 14, 2) and vel.shape == (2, 14, 2)
        assert torch.equal(plain[0], idx) and torch.equal(plain[1], mx) and torch.equal(plain[2], raw)      # the filter leaves the decode alone
        seq.append(tuple(a.reshape(FROWS, -1).clone() for a in (mx, raw, kp, vel)) + (state.clone(),))
    mx = np.stack([s[0].cpu().numpy()[:, 0] for s in seq])
    raw = np.stack([s[1].cpu().numpy() for s in seq])
    kp = np.stack([s[2].cpu().numpy() for s in seq])
    vel = np.stack([s[3].cpu().numpy() for s in seq])
    filt64, vel64 = ref_one_euro(raw, mx, sm)
    e_pos, e_vel = np.abs(kp - filt64).max(), np.abs(vel - vel64).max()
    print("One-Euro behind the integral decode, %d frames x %d rows: max |filtered - fp64| %.3e px, max |velocity - fp64| %.3e px/s "
          "(speeds up to %.1f px/s)" % (T, FROWS, e_pos, e_vel, np.abs(vel64).max()))
    assert e_pos <= TOL_FILTER and e_vel <= sm.rate_hz * TOL_FILTER
    assert np.abs(vel64).max() > 5.0 and np.abs(kp - raw).max() > 0.5                    # the joints move and the filter lags
    assert torch.equal(seq[0][2], seq[0][1]) and not seq[0][3].any().item()              # first sample: the raw keypoint, no velocity
    for t in (8, 9, 10):                                                                 # the drop-out holds its place, bit for bit
        assert mx[t, DROP] <= sm.min_score < mx[7, DROP]
        assert torch.equal(seq[t][2][DROP], seq[7][2][DROP]) and not seq[t][3][DROP].any().item()
        assert torch.equal(seq[t][4][DROP], seq[7][4][DROP])
        assert not torch.equal(seq[t][1][DROP], seq[7][1][DROP])                         # the raw keypoint goes on moving
    assert not torch.equal(seq[11][2][DROP], seq[7][2][DROP])                            # and it resumes from the held state
    last = seq[-1]
    assert torch.equal(last[4][:, 0:2], last[2]) and torch.equal(last[4][:, 2:4], last[3]) and last[4][:, 4].eq(1).all().item()


PT, PH, PW = 12, 8, 12
GONE, NEVER, LATE = (3, 8), 13, 20


def _bounce(n, length):
    """0, 1, ..., length - 1, length - 2, ..., 1, 0, 1, ...: a step of one pixel per frame between the two ends."""
    v = n % (2 * (length - 1))
    return v if v < length else 2 * (length - 1) - v


@functools.lru_cache(maxsize=None)
def pixel_maps():
    """(PT, 2 x 14 rows, 8, 12), zero but for one pixel of 0.5 that moves by one pixel per frame, and that pixel's (x, y), (-1, -1) on
    an empty map.  Even rows bounce inside the map and never touch its border; odd rows run along one of its four edges.  Rows GONE
    are empty in frames 4-5, row NEVER in every frame, row LATE before frame 6."""
    maps = np.zeros((PT, FROWS, PH, PW), dtype=np.float32)
    where = np.full((PT, FROWS, 2), -1)
    for t in range(PT):
        for r in range(FROWS):
            if r == NEVER or (r in GONE and 4 <= t <= 5) or (r == LATE and t < 6):
                continue
            if r % 2 == 0:
                x, y = 1 + _bounce(t + r, PW - 2), 1 + _bounce((0 if r % 4 == 0 else t) + r // 2, PH - 2)
            elif r % 4 == 1:
                x, y = _bounce(t + r, PW), (0 if r % 8 == 1 else PH - 1)
            else:
                x, y = (0 if r % 8 == 3 else PW - 1), _bounce(t + r, PH)
            maps[t, r, y, x] = 0.5
            where[t, r] = x, y
    maps.setflags(write=False)
    return maps, where


def test_both_decodes_run_one_filter_on_one_state_layout():
    """On a map that is one pixel, ``pose_decode(refine=False)`` and ``pose_decode_integral(radius=2)`` decode the same raw keypoint
    exactly (offset 0 in both: the window's mass is that pixel), so the One-Euro filter behind them (csrc/pose_filter.h) must give the
    same bits: filtered keypoints, velocity and state in every frame, also after the two state tensors change hands halfway."""
    from hupr_amd import functional as F_
    from hupr_amd.tools import PoseSmoothing
    maps, where = pixel_maps()
    border = (where[..., 0] == 0) | (where[..., 0] == PW - 1) | (where[..., 1] == 0) | (where[..., 1] == PH - 1)
    assert (~border.any(axis=0)).sum() >= FROWS // 2                                      # off the border on at least half the rows
    seen = (where[1:, :, 0] >= 0) & (where[:-1, :, 0] >= 0)
    assert (np.abs(np.diff(where, axis=0)).max(axis=-1)[seen] == 1).all() and seen.sum() > 200         # one pixel per frame
    sm = PoseSmoothing(10.0, beta=0.05)
    heat = dev(maps).view(PT, 2, 14, PH, PW)
    s_taylor, s_integral = F_.pose_filter_state(FROWS, "cuda"), F_.pose_filter_state(FROWS, "cuda")
    seq = []
    for t in range(PT):
        if t == PT // 2:
            s_taylor, s_integral = s_integral, s_taylor
        a = F_.pose_decode(heat[t], RATIO, refine=False, filter_state=s_taylor, smoothing=sm)
        b = F_.pose_decode_integral(heat[t], RATIO, 2, filter_state=s_integral, smoothing=sm)
        for what, u, v in zip(("index", "maximum", "raw keypoints", "filtered keypoints", "velocity"), a, b):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), (what, t)       # bit for bit
        assert torch.equal(s_taylor.view(torch.int32), s_integral.view(torch.int32)), ("state", t)
        want = np.where(where[t] >= 0, where[t], 0).astype(np.float32) * np.float32(RATIO)
        assert np.array_equal(a[2].reshape(FROWS, 2).cpu().numpy(), want), t
        seq.append([x.reshape(FROWS, 2).clone() for x in a[2:]])
    raws, kps, vels = zip(*seq)
    # the filter did something to compare: it lags, it reports speeds, and the special rows took the paths they are there for
    assert max((k - r).abs().max().item() for k, r in zip(kps, raws)) > 1.0 and max(v.abs().max().item() for v in vels) > 5.0
    for r in GONE:
        for t in (4, 5):
            assert torch.equal(kps[t][r], kps[3][r]) and not vels[t][r].any().item() and not raws[t][r].any().item()
        assert not torch.equal(kps[6][r], kps[3][r])
    assert not s_taylor[NEVER].any().item() and all(not k[NEVER].any().item() for k in kps)
    assert not any(k[LATE].any().item() for k in kps[:6]) and torch.equal(kps[6][LATE], raws[6][LATE]) and not vels[6][LATE].any().item()
    assert vels[7][LATE].any().item() and s_taylor[:, 4].tolist() == [0.0 if r == NEVER else 1.0 for r in range(FROWS)]


# ---- 7: the live stream --------------------------------------------------------------------------------------------------------------------------
class _IntegralCtx(_Ctx):
    """tests/test_stream_decode_gpu.py's context with the session's decode arguments as the key."""

    def session(self, new, lanes=1, graph=True):
        from hupr_amd.tools import PoseStream
        kw = dict(new) if new else {}
        if kw.pop("smooth", False):
            kw["smooth"] = self.smoothing()
        return PoseStream(self.model, self.cfg, lanes=lanes, graph=graph, **kw)


PLAIN = (("decode", "integral"),)
SMOOTH = (("decode", "integral"), ("smooth", True))
NARROW = (("decode", "integral"), ("decode_radius", 2), ("smooth", True))


@pytest.fixture(scope="module")
def ctx():
    c = _IntegralCtx()
    yield c
    c.engine.close()


@pytest.mark.parametrize("kind", [PLAIN, SMOOTH, NARROW], ids=["plain", "smooth", "radius2-smooth"])
def test_session_decodes_as_the_function_does(ctx, kind):
    """functional.pose_decode_integral on each emitted gcn_heatmap, with a filter state of its own, gives the session's frames bit for
    bit: 3 silent pushes, 2 eager poses, 7 graph replays, 3 flushed poses."""
    from hupr_amd import functional as F_
    s, frames = ctx.run(kind)
    radius = dict(kind).get("decode_radius", 6)
    assert s._fused and s.decode_radius == radius and len(frames) == STREAM_FRAMES and s._graphs
    smooth = "smooth" in dict(kind)
    state, sm = (F_.pose_filter_state(14, "cuda"), ctx.smoothing()) if smooth else (None, None)
    for pf in frames:
        idx, mx, raw, kp, vel = F_.pose_decode_integral(pf.gcn_heatmap, ctx.ratio, radius, filter_state=state, smoothing=sm)
        assert torch.equal(idx.view(1, 14), pf.indices) and torch.equal(mx.view(1, 14), pf.scores), pf.frame
        assert torch.equal(raw.view(1, 14, 2), pf.raw_keypoints), pf.frame
        if smooth:
            assert torch.equal(kp.view(1, 14, 2), pf.keypoints) and torch.equal(vel.view(1, 14, 2), pf.velocity), pf.frame
        else:
            assert torch.equal(raw.view(1, 14, 2), pf.keypoints) and pf.velocity is None and kp is None, pf.frame
    peaks = [torch.stack([pf.indices % 64, pf.indices // 64], dim=2).float() * ctx.ratio for pf in frames]
    assert any(not torch.equal(pf.raw_keypoints, p) for pf, p in zip(frames, peaks))      # the centroid is not the peak
    assert all((pf.raw_keypoints - p).abs().max().item() <= radius * ctx.ratio for pf, p in zip(frames, peaks))
    if smooth:
        assert any(not torch.equal(pf.raw_keypoints, pf.keypoints) for pf in frames[1:])


def test_graph_equals_eager(ctx):
    _, graph = ctx.run(SMOOTH, graph=True)
    _, eager = ctx.run(SMOOTH, graph=False)
    for a, b in zip(graph, eager):
        _same(a, b, what="integral + smoothing, graph vs eager")


def test_as_many_launches_as_the_subpixel_session(ctx):
    from hupr_amd import runtime as rt
    L = rt.lib()
    counts = {}
    for kind in ((("decode", "subpixel"),), PLAIN, (("decode", "subpixel"), ("smooth", True)), SMOOTH):
        s = ctx.session(kind, graph=False)
        for n in range(6):
            s.push(*ctx.frames(1, n))
        c0 = L.hupr_launch_count()
        assert s.push(*ctx.frames(1, 6)) is not None
        counts[kind] = L.hupr_launch_count() - c0
    torch.cuda.synchronize()
    print("launches of a steady eager push: %s" % sorted(counts.values()))
    assert len(set(counts.values())) == 1


# ---- 8: Runner.eval ------------------------------------------------------------------------------------------------------------------------------
def _eval(tmp_path, monkeypatch, name, **test_keys):
    import yaml
    from hupr_amd import main as hmain
    from hupr_amd.config_tree import CONFIG_DIR
    cfgd = yaml.safe_load(open(os.path.join(CONFIG_DIR, "mscsa_prgcn.yaml")))
    cfgd["DATASET"]["dataDir"] = "synthetic"
    cfgd["TEST"]["batchSize"] = 2
    cfgd["TEST"].update(test_keys)
    for d in ("config", "logs", "visualization"):
        (tmp_path / d).mkdir(exist_ok=True)
    yaml.safe_dump(cfgd, open(tmp_path / "config" / (name + ".yaml"), "w"))
    monkeypatch.chdir(tmp_path)
    hmain.main(["--config", name + ".yaml", "--dir", name, "--synthetic_length", "4", "--eval"])
    return tmp_path / "logs" / name / "test_results.json"


def test_runner_eval_decodes_with_the_centroid_and_prints_the_position_error(tmp_path, monkeypatch, capsys):
    """The evaluation entry point on the synthetic dataset (freshly initialised weights, two batches of two): with ``TEST.decode:
    integral`` the written keypoints are get_integral_preds' at the default radius times the image ratio and the MPJPE line appears;
    with the keys absent the written keypoints are get_max_preds' times the ratio, get_integral_preds is never called and no such
    line is printed."""
    from hupr_amd.misc import losses, metrics
    calls = {"integral": [], "max": []}

    def integral(heat, radius):
        out = metrics.get_integral_preds(heat, radius)
        calls["integral"].append((radius, out[0].copy()))
        return out

    def maxp(heat):
        out = metrics.get_max_preds(heat)
        calls["max"].append(out[0].copy())
        return out

    monkeypatch.setattr(losses, "get_integral_preds", integral)
    monkeypatch.setattr(losses, "get_max_preds", maxp)

    def written(path):
        recs = json.load(open(path))
        assert len(recs) == 4 and all(len(r["keypoints"]) == 42 for r in recs)
        kp = np.array([r["keypoints"] for r in recs]).reshape(4, 14, 3)
        assert (kp[..., 2] == 1.0).all()
        return kp[..., :2]

    plain = written(_eval(tmp_path, monkeypatch, "plain"))
    out = capsys.readouterr().out
    assert "AP: " in out and "MPJPE" not in out and not calls["integral"]
    assert len(calls["max"]) == 4                                        # per batch: the prediction's decode, then the targets'
    assert np.array_equal(plain, np.concatenate(calls["max"][0::2]).astype(np.float64) * 4.0)
    assert np.array_equal(plain, np.round(plain)) and (plain % 4 == 0).all()

    calls["max"].clear()
    got = written(_eval(tmp_path, monkeypatch, "integral", decode="integral"))
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("MPJPE:")]
    assert len(lines) == 1 and re.fullmatch(r"MPJPE: \d+\.\d{3} px \(n = 4\)", lines[0]), out
    assert "AP: " in out
    assert [r for r, _ in calls["integral"]] == [6, 6] and len(calls["max"]) == 2         # the targets' decode is the arg-max still
    want = np.concatenate([p for _, p in calls["integral"]])
    assert want.dtype == np.float32 and np.array_equal(got, (want * np.float32(4.0)).astype(np.float64))
    assert not np.array_equal(got, plain) and np.abs(got - plain).max() <= 6 * 4.0
    # a radius of its own reaches the decode
    calls["integral"].clear()
    _eval(tmp_path, monkeypatch, "whole", decode="integral", decodeRadius=0)
    assert [r for r, _ in calls["integral"]] == [0, 0]
