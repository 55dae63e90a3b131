"""GPU (-m gpu): hupr_pose_track_f32 (csrc/pose_track.hip) — the decode of hupr_pose_decode_f32, a measurement covariance read off the
heat-map, and a constant-velocity Kalman filter per row — against the NumPy statement of the rule in tests/pose_track_ref.py.

Bounds.  Decode: bit equality with functional.pose_decode.  Window moments: 1e-4 heat-map pixel^2 — 49-term fp32 sums of window-
relative values <= 9 err by at most about 49 x 2^-24 x 9 = 2.6e-5, the bound leaves 4 x.  Filtered keypoints and forecast:
TOL_FILTER = 2e-3 image pixel, the bound of the One-Euro recurrence (tests/test_pose_decode_gpu.py); velocity rate_hz x that.  The
NumPy fp32 run of the restatement differs from the fp64 one by 3.8e-5 pixel and 7.1e-5 pixel / s on the scenario.  Covariance:
relative to the larger variance of the fp64 one; the NumPy fp32 run (window moments included) differs from the fp64 run by
COV_REL_FP32 = 3.02e-7 on the scenario (measured on the CPU, tests/test_pose_track_cpu.py prints it again), and the bound is 16 x
that = 4.83e-6: the kernel contracts to FMAs and may order sums differently from NumPy.  The test prints what the GPU shows.

The scenario (pose_track_ref.scenario, seed 11): in the fp64 run the largest accepted d2 is 4.85 and the smallest refused one 99.3
against the gate of 13.816, so no decision is within 1 % of the gate (asserted).

max_coast: the rule ends a track on the frame it would coast for the (max_coast + 1)-th time in a row, so a joint that disappears
with max_coast = 5 shows five coasts, then LOST."""
import functools

import numpy as np
import pytest
import torch

import pose_track_ref as ref

pytestmark = pytest.mark.gpu
TOL_MOMENT = 1e-4
TOL_FILTER = 2e-3
COV_REL_FP32 = 3.02e-7
TOL_COV_REL = 16 * COV_REL_FP32
OUT = ("idx", "maxval", "raw", "kp", "vel", "cov", "fc", "status")


def tracking(**kw):
    from hupr_amd.tools import PoseTracking
    return PoseTracking(ref.RATE, **dict(dict(accel_psd=100.0, min_score=ref.MIN_SCORE), **kw))


def track(maps, ratio, state, p, refine=True):
    from hupr_amd import functional as F_
    heat = maps if isinstance(maps, torch.Tensor) else torch.from_numpy(np.array(maps)).cuda()
    return dict(zip(OUT, F_.pose_track(heat, ratio, refine=refine, track_state=state, tracking=p)))


# ---- 1: bit anchor ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [False, True], ids=["argmax", "subpixel"])
def test_the_decode_is_pose_decode_bit_for_bit(refine):
    from hupr_amd import functional as F_
    rows, H, W, ratio = 28, 64, 64, 4.0
    maps = np.random.RandomState(3).uniform(-0.2, 1.0, (rows, H, W)).astype(np.float32)
    maps[5].reshape(-1)[[77, 1300, 4000]] = 2.0                # tied maxima: the first wins
    maps[9] = -np.abs(maps[9])                                 # all <= 0 -> (0, 0)
    maps[10] = 0.0
    heat = torch.from_numpy(maps).cuda()
    idx, mx, raw, _, _ = F_.pose_decode(heat, ratio, refine=refine)
    state = F_.pose_track_state(rows, "cuda")
    assert state.shape == (rows, 16) and not state.any().item()
    o = track(heat, ratio, state, tracking(min_score=0.0), refine=refine)
    assert o["idx"].dtype == torch.int32 and o["status"].dtype == torch.int32
    assert torch.equal(o["idx"], idx) and torch.equal(o["maxval"], mx) and torch.equal(o["raw"], raw)
    assert idx[5].item() == 77 and raw[9].tolist() == [0.0, 0.0] and raw[10].tolist() == [0.0, 0.0]
    usable = torch.ones(rows, dtype=torch.bool, device="cuda")
    usable[[9, 10]] = False
    assert torch.equal(o["status"], torch.where(usable, ref.STARTED, ref.LOST).to(torch.int32))
    assert torch.equal(o["kp"], raw) and torch.equal(o["fc"], raw) and not o["vel"].any().item()
    assert (o["cov"][usable][:, [0, 2]] > 0).all().item() and not o["cov"][~usable].any().item()
    assert not state[~usable].any().item() and (state[usable][:, 14] == 1).all().item()
    assert torch.equal(state[usable][:, :2], raw[usable])


# ---- 2: covariance known answers -----------------------------------------------------------------------------------------------------------
def covariance_maps(H, W):
    """One map per case -> (maps, names).  Coordinates (x, y)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    maps, names = [], []

    def add(name, m):
        maps.append(m.astype(np.float32))
        names.append(name)

    cx, cy = 0.47 * W + 0.3, 0.45 * H + 0.1
    add("isotropic sigma 1", 0.9 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 2.0))
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    a, b = (xx - cx) * c + (yy - cy) * s, -(xx - cx) * s + (yy - cy) * c      # along / across the major axis, 30 degrees from x
    add("axes 3 and 1 at 30 degrees", 0.9 * np.exp(-0.5 * (a ** 2 / 9.0 + b ** 2)))
    add("one pixel from the far corner", 0.9 * np.exp(-((xx - (W - 2)) ** 2 + (yy - (H - 2)) ** 2) / (2 * 1.5 ** 2)))
    add("one pixel from the origin", 0.9 * np.exp(-((xx - 1.2) ** 2 + (yy - 0.9) ** 2) / (2 * 1.5 ** 2)))
    add("plateau", np.full((H, W), 0.5))
    m = -0.3 + 1.0 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * 1.2 ** 2))   # negative beyond ~1.9 pixels of the peak
    add("negative surroundings", m)
    return np.stack(maps), names


@pytest.mark.parametrize("H,W", [(64, 64), (8, 12)], ids=["64x64", "8x12"])
def test_measurement_covariance_is_the_window_moments(H, W):
    """On a STARTED frame the covariance is R = ratio^2 gain S + meas_std^2 I.  8 x 12: 96 elements (no multiple of the wave) and
    not square (an x / y or stride mix-up shows)."""
    from hupr_amd import functional as F_
    maps, names = covariance_maps(H, W)
    rows, ratio, ms = len(names), 4.0, 1.5
    o = track(maps, ratio, F_.pose_track_state(rows, "cuda"), tracking(min_score=0.0, meas_std=ms, heatmap_gain=1.0))
    assert (o["status"] == ref.STARTED).all().item()
    idx = o["idx"].cpu().numpy()
    mom = ref.window_moments(maps, idx)
    cov = o["cov"].cpu().numpy().astype(np.float64)
    got = (cov - np.array([ms * ms, 0.0, ms * ms])) / ratio ** 2
    for r, name in enumerate(names):
        print("%-32s peak (%2d, %2d)  got (%.5f, %+.5f, %.5f)  fp64 (%.5f, %+.5f, %.5f)"
              % ((name, idx[r] % W, idx[r] // W) + tuple(got[r]) + tuple(mom[r, 1:])))
    err = np.abs(got - mom[:, 1:]).max()
    print("max |moment - fp64| %.3e heat-map pixel^2" % err)
    assert err <= TOL_MOMENT
    n = dict(zip(names, range(rows)))
    iso, rot = got[n["isotropic sigma 1"]], got[n["axes 3 and 1 at 30 degrees"]]
    assert abs(iso[0] - iso[2]) < 0.05 and abs(iso[1]) < 0.05 and 0.7 < iso[0] < 1.05          # sigma 1 fits the window
    assert rot[1] > 0.2 and rot[0] > rot[2] > 0                                             # the sign and the order of the axes
    assert idx[n["plateau"]] == 0 and abs(got[n["plateau"]][0] - 1.25) < 1e-4                 # 4 x 4 uniform corner: (16 - 1) / 12
    assert abs(got[n["plateau"]][1]) < 1e-4
    assert (maps[n["negative surroundings"]] < 0).sum() > 20 and got[n["negative surroundings"]][0] < 1.2 ** 2
    # heatmap_gain = 0: the constant isotropic R, exactly
    z = track(maps, ratio, F_.pose_track_state(rows, "cuda"), tracking(min_score=0.0, meas_std=ms, heatmap_gain=0.0))
    want = torch.tensor([ms * ms, 0.0, ms * ms], device="cuda").expand(rows, 3)
    assert (z["status"] == ref.STARTED).all().item() and torch.equal(z["cov"], want)


# ---- 3: recurrence ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scenario_on_gpu():
    return torch.from_numpy(np.array(ref.scenario()[0])).cuda()


@functools.lru_cache(maxsize=None)
def gpu_run(horizon_s=0.0, run=0):
    """The scenario through the kernel from a fresh state -> [per frame: dict of cloned outputs and the state after the frame]."""
    from hupr_amd import functional as F_
    heat, p = scenario_on_gpu(), tracking(horizon_s=horizon_s)
    state = F_.pose_track_state(ref.ROWS, "cuda")
    seq = []
    for t in range(ref.T):
        o = track(heat[t], ref.RATIO, state, p)
        o["state"] = state.clone()
        seq.append(o)
    return seq


def stacked(seq, key):
    return np.stack([o[key].cpu().numpy() for o in seq])


@functools.lru_cache(maxsize=None)
def fp64_run(horizon_s=0.0):
    """The restatement fed the GPU's own raw keypoints and maxima and the fp64 window moments of the same float32 maps."""
    seq = gpu_run(horizon_s)
    idx = stacked(seq, "idx")
    mom = np.stack([ref.window_moments(ref.scenario()[0][t], idx[t]) for t in range(ref.T)])
    return ref.ref_track(stacked(seq, "raw"), stacked(seq, "maxval"), mom, tracking(horizon_s=horizon_s), ref.RATIO)


def test_the_recurrence_follows_the_fp64_rule():
    seq, o64, p = gpu_run(0.3), fp64_run(0.3), tracking(horizon_s=0.3)
    status = stacked(seq, "status")
    # the condition on the inputs: no decision of the fp64 run is within 1 % of the gate
    d2 = o64["d2"][o64["usable"] & np.isfinite(o64["d2"])]
    assert d2.size > 1500 and (np.abs(d2 / p.gate - 1.0) > 0.01).all()
    assert np.array_equal(status, o64["status"])                                           # every row, every frame
    e_kp, e_fc = np.abs(stacked(seq, "kp") - o64["kp"]).max(), np.abs(stacked(seq, "fc") - o64["fc"]).max()
    e_vel = np.abs(stacked(seq, "vel") - o64["vel"]).max()
    e_cov = ref.cov_rel_diff(stacked(seq, "cov"), o64["cov"])
    print("Kalman over %d frames x %d rows: max |filtered - fp64| %.3e px, |forecast - fp64| %.3e px, |velocity - fp64| %.3e px/s, "
          "covariance relative %.3e (bound %.3e); statuses %s"
          % (ref.T, ref.ROWS, e_kp, e_fc, e_vel, e_cov, TOL_COV_REL, np.bincount(status.ravel(), minlength=5).tolist()))
    assert e_kp <= TOL_FILTER and e_fc <= TOL_FILTER
    assert e_vel <= p.rate_hz * TOL_FILTER
    assert e_cov <= TOL_COV_REL
    assert np.abs(o64["state"] - seq[-1]["state"].cpu().numpy()).max() <= 1.0               # the layout of the state: x, P, live, coast
    assert np.array_equal(o64["state"][:, 14:], seq[-1]["state"][:, 14:].cpu().numpy())
    # a real test: the joints move, the filter moves the keypoints, and it beats the raw ones
    _, truth, _ = ref.scenario()
    normal = [r for r in range(ref.ROWS) if r not in (ref.DROP, ref.OUTLIER, ref.GONE, ref.NEVER)]
    raw, kp = stacked(seq, "raw"), stacked(seq, "kp")
    assert np.abs(o64["vel"]).max() > 10.0 and np.abs(kp - raw)[:, normal].max() > 1.0
    rms = lambda a: float(np.sqrt(np.mean(np.sum(a.astype(np.float64) ** 2, axis=-1))))
    assert rms((kp - truth)[:, normal]) < rms((raw - truth)[:, normal])
    assert (status[0, normal] == ref.STARTED).all() and (status[1:, normal] == ref.UPDATED).all()

    # the drop-out: it coasts, its keypoints go on moving (One-Euro holds them), and it resumes with an update
    first, last = ref.DROP_FRAMES[0], ref.DROP_FRAMES[-1]
    for t in ref.DROP_FRAMES:
        assert stacked(seq, "maxval")[t, ref.DROP] <= ref.MIN_SCORE and status[t, ref.DROP] == ref.COASTED_MISSING
        assert not np.array_equal(kp[t, ref.DROP], kp[t - 1, ref.DROP])
        assert torch.equal(seq[t]["vel"][ref.DROP], seq[first - 1]["vel"][ref.DROP])         # on the track's own velocity
        assert seq[t]["state"][ref.DROP, 15].item() == t - first + 1
        assert seq[t]["cov"][ref.DROP, 0].item() > seq[t - 1]["cov"][ref.DROP, 0].item()     # and its uncertainty grows
    assert status[last + 1, ref.DROP] == ref.UPDATED and seq[last + 1]["state"][ref.DROP, 15].item() == 0
    # the outlier: refused by the gate, the track stays where it was heading, the next frame updates
    t = ref.OUTLIER_FRAME
    assert status[t, ref.OUTLIER] == ref.COASTED_GATED and status[t + 1, ref.OUTLIER] == ref.UPDATED
    assert np.abs(raw[t, ref.OUTLIER] - kp[t, ref.OUTLIER]).max() > 30.0 and np.abs(kp[t, ref.OUTLIER] - truth[t, ref.OUTLIER]).max() < 10.0
    assert (np.delete(status[:, ref.OUTLIER], [0, t]) == ref.UPDATED).all()
    # gone for ten frames with max_coast = 5: five coasts, LOST until it returns, then a new track from the raw keypoint
    g0 = ref.GONE_FRAMES[0]
    assert p.max_coast == 5 and len(ref.GONE_FRAMES) == 10
    assert status[g0:g0 + 11, ref.GONE].tolist() == [ref.COASTED_MISSING] * 5 + [ref.LOST] * 5 + [ref.STARTED]
    assert status[g0 + 11, ref.GONE] == ref.UPDATED
    for t in range(g0 + 5, g0 + 10):
        assert not seq[t]["state"][ref.GONE].any().item() and torch.equal(seq[t]["kp"][ref.GONE], seq[t]["raw"][ref.GONE])
        assert not seq[t]["vel"][ref.GONE].any().item() and not seq[t]["cov"][ref.GONE].any().item()
    assert torch.equal(seq[g0 + 10]["kp"][ref.GONE], seq[g0 + 10]["raw"][ref.GONE]) and not seq[g0 + 10]["vel"][ref.GONE].any().item()
    # never usable: LOST throughout, the state stays zero
    assert (status[:, ref.NEVER] == ref.LOST).all()
    for o in seq:
        assert not o["state"][ref.NEVER].any().item() and torch.equal(o["kp"][ref.NEVER], o["raw"][ref.NEVER])


def test_a_gated_track_that_runs_out_restarts_in_the_same_frame():
    """max_coast = 1 and a joint that jumps for good: one COASTED_GATED frame, then the old track ends and a new one STARTS from the
    measurement in the same frame.  max_coast = 0: no coasting at all."""
    from hupr_amd import functional as F_
    here, there = np.array([[100.0, 120.0]]), np.array([[180.0, 60.0]])
    amp = np.array([0.8])
    near, far = ref.gaussian_maps(here / ref.RATIO, amp), ref.gaussian_maps(there / ref.RATIO, amp)
    frames = [near, near, near, far, far, far]
    for max_coast, want in ((1, [ref.STARTED, ref.UPDATED, ref.UPDATED, ref.COASTED_GATED, ref.STARTED, ref.UPDATED]),
                            (0, [ref.STARTED, ref.UPDATED, ref.UPDATED, ref.STARTED, ref.UPDATED, ref.UPDATED])):
        state, p = F_.pose_track_state(1, "cuda"), tracking(max_coast=max_coast)
        outs = [track(m, ref.RATIO, state, p) for m in frames]
        assert [o["status"].item() for o in outs] == want, max_coast
        k = want.index(ref.STARTED, 1)
        assert torch.equal(outs[k]["kp"], outs[k]["raw"]) and not outs[k]["vel"].any().item()
        assert np.abs(outs[k]["raw"].cpu().numpy() - there).max() < 0.01
        idx = np.stack([o["idx"].cpu().numpy() for o in outs])
        mom = np.stack([ref.window_moments(m, i) for m, i in zip(frames, idx)])
        o64 = ref.ref_track(np.stack([o["raw"].cpu().numpy() for o in outs]), np.stack([o["maxval"].cpu().numpy() for o in outs]), mom,
                            p, ref.RATIO)
        assert o64["status"][:, 0].tolist() == want


# ---- 4: run to run -----------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_identical_and_a_zeroed_state_starts_again():
    from hupr_amd import functional as F_
    a, b = gpu_run(0.3, run=0), gpu_run(0.3, run=1)
    assert a is not b
    for t in range(ref.T):
        for k in OUT + ("state",):
            assert torch.equal(a[t][k], b[t][k]), (t, k)
    state = a[-1]["state"].clone()
    assert state.any().item()
    state.zero_()
    o = track(scenario_on_gpu()[12], ref.RATIO, state, tracking())
    usable = o["maxval"] > ref.MIN_SCORE
    assert usable.sum().item() == ref.ROWS - 1
    assert torch.equal(o["status"], torch.where(usable, ref.STARTED, ref.LOST).to(torch.int32))
    assert torch.equal(o["kp"], o["raw"]) and not o["vel"].any().item()


# ---- 5: horizon -----------------------------------------------------------------------------------------------------------------------------------
def test_the_forecast_is_the_keypoint_plus_horizon_times_velocity():
    zero, ahead = gpu_run(0.0), gpu_run(0.3)
    moved = 0.0
    for t in range(ref.T):
        assert torch.equal(zero[t]["fc"], zero[t]["kp"]), t
        for k in ("kp", "vel", "cov", "status", "state"):                                  # the horizon touches the forecast only
            assert torch.equal(zero[t][k], ahead[t][k]), (t, k)
        kp, vel, fc = (ahead[t][k].cpu().numpy().astype(np.float64) for k in ("kp", "vel", "fc"))
        ulp = np.spacing(np.abs(ahead[t]["fc"].cpu().numpy()))
        assert (np.abs((fc - kp) - float(np.float32(0.3)) * vel) <= ulp).all(), t
        moved = max(moved, np.abs(fc - kp).max())
    assert moved > 3.0
