"""The rule of hupr_pose_track_assoc_f32 (include/hupr.h) restated in NumPy fp64 — the candidates of a heat-map, the association of a
track with one of them, the presence flag — the distractor scenario and the hand-placed multi-peak maps its tests share.  Written
here: the reference project has no tracker.  Imported by tests/test_pose_assoc_cpu.py, tests/test_pose_assoc_gpu.py and
tests/test_stream_assoc_gpu.py; no GPU needed."""
import functools

import numpy as np

import pose_track_ref as ref


# ---- candidates --------------------------------------------------------------------------------------------------------------------------
def local_maxima(h32):
    """(H, W) float32 -> bool (H, W): h[p] > 0 and no neighbour q inside the map stands in front of p (h[q] > h[p], or h[q] == h[p]
    and q < p).  A NaN is no maximum and stands in front of nothing."""
    H, W = h32.shape
    pad = np.full((H + 2, W + 2), -np.inf, dtype=np.float32)
    pad[1:-1, 1:-1] = np.where(np.isnan(h32), np.float32(-np.inf), h32)
    with np.errstate(invalid="ignore"):
        top = h32 > 0
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                q = pad[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
                earlier = dy < 0 or (dy == 0 and dx < 0)
                top &= ~((q > h32) | ((q == h32) & earlier))
    return top


def peak_indices(h32, K, min_separation, peak_ratio):
    """(H, W) float32 -> the pixel indices of the up to K candidates, in the order they are taken."""
    H, W = h32.shape
    flat = h32.reshape(-1)
    clean = np.where(np.isnan(flat), np.float32(-np.inf), flat)
    b = int(np.argmax(clean))                                                   # first maximum wins; a NaN is never the maximum
    best = clean[b]
    if not best > 0:
        return []
    floor = np.float32(peak_ratio) * np.float32(best)                           # the fp32 product
    taken = [b]
    tops = np.flatnonzero(local_maxima(h32).reshape(-1))
    assert b in tops
    for p in tops[np.argsort(-flat[tops], kind="stable")]:                      # value descending, index ascending
        if len(taken) == K or not flat[p] >= floor:
            break
        if all(max(abs(p % W - t % W), abs(p // W - t // W)) > min_separation for t in taken):
            taken.append(int(p))
    return taken


def refine_offset(h32, px, py):
    """The sub-pixel offset of pose_refine.h at pixel (px, py) in fp64 (the rule beside hupr_pose_decode_f32)."""
    H, W = h32.shape
    if not (0 < px < W - 1 and 0 < py < H - 1):
        return np.zeros(2)
    n = h32[py - 1:py + 2, px - 1:px + 2].astype(np.float64)
    with np.errstate(all="ignore"):
        l = np.log(np.maximum(n, 1e-10))                                        # np.maximum hands a NaN on
        if not np.isfinite(l).all():
            return np.zeros(2)
        dx, dy = 0.5 * (l[1, 2] - l[1, 0]), 0.5 * (l[2, 1] - l[0, 1])
        dxx, dyy = l[1, 2] - 2 * l[1, 1] + l[1, 0], l[2, 1] - 2 * l[1, 1] + l[0, 1]
        dxy = 0.25 * (l[2, 2] - l[2, 0] - l[0, 2] + l[0, 0])
        det = dxx * dyy - dxy * dxy
        if dxx < 0 and det > 0:
            t = np.array([-(dyy * dx - dxy * dy) / det, -(dxx * dy - dxy * dx) / det])
        else:
            t = 0.25 * np.array([np.sign(n[1, 2] - n[1, 0]), np.sign(n[2, 1] - n[0, 1])])
    return np.clip(t, -0.5, 0.5) if np.isfinite(t).all() else np.zeros(2)


def ref_peaks(maps, K, min_separation, peak_ratio, ratio, refine=True):
    """maps (rows, H, W) float32 -> dict: idx (rows, K) int, score (rows, K) float32, xy (rows, K, 2) fp64 image pixels, count (rows,),
    mom (rows, K, 4) the fp64 window moments of every candidate; the slots past the count hold zeros."""
    rows, H, W = maps.shape
    out = dict(idx=np.zeros((rows, K), np.int64), score=np.zeros((rows, K), np.float32), xy=np.zeros((rows, K, 2)),
               count=np.zeros(rows, np.int64), mom=np.zeros((rows, K, 4)))
    for r in range(rows):
        taken = peak_indices(maps[r], K, min_separation, peak_ratio)
        out["count"][r] = len(taken)
        for k, p in enumerate(taken):
            off = refine_offset(maps[r], p % W, p // W) if refine else np.zeros(2)
            out["idx"][r, k], out["score"][r, k] = p, maps[r].reshape(-1)[p]
            out["xy"][r, k] = ((p % W + off[0]) * ratio, (p // W + off[1]) * ratio)
    out["mom"] = candidate_moments(maps, out["idx"], out["count"])
    return out


def candidate_moments(maps, idx, count):
    """The fp64 window moments (pose_track_ref.window_moments) of the candidates at pixel indices idx (rows, K) -> (rows, K, 4)."""
    rows, K = idx.shape
    mom = np.zeros((rows, K, 4))
    for k in range(K):
        has = count > k
        if has.any():
            mom[has, k] = ref.window_moments(maps[has], idx[has, k])
    return mom


# ---- association -------------------------------------------------------------------------------------------------------------------------
def ref_assoc(xy, score, count, mom, p, ratio, present=None, rows_per_group=1):
    """The recurrence over the candidates of T frames: xy (T, rows, K, 2), score (T, rows, K), count (T, rows), mom (T, rows, K, 4),
    ``p`` a PoseTracking, ``present`` None or (T, rows / rows_per_group) flags -> pose_track_ref.ref_track's dict plus chosen (T, rows),
    d2 and cost (T, rows, K; NaN where none was computed) and usable (T, rows, K).  fp64, in matrix form."""
    f = np.float64
    T, rows, K = score.shape
    dt = f(1) / f(p.rate_hz)
    F = np.eye(4)
    F[0, 2] = F[1, 3] = dt
    q = f(p.accel_psd)
    Q = np.zeros((4, 4))
    Q[0, 0] = Q[1, 1] = q * dt * dt * dt / f(3)
    Q[0, 2] = Q[2, 0] = Q[1, 3] = Q[3, 1] = q * dt * dt / f(2)
    Q[2, 2] = Q[3, 3] = q * dt
    Hm = np.zeros((2, 4))
    Hm[0, 0] = Hm[1, 1] = 1
    I4, I2 = np.eye(4), np.eye(2)
    gain, floor2 = f(ratio) * f(ratio) * f(p.heatmap_gain), f(p.meas_std) * f(p.meas_std)
    x, P = np.zeros((rows, 4)), np.zeros((rows, 4, 4))
    live, coast = np.zeros(rows, bool), np.zeros(rows, int)
    out = dict(kp=np.zeros((T, rows, 2)), vel=np.zeros((T, rows, 2)), cov=np.zeros((T, rows, 3)), fc=np.zeros((T, rows, 2)),
               status=np.zeros((T, rows), np.int32), chosen=np.full((T, rows), -1, np.int32), d2=np.full((T, rows, K), np.nan),
               cost=np.full((T, rows, K), np.nan), usable=np.zeros((T, rows, K), bool))
    for t in range(T):
        for r in range(rows):
            seen = present is None or present[t, r // rows_per_group] != 0
            zs, Rs, use = [], [], []
            for k in range(int(count[t, r])):
                z = xy[t, r, k].astype(f)
                m, sxx, sxy, syy = mom[t, r, k]
                with np.errstate(all="ignore"):
                    R = gain * np.array([[sxx, sxy], [sxy, syy]]) + floor2 * I2
                zs.append(z)
                Rs.append(R)
                use.append(bool(seen and score[t, r, k] > p.min_score and np.isfinite(z).all() and m > 0 and np.isfinite(R).all()))
                out["usable"][t, r, k] = use[-1]
            code, pick = ref.LOST, -1
            if live[r]:
                xm, Pm = F @ x[r], F @ P[r] @ F.T + Q
                best = np.inf
                for k in range(len(zs)):
                    if not use[k]:
                        continue
                    nu = zs[k] - Hm @ xm
                    S = Hm @ Pm @ Hm.T + Rs[k]
                    det = S[0, 0] * S[1, 1] - S[0, 1] * S[0, 1]
                    if det > 0 and np.isfinite(det):
                        Si = np.array([[S[1, 1], -S[0, 1]], [-S[0, 1], S[0, 0]]]) / det
                        d2 = nu @ Si @ nu
                        out["d2"][t, r, k] = d2
                        if d2 <= f(p.gate):
                            c = d2 + np.log(det)
                            out["cost"][t, r, k] = c
                            if c < best:                                         # a tie goes to the lower k
                                best, pick, pnu, pSi, pR = c, k, nu, Si, Rs[k]
                if pick >= 0:
                    Kg = Pm @ Hm.T @ pSi
                    A = I4 - Kg @ Hm
                    Pn = A @ Pm @ A.T + Kg @ pR @ Kg.T
                    x[r], P[r], coast[r], code = xm + Kg @ pnu, 0.5 * (Pn + Pn.T), 0, ref.UPDATED
                elif coast[r] + 1 > p.max_coast:
                    live[r] = False
                else:
                    x[r], P[r], code = xm, Pm, ref.COASTED_GATED if any(use) else ref.COASTED_MISSING
                    coast[r] += 1
            z0 = zs[0] if zs else np.zeros(2)                                    # no candidate: the (0, 0) of a non-positive maximum
            if not live[r]:
                x[r], P[r], coast[r], pick = 0, 0, 0, -1
                if use and use[0]:
                    x[r, :2] = z0
                    P[r, :2, :2] = Rs[0]
                    P[r, 2, 2] = P[r, 3, 3] = f(p.init_speed_std) * f(p.init_speed_std)
                    live[r], code, pick = True, ref.STARTED, 0
            kp = x[r, :2] if live[r] else z0
            out["kp"][t, r], out["vel"][t, r], out["cov"][t, r] = kp, x[r, 2:], (P[r, 0, 0], P[r, 0, 1], P[r, 1, 1])
            out["fc"][t, r] = kp + x[r, 2:] * f(p.horizon_s)
            out["status"][t, r], out["chosen"][t, r] = code, pick
    iu = np.triu_indices(4)
    out["state"] = np.concatenate([x, P[:, iu[0], iu[1]], live[:, None].astype(f), coast[:, None].astype(f)], axis=1)
    return out


def ref_run(maps, p, ratio=ref.RATIO, K=None, present=None, rows_per_group=1):
    """maps (T, rows, H, W) float32 through the whole restatement (candidates, then association) -> (ref_assoc's dict, the stacked
    ref_peaks dict).  ``K``: p.candidates unless given."""
    K = p.candidates if K is None else K
    per = [ref_peaks(maps[t], K, p.min_separation, p.peak_ratio, ratio) for t in range(maps.shape[0])]
    c = {k: np.stack([o[k] for o in per]) for k in per[0]}
    return ref_assoc(c["xy"], c["score"], c["count"], c["mom"], p, ratio, present, rows_per_group), c


# ---- the distractor scenario -----------------------------------------------------------------------------------------------------------------
DISTRACTED = tuple(range(14))                     # rows 0..13 carry the ghost
CLEAN = tuple(range(14, ref.ROWS))
GHOST_FRAMES = tuple(range(20, 36))               # frames 20..35
GHOST_AMPLITUDE, GHOST_SEED = 1.0, 5


@functools.lru_cache(maxsize=None)
def distractor_scenario():
    """pose_track_ref.scenario(events=False) with a mirrored bump: on rows 0..13 and frames 20..35 a Gaussian of amplitude 1.0 (the
    joint's is 0.8) at (256 - x, y) of the joint's true position plus N(0, 3 pixel) noise from RandomState(5), merged by np.maximum
    -> (maps (T, ROWS, 64, 64) float32, truth (T, ROWS, 2))."""
    maps, truth, _ = ref.scenario(events=False)
    maps = maps.copy()
    rng = np.random.RandomState(GHOST_SEED)
    rows = list(DISTRACTED)
    for t in GHOST_FRAMES:
        ghost = np.stack([256.0 - truth[t, rows, 0], truth[t, rows, 1]], axis=1) + rng.normal(0.0, 3.0, (len(rows), 2))
        bump = ref.gaussian_maps(ghost / ref.RATIO, np.full(len(rows), GHOST_AMPLITUDE))
        maps[t, rows] = np.maximum(maps[t, rows], bump)
    maps.setflags(write=False)
    return maps, truth


def rms(a):
    """Root mean square length of the (..., 2) vectors of ``a``."""
    return float(np.sqrt(np.mean(np.sum(np.asarray(a, dtype=np.float64) ** 2, axis=-1))))


def distractor_errors(kp, truth):
    """-> (rms error on the distracted rows from the first ghost frame on, the same on the untouched rows)."""
    t0 = GHOST_FRAMES[0]
    e = kp[t0:] - truth[t0:]
    return rms(e[:, list(DISTRACTED)]), rms(e[:, list(CLEAN)])


# ---- hand-placed maps ------------------------------------------------------------------------------------------------------------------------
HAND_K, HAND_SEPARATION, HAND_PEAK_RATIO = 4, 2, 0.25
HAND_SHAPES = ((8, 12), (64, 64))


@functools.lru_cache(maxsize=None)
def hand_maps(H, W):
    """-> (maps (9, H, W) float32, expected: per map the list of (x, y) candidates in order), for K = 4, min_separation = 2,
    peak_ratio = 0.25.  At 8 x 12 the interior features sit at the coordinates written here; at 64 x 64 they are shifted by (23, 31)
    — past one lane's first pixels and across rows of the wave's stride — and the border ones stay on the borders."""
    ox, oy = (0, 0) if (H, W) == (8, 12) else (23, 31)
    m = np.zeros((9, H, W), dtype=np.float32)
    want = []

    def put(i, x, y, v):
        m[i, y + oy, x + ox] = v
        return (x + ox, y + oy)

    # 0: an equal-valued 2 x 2 plateau and an equal-valued pixel elsewhere: the plateau's first pixel wins, then the lone pixel
    for x, y in ((2, 2), (3, 2), (2, 3), (3, 3)):
        put(0, x, y, 0.9)
    want.append([(2 + ox, 2 + oy), put(0, 9, 5, 0.9)])
    # 1: a peak exactly min_separation from the maximum is refused, one at min_separation + 1 is taken
    a = put(1, 3, 3, 1.0)
    put(1, 3 + HAND_SEPARATION, 3, 0.8)
    want.append([a, put(1, 3, 3 + HAND_SEPARATION + 1, 0.7)])
    # 2: the maximum in the corner, peaks on the right and on the bottom border
    m[2, 0, 0], m[2, 4, W - 1], m[2, H - 1, 5] = 1.0, 0.8, 0.6
    want.append([(0, 0), (W - 1, 4), (5, H - 1)])
    # 3: a peak under peak_ratio x maximum is no candidate, one just above is
    a = put(3, 4, 4, 1.0)
    put(3, 9, 2, 0.2)
    want.append([a, put(3, 9, 6, 0.26)])
    # 4: a NaN beside a peak neither hides it nor becomes one
    a, b = put(4, 4, 3, 1.0), put(4, 9, 5, 0.7)
    put(4, 5, 3, np.nan)
    put(4, 9, 4, np.nan)
    want.append([a, b])
    # 5: nothing positive
    m[5] = -0.1
    put(5, 6, 4, 0.0)
    want.append([])
    # 6: two smooth bumps (the refinement moves both off their pixels)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for cx, cy, amp in ((3.3, 3.6, 0.9), (8.4, 4.2, 0.6)):
        m[6] += (amp * np.exp(-((xx - cx - ox) ** 2 + (yy - cy - oy) ** 2) / (2 * 1.2 ** 2))).astype(np.float32)
    want.append([(3 + ox, 4 + oy), (8 + ox, 4 + oy)])
    # 7: six separated peaks: the four highest, by value
    vals = {(1, 1): 0.5, (5, 1): 0.9, (9, 1): 0.6, (1, 5): 0.8, (5, 5): 0.4, (9, 5): 0.7}
    for (x, y), v in vals.items():
        put(7, x, y, v)
    want.append([(x + ox, y + oy) for (x, y), v in sorted(vals.items(), key=lambda kv: -kv[1])[:4]])
    # 8: equal maxima far apart: index order
    want.append([put(8, 2, 1, 0.5), put(8, 10, 1, 0.5), put(8, 6, 6, 0.5)])
    m.setflags(write=False)
    return m, want
