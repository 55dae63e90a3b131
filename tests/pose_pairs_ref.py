"""The rule of hupr_pose_track_pairs_f32 (include/hupr.h) restated in NumPy fp64, in matrix form — the pool of a unit, the admissible
measurements, the joint assignment of two partner tracks, the start rule — the swap scenario and the hand-placed maps its tests share.
It builds on tests/pose_assoc_ref.py (the candidates of a map) and tests/pose_track_ref.py (the scenario).  Written here: the
reference project has no tracker.  Imported by tests/test_pose_pairs_cpu.py and tests/test_pose_pairs_gpu.py; no GPU needed."""
import functools

import numpy as np

import pose_assoc_ref as A
import pose_track_ref as ref

JOINTS = ("R_Hip", "R_Knee", "R_Ankle", "L_Hip", "L_Knee", "L_Ankle", "Neck", "Head", "L_Shoulder", "L_Elbow", "L_Wrist", "R_Shoulder",
          "R_Elbow", "R_Wrist")                       # DATASET.idxToJoints of config/mscsa_prgcn.yaml
GROUP = len(JOINTS)
PARTNER = (3, 4, 5, 0, 1, 2, 6, 7, 11, 12, 13, 8, 9, 10)
PAIRS = ((0, 3), (1, 4), (2, 5), (8, 11), (9, 12), (10, 13))
IDENTITY = tuple(range(GROUP))


def units(partner):
    """The units of one group in the kernel's order: (a, b) with a < b for two partner rows, (a, None) for a row by itself."""
    partner = [int(q) for q in partner]
    assert all(0 <= q < len(partner) and partner[q] == j for j, q in enumerate(partner)), "the partner table is no involution"
    return [(j, q if q > j else None) for j, q in enumerate(partner) if q >= j]


def ref_pairs(xy, score, count, mom, p, ratio, partner, swap_cost=0.0, present=None):
    """The recurrence over the candidates of T frames: xy (T, rows, K, 2), score (T, rows, K), count (T, rows), mom (T, rows, K, 4),
    ``p`` a PoseTracking, ``partner`` the table of one group (rows is a multiple of its length), ``present`` None or (T, groups)
    flags -> pose_assoc_ref.ref_assoc's dict (kp, vel, cov, fc, status, chosen, state, usable) plus source (T, rows), d2 and cost
    (T, rows, 2 K: row r's track against the pool of its unit, its own map's K slots first, then its partner's; NaN where none was
    computed; cost holds swap_cost) and alt (T, rows): per unit, on its first row, the cost of the best assignment of the same
    cardinality that is not the one taken (inf without one; NaN elsewhere).  fp64."""
    f = np.float64
    T, rows, K = score.shape
    G = len(partner)
    assert rows % G == 0
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
               status=np.zeros((T, rows), np.int32), chosen=np.full((T, rows), -1, np.int32), source=np.full((T, rows), -1, np.int32),
               d2=np.full((T, rows, 2 * K), np.nan), cost=np.full((T, rows, 2 * K), np.nan), usable=np.zeros((T, rows, K), bool),
               alt=np.full((T, rows), np.nan))
    group_units = units(partner)
    for t in range(T):
        for g in range(rows // G):
            seen = present is None or present[t, g] != 0
            for ua, ub in group_units:
                members = [g * G + ua] + ([g * G + ub] if ub is not None else [])
                # ---- the pool: (row index inside the unit, slot, z, R, usable), a's candidates first ----------------------------------
                pool = []
                for m, r in enumerate(members):
                    for k in range(K):
                        if k >= count[t, r]:
                            pool.append((m, k, None, None, False))
                            continue
                        z = xy[t, r, k].astype(f)
                        mass, sxx, sxy, syy = mom[t, r, k]
                        with np.errstate(all="ignore"):
                            R = gain * np.array([[sxx, sxy], [sxy, syy]]) + floor2 * I2
                        use = bool(seen and score[t, r, k] > p.min_score and np.isfinite(z).all() and mass > 0 and np.isfinite(R).all())
                        out["usable"][t, r, k] = use
                        pool.append((m, k, z, R, use))
                n = len(pool)
                any_usable = any(e[4] for e in pool)
                # ---- admissible entries and their costs, per live track -----------------------------------------------------------------
                pred, adm = {}, {}
                for m, r in enumerate(members):
                    adm[m] = {}
                    if not live[r]:
                        continue
                    xm, Pm = F @ x[r], F @ P[r] @ F.T + Q
                    pred[m] = (xm, Pm)
                    for e, (em, k, z, R, use) in enumerate(pool):
                        if not use:
                            continue
                        nu = z - Hm @ xm
                        S = Hm @ Pm @ Hm.T + R
                        det = S[0, 0] * S[1, 1] - S[0, 1] * S[0, 1]
                        if det > 0 and np.isfinite(det):
                            Si = np.array([[S[1, 1], -S[0, 1]], [-S[0, 1], S[0, 0]]]) / det
                            d2 = nu @ Si @ nu
                            col = k if em == m else K + k
                            out["d2"][t, r, col] = d2
                            if d2 <= f(p.gate):
                                c = d2 + np.log(det) + (f(swap_cost) if em != m else 0.0)
                                out["cost"][t, r, col] = c
                                adm[m][e] = (c, nu, Si, R)
                # ---- assignment: most tracks, then the smallest sum, then the lexicographically smaller (entry of a, entry of b) ------
                options = []
                for ea in list(adm[0]) + [n]:
                    for eb in (list(adm[1]) if len(members) == 2 else []) + [n]:
                        if ea == eb and ea < n:
                            continue
                        card = (ea < n) + (eb < n)
                        total = (adm[0][ea][0] if ea < n else 0.0) + (adm[1][eb][0] if eb < n else 0.0)
                        options.append((-card, total, ea, eb))
                options.sort()
                _, _, ea, eb = options[0]
                same = [o for o in options[1:] if o[0] == options[0][0]]
                out["alt"][t, members[0]] = same[0][1] - options[0][1] if same else np.inf
                taken = (ea, eb)
                # ---- update or coast ---------------------------------------------------------------------------------------------------------
                codes = {}
                for m, r in enumerate(members):
                    code, e = ref.LOST, taken[m]
                    if live[r]:
                        xm, Pm = pred[m]
                        if e < n:
                            c, nu, Si, R = adm[m][e]
                            Kg = Pm @ Hm.T @ Si
                            Aj = I4 - Kg @ Hm
                            Pn = Aj @ Pm @ Aj.T + Kg @ R @ Kg.T
                            x[r], P[r], coast[r], code = xm + Kg @ nu, 0.5 * (Pn + Pn.T), 0, ref.UPDATED
                            out["chosen"][t, r], out["source"][t, r] = pool[e][1], int(pool[e][0] != m)
                        elif coast[r] + 1 > p.max_coast:
                            live[r] = False
                        else:
                            x[r], P[r], code = xm, Pm, ref.COASTED_GATED if any_usable else ref.COASTED_MISSING
                            coast[r] += 1
                    codes[m] = code
                # ---- start, and the outputs -------------------------------------------------------------------------------------------------
                for m, r in enumerate(members):
                    own0 = pool[m * K]
                    z0 = own0[2] if own0[2] is not None else np.zeros(2)          # no candidate: the (0, 0) of a non-positive maximum
                    if not live[r]:
                        x[r], P[r], coast[r] = 0, 0, 0
                        if own0[4] and m * K not in taken:
                            x[r, :2] = z0
                            P[r, :2, :2] = own0[3]
                            P[r, 2, 2] = P[r, 3, 3] = f(p.init_speed_std) * f(p.init_speed_std)
                            live[r], codes[m] = True, ref.STARTED
                            out["chosen"][t, r], out["source"][t, r] = 0, 0
                    kp = x[r, :2] if live[r] else z0
                    out["kp"][t, r], out["vel"][t, r], out["cov"][t, r] = kp, x[r, 2:], (P[r, 0, 0], P[r, 0, 1], P[r, 1, 1])
                    out["fc"][t, r] = kp + x[r, 2:] * f(p.horizon_s)
                    out["status"][t, r] = codes[m]
    iu = np.triu_indices(4)
    out["state"] = np.concatenate([x, P[:, iu[0], iu[1]], live[:, None].astype(f), coast[:, None].astype(f)], axis=1)
    return out


def candidates(maps, p, ratio=ref.RATIO, K=None):
    """maps (T, rows, H, W) float32 -> the stacked pose_assoc_ref.ref_peaks dict of every frame."""
    K = p.candidates if K is None else K
    per = [A.ref_peaks(maps[t], K, p.min_separation, p.peak_ratio, ratio) for t in range(maps.shape[0])]
    return {k: np.stack([o[k] for o in per]) for k in per[0]}


def ref_run(maps, p, partner=PARTNER, swap_cost=0.0, ratio=ref.RATIO, K=None, present=None, c=None):
    """maps (T, rows, H, W) float32 through the whole restatement (candidates, then the joint assignment) -> (ref_pairs' dict, the
    candidates).  ``c``: candidates computed before, for the same maps and settings."""
    c = candidates(maps, p, ratio, K) if c is None else c
    return ref_pairs(c["xy"], c["score"], c["count"], c["mom"], p, ratio, partner, swap_cost, present), c


# ---- the swap scenario -------------------------------------------------------------------------------------------------------------------
SWAP_FRAMES = tuple(range(20, 36))                # frames 20..35
SWAP_LANE = 0                                     # rows 0..13


def swapped_rows(lane=SWAP_LANE):
    return tuple(lane * GROUP + j for pair in PAIRS for j in pair)


@functools.lru_cache(maxsize=None)
def swap_scenario(frames=SWAP_FRAMES, lane=SWAP_LANE):
    """pose_track_ref.scenario(events=False) = 2 lanes of 14 joints, with the heat-maps of every L_* / R_* pair of ``lane`` exchanged
    in ``frames`` — what a network that mixes up left and right emits -> (maps (T, ROWS, 64, 64) float32, truth (T, ROWS, 2)).
    ``frames=()``: the scenario itself."""
    maps, truth, _ = ref.scenario(events=False)
    maps = maps.copy()
    for t in frames:
        for a, b in PAIRS:
            ra, rb = lane * GROUP + a, lane * GROUP + b
            maps[t, [ra, rb]] = maps[t, [rb, ra]]
    maps.setflags(write=False)
    return maps, truth


def swap_errors(kp, truth, frames=SWAP_FRAMES, lane=SWAP_LANE):
    """-> (rms error on the rows of the swapped pairs from the first swapped frame on, the same on all rows of the other lanes)."""
    t0 = frames[0] if frames else SWAP_FRAMES[0]
    e = np.asarray(kp, dtype=np.float64)[t0:] - truth[t0:]
    rows = list(swapped_rows(lane))
    others = [r for r in range(truth.shape[1]) if r // GROUP != lane]
    return A.rms(e[:, rows]), A.rms(e[:, others])


# ---- hand-placed maps: exclusivity, the start rule, the status ---------------------------------------------------------------------------------
HAND_PARTNER = (1, 0)                             # one group of two partner rows
HAND_H, HAND_W = 8, 12


def hand_bump(x, y, amp=0.8, sigma=1.0):
    yy, xx = np.mgrid[0:HAND_H, 0:HAND_W].astype(np.float64)
    return (amp * np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * sigma ** 2))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def hand_one_peak():
    """Two live tracks and one admissible peak.  Frame 0 starts track 0 at (3, 4) and track 1 at (8, 4) heat-map pixels; in frame 1
    map 0 shows one bump at (5, 4) — between them, nearer to track 0 (2 pixels against 3) — and map 1 nothing above min_score.
    -> maps (2, 2, 8, 12) float32.  Expected: row 0 takes it from its own map, row 1 is COASTED_GATED (a pool entry was usable)."""
    m = np.zeros((2, 2, HAND_H, HAND_W), np.float32)
    m[0, 0], m[0, 1] = hand_bump(3, 4), hand_bump(8, 4)
    m[1, 0], m[1, 1] = hand_bump(5, 4), hand_bump(8, 4, amp=0.05)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def hand_taken_start():
    """A dead row whose candidate 0 was taken by its partner.  Frame 0: map 0 faint (row 0 stays LOST), map 1 starts track 1 at
    (6, 4).  Frame 1: map 0 shows the bump at (6, 4), map 1 is faint: track 1 takes map 0's candidate 0 (source 1), and row 0, which
    has no track, may not start from it: LOST.  Frame 2, the same maps: likewise.
    -> maps (3, 2, 8, 12) float32."""
    m = np.zeros((3, 2, HAND_H, HAND_W), np.float32)
    m[0, 0], m[0, 1] = hand_bump(6, 4, amp=0.05), hand_bump(6, 4)
    for t in (1, 2):
        m[t, 0], m[t, 1] = hand_bump(6, 4), hand_bump(6, 4, amp=0.05)
    m.setflags(write=False)
    return m
