"""Live pose streaming: one hori + vert radar frame in per frame period, one pose out.

The offline route treats every frame like a dataset item: gather its G-frame window (datasets.window_indices), upload and transform
all 2 G sensor-frames, run HuPRNet.  Consecutive windows share all but one frame, and everything in front of the 3-D encoders is a
pure function of ONE sensor-frame (the FFT chain with its frame-keyed dither, the fused loader, the MNet front end on the 16
elevation-mean planes).  ``PoseStream`` therefore keeps a ring of mean planes on the device (256 KB per sensor-frame), transforms only
the new frame, and runs the MNet over the window straight from the ring (csrc/stream_window.hip) — bit-identical to the offline route.

Window rule: ``stream_window_sources(center, newest, G)``.  With ``lookahead = L`` the pose of frame ``n - L`` is emitted once frame
``n`` has been pushed; ``flush()`` emits the last ``min(L, frames pushed)`` poses with ``newest`` held at the last frame.  The default
``L = G // 2 - 1`` reproduces ``window_indices`` for every frame of a sequence; ``L = 0`` answers every push at once, the upper half of
the window repeating the newest frame (what the reference's loader does at the end of a sequence).

The frame and pose counters the kernels read live on the device and are advanced by a launch of their own, so no launch argument
depends on the frame number: with ``graph=True`` the steady-state push is ONE hipGraph replay (upload from pinned staging, FFT chain,
window MNet, state advance, encoders / decoder / heads, arg-max, keypoint decode).

Decode: by default the keypoint is the arg-max pixel times imgSize / heatmapSize, as the reference decodes it.  ``decode="subpixel"``
refines the peak to sub-pixel position and ``smooth=PoseSmoothing(rate_hz)`` runs a One-Euro filter over the keypoints, its state on
the device; either replaces the two decode launches by one (csrc/pose_decode.hip), inside the captured graph like them.
``track=PoseTracking(rate_hz)`` runs a constant-velocity Kalman filter per joint instead (csrc/pose_track.hip, one launch likewise):
outliers are gated, drop-outs coast on the track's velocity, every joint carries a covariance and a forecast.  With
``PoseTracking(candidates=C)``, C > 1, the track chooses its measurement among up to C peaks of the heat-map instead of taking the
strongest (csrc/pose_assoc.hip, one launch in the tracker's place), and ``gate_on_presence=True`` takes the measurement away where the
presence gate sees nobody.  ``PoseTracking(pair_swap=True)`` assigns the left / right partners of the skeleton jointly, each pair
sharing the peaks of both its maps (csrc/pose_pairs.hip, one launch likewise): a left / right exchange by the network is followed.
``PoseTracking(accel_psd_moving=Q)`` runs a still and a moving model per joint and mixes them, the interacting-multiple-model
estimator (csrc/pose_imm.hip, one launch likewise): a joint that rests and reaches gets the right process noise in both regimes.
``decode="integral"`` decodes the mass centroid of the window of ``decode_radius`` pixels around the peak (default: the targets' patch
radius; 0: the whole map) — what the integral coordinate loss trains — in one launch of csrc/pose_integral.hip in place of the two,
``smooth`` included; it does not combine with ``track``, whose measurement is pinned to the sub-pixel decode.

    python -m hupr_amd.tools.stream --config mscsa_prgcn.yaml --dir <logs name> --raw <dir with hori/ and vert/ adc_data.bin>
                                    [--lookahead N] [--math f32|bf16] [--no-graph] [--out poses.json]
                                    [--decode argmax|subpixel|integral [--decode-radius N]] [--smooth --rate FPS]
                                    [--track --rate FPS [--predict-now] [--accel-psd Q] [--gate D2] [--max-coast N] [--rts]
                                     [--track-candidates N] [--track-separation N] [--track-peak-ratio X] [--track-on-presence]
                                     [--track-pairs [--track-swap-cost X]] [--track-lag N]
                                     [--track-moving-psd Q [--track-switch-prob P] [--track-moving-prior M]]]
                                    [--presence [--pfa X] [--cfar-guard N] [--cfar-train N] [--min-cells N] [--confirm N] [--hold N]]

``presence=PresenceGate(...)`` / ``--presence``: scene occupancy.  A CA-CFAR detector on the centre frame's horizontal mean planes and a
presence gate over its detections (csrc/cfar.hip) tell whether a mover stands in front of the radar; every emitted frame and every
record gains ``present`` and ``occupancy``.  It reports only, the pose is what it is without it.

``--rts`` (with ``--track``): the capture is a finished file, so after the flush the recorded tracker states go through the
Rauch-Tung-Striebel smoother (tools/smooth.py, csrc/pose_smooth.hip) and every record gains the smoothed pose.

``lag=N`` / ``--track-lag N`` (with ``--track``): fixed-lag smoothing while the stream runs (csrc/pose_lag.hip, one launch behind the
tracker's inside the same replay): every emitted frame carries the pose of N frames earlier smoothed over the N frames since, and every
record gains ``lagged``, ``lagged_velocity``, ``lagged_covariance`` and ``lagged_flag``, the last N from ``lag_tail()``.
"""
import argparse
import json
import math
import os

import numpy as np
import torch

from .. import functional as F_
from .. import runtime as rt
from ..preprocessing import process_iwr1843 as pre

ADC_SHAPE = (4, 192, 256, 2)           # one sensor-frame: rx, chirp, sample, I/Q (int16)
WARMUP_PUSHES = 2                      # eager pose-emitting pushes in front of the capture


class StreamError(ValueError):
    """Base of the session's argument errors."""


class LookaheadError(StreamError):
    """``lookahead`` outside 0 .. G // 2 - 1."""


class FrameShapeError(StreamError):
    """A pushed frame is not (lanes, 4, 192, 256, 2), or hori and vert differ."""


class FrameDtypeError(StreamError):
    """A pushed frame is not int16."""


class StreamEndedError(StreamError):
    """push() after flush(): the sequence has ended, reset() starts the next one."""


class DecodeError(StreamError):
    """``decode`` is none of "argmax", "subpixel" and "integral", or ``decode_radius`` is out of range or given without
    ``decode="integral"``."""


class SmoothingError(StreamError):
    """A ``PoseSmoothing`` parameter out of range, or ``smooth`` is not a ``PoseSmoothing``."""


class TrackingError(StreamError):
    """A ``PoseTracking`` parameter out of range, ``track`` is not a ``PoseTracking``, ``track`` together with ``smooth`` or with
    ``decode="integral"``, ``predict_now``, ``history`` or ``lag`` without ``track``, or ``lag`` outside 1..64."""


class InterferenceError(StreamError):
    """``interference`` is not an ``InterferenceFilter``, or one of its settings is out of range."""


class PresenceError(StreamError):
    """A ``PresenceGate`` parameter out of range, or ``presence`` is not a ``PresenceGate``."""


DECODES = ("argmax", "subpixel", "integral")
WEIGHTS = ("live", "averaged")      # which parameters of model_best.pth: as trained, or their moving average (TRAINING.emaDecay)


def _finite(error, field, v):
    """``v`` where it is a finite number and no bool; otherwise ``error`` in the name of ``field`` ("Class.field")."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise error("%s must be a finite number, got %r" % (field, v))
    return v


def _count(error, field, v, lo):
    """``v`` as an int where it is an integer (no bool) with lo <= v < 2^31; otherwise ``error`` in the name of ``field``."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v < 2 ** 31:
        raise error("%s must be an integer >= %d, got %r" % (field, lo, v))
    return int(v)


def _settings_repr(self):
    return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__))


class PoseSmoothing:
    """One-Euro filter settings (Casiez et al.) of a session: ``rate_hz`` the frame rate of the stream, ``min_cutoff`` (Hz) the
    cut-off at rest, ``beta`` its growth per pixel / second of speed, ``d_cutoff`` (Hz) the cut-off of the velocity estimate.  A
    joint whose score is <= ``min_score`` (or whose keypoint is not finite) is missing: it holds its last filtered position, reports
    zero velocity and leaves the filter state alone."""
    __slots__ = ("rate_hz", "min_cutoff", "beta", "d_cutoff", "min_score")

    def __init__(self, rate_hz, min_cutoff=1.0, beta=0.01, d_cutoff=1.0, min_score=0.0):
        vals = dict(rate_hz=rate_hz, min_cutoff=min_cutoff, beta=beta, d_cutoff=d_cutoff, min_score=min_score)
        vals = {k: _finite(SmoothingError, "PoseSmoothing." + k, v) for k, v in vals.items()}
        for k in ("rate_hz", "min_cutoff", "d_cutoff"):
            if not vals[k] > 0:
                raise SmoothingError("PoseSmoothing.%s must be positive, got %r" % (k, vals[k]))
        if beta < 0:
            raise SmoothingError("PoseSmoothing.beta must not be negative, got %r" % (beta,))
        for k, v in vals.items():
            setattr(self, k, float(v))

    __repr__ = _settings_repr


class _AssociationFields:
    """The four settings ``PoseTracking`` gained with the choice among heat-map peaks (a base class of their own, so that
    ``PoseTracking.__slots__`` lists what it always listed; ``PoseTracking.ARGUMENTS`` lists all)."""
    __slots__ = ("candidates", "min_separation", "peak_ratio", "gate_on_presence")


class _PairFields(_AssociationFields):
    """The three settings ``PoseTracking`` gained with the joint assignment of left / right partners (a base class of their own, for
    the same reason; ``PoseTracking.PAIR_ARGUMENTS`` lists them)."""
    __slots__ = ("pair_swap", "swap_cost", "pairs")


class _ManeuverFields(_PairFields):
    """The three settings ``PoseTracking`` gained with the second, "moving" motion model (a base class of their own, for the same
    reason; ``PoseTracking.MANEUVER_ARGUMENTS`` lists them)."""
    __slots__ = ("accel_psd_moving", "switch_prob", "moving_prior")


def check_pairs(pairs, joints=None):
    """A partner table: a sequence of 1..``F_.MAX_GROUP_ROWS`` integers (no bools), entry j the partner of joint j or j itself, its own
    inverse, and ``joints`` long where that is given -> the table as a tuple of ints.  Anything else is a TrackingError."""
    try:
        table = tuple(pairs)
    except TypeError:
        raise TrackingError("PoseTracking.pairs must be None or a sequence of joint indices, got %r" % (pairs,)) from None
    if not 1 <= len(table) <= F_.MAX_GROUP_ROWS or (joints is not None and len(table) != joints):
        raise TrackingError("PoseTracking.pairs must hold one entry per joint (%s), got %d"
                            % ("1..%d" % F_.MAX_GROUP_ROWS if joints is None else joints, len(table)))
    for j, q in enumerate(table):
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 0 <= q < len(table) or table[int(q)] != j:
            raise TrackingError("PoseTracking.pairs[%d] = %r: every entry is a joint index, and the partner's partner is the joint itself"
                                % (j, q))
    return tuple(int(q) for q in table)


class PoseTracking(_ManeuverFields):
    """Kalman tracker settings of a session (a constant-velocity filter per joint; the rule is stated beside hupr_pose_track_f32 in
    include/hupr.h): ``rate_hz`` the frame rate of the stream; ``accel_psd`` (pixel^2 / s^3) the power of the white acceleration that
    drives the process noise; the measurement noise is ``heatmap_gain`` times the spread of the heat-map around its peak plus
    ``meas_std`` (pixel) squared; ``gate`` the largest squared Mahalanobis distance of an accepted measurement (a chi-square
    quantile, 2 d.o.f.; the default is the 99.9 % one); ``max_coast`` the number of consecutive frames a track goes on without an
    accepted measurement before it ends; ``init_speed_std`` (pixel / s) the velocity uncertainty of a new track; a joint whose score
    is <= ``min_score`` has no measurement; ``horizon_s`` (s) how far ahead of the filtered pose the forecast looks.  The defaults
    are guesses: good values for real captures are unmeasured, and ``tools.calibrate.fit_tracking`` (``PoseStream.fit_tracking``,
    ``TEST.temporalFit``) fits ``accel_psd``, ``meas_std`` and ``heatmap_gain`` to a recording by maximum likelihood.
    ``candidates`` (1..4) > 1: the track chooses its measurement among that many peaks of the heat-map (csrc/pose_assoc.hip; the
    rule is stated beside hupr_pose_track_assoc_f32): the arg-max and the next local maxima that are at least ``peak_ratio`` (in
    (0, 1]) times as high and more than ``min_separation`` heat-map pixels from every peak taken; the one inside the gate with the
    smallest d2 + ln det S updates the track.  ``gate_on_presence`` (a session with ``presence`` only): a lane the presence gate calls
    empty has no measurement, its tracks coast and end.  The defaults of these three are guesses too, unmeasured on real captures;
    ``candidates=1`` is today's tracker, and stays the default because a second candidate can be the wrong one.
    ``pair_swap=True``: the left / right partners of the skeleton are assigned jointly (csrc/pose_pairs.hip; the rule is stated beside
    hupr_pose_track_pairs_f32): the two tracks of a pair share the peaks of both maps — each takes one, none is taken twice, the most
    tracks updated and then the smallest summed cost win — so that a network which exchanges a left and a right limb is followed
    instead of both tracks ending.  ``pairs``: the partner of every joint (itself for a joint without one), None = the ``L_*`` /
    ``R_*`` names of ``DATASET.idxToJoints`` (``tools.augment.mirror_pairs``).  ``swap_cost`` (>= 0) is added to the cost of a peak
    from the partner's map: 0 follows a swap at once, but two partners that pass close to each other then take each other's peak now
    and then; a larger value keeps those apart and follows a real swap late (PAPERS.md has the numbers).  Hence off by default; a good
    ``swap_cost`` for real captures is unmeasured.  It composes with ``candidates`` and ``gate_on_presence``.
    ``accel_psd_moving`` (None = off, else finite and >= ``accel_psd``): two filters per joint instead of one, the interacting-multiple-
    model estimator (csrc/pose_imm.hip; the rule is stated beside hupr_pose_track_imm_f32): a "still" model with ``accel_psd`` and a
    "moving" one with ``accel_psd_moving`` run on the same measurement, a Markov chain that changes model with probability
    ``switch_prob`` (in [0, 0.5]) per frame couples them, the likelihood of each filter's innovation updates their probabilities, and
    the pose is their mixture; a new track gives the moving model ``moving_prior`` (in [0, 1]).  For joints that rest, reach and rest
    again, where one ``accel_psd`` is wrong for one of the two regimes (PAPERS.md has the numbers, on a synthetic scenario).  The
    defaults of the three are guesses, unmeasured on real captures, and the default ``accel_psd`` of 200 is too high for a still
    model: lower it beside ``accel_psd_moving``.  The measurement is the arg-max: not with ``candidates`` > 1 or ``pair_swap``;
    ``gate_on_presence`` composes."""
    __slots__ = ("rate_hz", "accel_psd", "meas_std", "heatmap_gain", "gate", "max_coast", "init_speed_std", "min_score", "horizon_s")
    ARGUMENTS = __slots__ + _AssociationFields.__slots__
    PAIR_ARGUMENTS = _PairFields.__slots__
    MANEUVER_ARGUMENTS = _ManeuverFields.__slots__

    def __init__(self, rate_hz, accel_psd=200.0, meas_std=1.0, heatmap_gain=1.0, gate=13.816, max_coast=5, init_speed_std=50.0,
                 min_score=0.0, horizon_s=0.0, candidates=1, min_separation=3, peak_ratio=0.25, gate_on_presence=False, pair_swap=False,
                 swap_cost=0.0, pairs=None, accel_psd_moving=None, switch_prob=0.05, moving_prior=0.5):
        vals = dict(rate_hz=rate_hz, accel_psd=accel_psd, meas_std=meas_std, heatmap_gain=heatmap_gain, gate=gate,
                    init_speed_std=init_speed_std, min_score=min_score, horizon_s=horizon_s, peak_ratio=peak_ratio, swap_cost=swap_cost)
        vals = {k: _finite(TrackingError, "PoseTracking." + k, v) for k, v in vals.items()}
        for k in ("rate_hz", "meas_std", "gate", "init_speed_std"):
            if not vals[k] > 0:
                raise TrackingError("PoseTracking.%s must be positive, got %r" % (k, vals[k]))
        for k in ("accel_psd", "heatmap_gain", "horizon_s", "swap_cost"):
            if vals[k] < 0:
                raise TrackingError("PoseTracking.%s must not be negative, got %r" % (k, vals[k]))
        if not isinstance(pair_swap, bool):
            raise TrackingError("PoseTracking.pair_swap must be True or False, got %r" % (pair_swap,))
        self.pair_swap = pair_swap
        self.pairs = None if pairs is None else check_pairs(pairs)
        if not 0 < peak_ratio <= 1:
            raise TrackingError("PoseTracking.peak_ratio must be in (0, 1], got %r" % (peak_ratio,))
        self.max_coast = _count(TrackingError, "PoseTracking.max_coast", max_coast, 0)
        self.candidates = _count(TrackingError, "PoseTracking.candidates", candidates, 1)
        if self.candidates > F_.MAX_CANDIDATES:
            raise TrackingError("PoseTracking.candidates must be an integer in 1..%d, got %r" % (F_.MAX_CANDIDATES, candidates))
        self.min_separation = _count(TrackingError, "PoseTracking.min_separation", min_separation, 0)
        if not isinstance(gate_on_presence, bool):
            raise TrackingError("PoseTracking.gate_on_presence must be True or False, got %r" % (gate_on_presence,))
        self.gate_on_presence = gate_on_presence
        for k, v in vals.items():
            setattr(self, k, float(v))
        self.switch_prob = float(_finite(TrackingError, "PoseTracking.switch_prob", switch_prob))
        self.moving_prior = float(_finite(TrackingError, "PoseTracking.moving_prior", moving_prior))
        if not 0 <= self.switch_prob <= 0.5:
            raise TrackingError("PoseTracking.switch_prob must be in [0, 0.5], got %r" % (switch_prob,))
        if not 0 <= self.moving_prior <= 1:
            raise TrackingError("PoseTracking.moving_prior must be in [0, 1], got %r" % (moving_prior,))
        self.accel_psd_moving = None
        if accel_psd_moving is not None:
            self.accel_psd_moving = float(_finite(TrackingError, "PoseTracking.accel_psd_moving", accel_psd_moving))
            if self.accel_psd_moving < self.accel_psd:
                raise TrackingError("PoseTracking.accel_psd_moving must not be below accel_psd %r, got %r" % (self.accel_psd, accel_psd_moving))
            if self.candidates > 1 or self.pair_swap:
                raise TrackingError("PoseTracking.accel_psd_moving excludes candidates > 1 and pair_swap: the two models run on the "
                                    "arg-max measurement")

    def __repr__(self):
        shown = self.ARGUMENTS + (self.PAIR_ARGUMENTS if self.pair_swap else ())        # without the option: what it always printed
        shown += self.MANEUVER_ARGUMENTS if self.maneuvers else ()
        return "PoseTracking(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in shown)

    @property
    def associates(self):
        """Whether a session with these settings launches an associating tracker (csrc/pose_assoc.hip, or csrc/pose_pairs.hip with
        ``pair_swap``) instead of the plain one."""
        return (self.candidates > 1 or self.gate_on_presence or self.pair_swap) and not self.maneuvers

    @property
    def maneuvers(self):
        """Whether a session with these settings launches the two-model tracker (csrc/pose_imm.hip) instead of the plain one."""
        return self.accel_psd_moving is not None

    def _copy(self, **changed):
        return PoseTracking(**dict({k: getattr(self, k) for k in self.ARGUMENTS + self.PAIR_ARGUMENTS + self.MANEUVER_ARGUMENTS},
                                   **changed))

    def with_horizon(self, horizon_s):
        """A copy that forecasts ``horizon_s`` seconds ahead."""
        return self._copy(horizon_s=horizon_s)

    def for_joints(self, names):
        """With ``pair_swap``: a copy whose ``pairs`` fit the joints ``names`` — ``mirror_pairs(names)`` where ``pairs`` is None, else
        ``pairs`` itself, which must hold one entry per name.  Without ``pair_swap``: these settings themselves."""
        if not self.pair_swap:
            return self
        names = list(names)
        pairs = self.pairs
        if pairs is None:
            from .augment import mirror_pairs
            try:
                pairs = mirror_pairs(names)
            except ValueError as e:
                raise TrackingError("PoseTracking.pairs: %s" % e) from None
        return self._copy(pairs=check_pairs(pairs, len(names)))


class PresenceGate:
    """Scene-occupancy settings of a session (frozen; the rule is stated beside hupr_cfar_ra_f32 in include/hupr.h).  The CA-CFAR
    detector on the centre frame's horizontal mean planes: ``pfa`` the design false-alarm probability per cell, ``guard`` and ``train``
    the half-widths of the guard area and of the training area beyond it (``guard + train <= 8``).  The gate over its detections: a
    frame is a hit when it holds at least ``min_cells`` detections; an absent lane becomes present after ``confirm`` consecutive
    hits, a present lane absent after more than ``hold`` consecutive misses — a person who stands still vanishes under clutter
    removal, and ``hold`` bridges the pause.  The six defaults are guesses: nobody has run this on a real capture."""
    __slots__ = ("pfa", "guard", "train", "min_cells", "confirm", "hold")

    def __init__(self, pfa=1e-5, guard=2, train=4, min_cells=3, confirm=2, hold=20):
        from ..preprocessing.cfar import check_cfar
        try:
            pfa, guard, train = check_cfar(pfa, guard, train)
        except ValueError as e:
            raise PresenceError("PresenceGate: %s" % e) from None
        vals = dict(pfa=pfa, guard=guard, train=train)
        for k, v, lo in (("min_cells", min_cells, 1), ("confirm", confirm, 1), ("hold", hold, 0)):
            vals[k] = _count(PresenceError, "PresenceGate." + k, v, lo)
        for k, v in vals.items():
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError("PresenceGate is frozen")

    def __delattr__(self, name):
        raise AttributeError("PresenceGate is frozen")

    def __eq__(self, other):
        return isinstance(other, PresenceGate) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, k) for k in self.__slots__))

    __repr__ = _settings_repr


def check_interference(interference):
    """The session's ``interference`` argument: None or an InterferenceFilter."""
    from ..preprocessing.interference import InterferenceFilter
    if interference is not None and not isinstance(interference, InterferenceFilter):
        raise InterferenceError("interference must be an InterferenceFilter or None, got %r" % (interference,))
    return interference


def check_presence(presence):
    """The session's ``presence`` argument: None or a PresenceGate."""
    if presence is not None and not isinstance(presence, PresenceGate):
        raise PresenceError("presence must be a PresenceGate or None, got %r" % (presence,))
    return presence


def presence_setting(cfg):
    """``TEST.presence`` (no key of the reference's YAML) -> None with the key absent or ``false``, ``PresenceGate()`` with ``true``, a
    PresenceGate of the given values with a mapping of its six names.  Anything else raises here, where the config is read."""
    v = getattr(getattr(cfg, "TEST", None), "presence", None)
    if v is None or v is False:
        return None
    if v is True:
        return PresenceGate()
    if not isinstance(v, dict):                         # config_tree.obj: a YAML mapping as attributes
        if not hasattr(v, "__dict__") or isinstance(v, type):
            raise ValueError("TEST.presence must be true, false or a mapping of PresenceGate arguments, got %r" % (v,))
        v = vars(v)
    for k in v:
        if k not in PresenceGate.__slots__:
            raise ValueError("TEST.presence.%s is no PresenceGate argument (%s)" % (k, ", ".join(PresenceGate.__slots__)))
    try:
        return PresenceGate(**dict(v))
    except PresenceError as e:
        raise ValueError("TEST.presence: %s" % e) from None


def check_decode(decode, smooth, decode_radius=None, heatmap_size=None):
    """The session's decode arguments: ``decode`` one of DECODES, ``smooth`` None or a PoseSmoothing, ``decode_radius`` only with
    ``decode="integral"`` -> the integral decode's window radius (None for the other decodes): ``decode_radius`` itself, 0 (the whole
    map) or an integer in [1, heatmap_size - 1], or by default the targets' patch radius at ``heatmap_size``."""
    if not isinstance(decode, str) or decode not in DECODES:
        raise DecodeError("decode must be 'argmax', 'subpixel' or 'integral', got %r" % (decode,))
    if smooth is not None and not isinstance(smooth, PoseSmoothing):
        raise SmoothingError("smooth must be a PoseSmoothing or None, got %r" % (smooth,))
    if decode != "integral":
        if decode_radius is not None:
            raise DecodeError("decode_radius needs decode='integral', got decode %r" % (decode,))
        return None
    from ..misc.metrics import check_decode_radius, default_decode_radius
    try:
        if decode_radius is None:
            return default_decode_radius(heatmap_size)
        return check_decode_radius(decode_radius, heatmap_size, "decode_radius")
    except ValueError as e:
        raise DecodeError(str(e)) from None


def check_track(track, smooth, predict_now, decode="argmax", presence=None):
    """The session's tracker arguments: ``track`` None or a PoseTracking, never beside ``smooth`` or ``decode="integral"``;
    ``predict_now`` only with it; ``gate_on_presence`` only in a session with ``presence``."""
    if track is not None and not isinstance(track, PoseTracking):
        raise TrackingError("track must be a PoseTracking or None, got %r" % (track,))
    if track is not None and track.gate_on_presence and presence is None:
        raise TrackingError("PoseTracking.gate_on_presence needs presence: the verdict is the presence gate's")
    if track is not None and decode == "integral":
        raise TrackingError("track and decode='integral' exclude each other: the tracker's measurement is the sub-pixel decode's")
    if track is not None and smooth is not None:
        raise TrackingError("track and smooth exclude each other: a session has one temporal filter")
    if predict_now and track is None:
        raise TrackingError("predict_now needs track: the forecast is the tracker's")


def stream_window_sources(center, newest, G):
    """Frame numbers (counted from the start of the stream) of the G-frame window around ``center`` when ``newest`` is the last frame
    that exists: frames before the start repeat frame 0, frames that have not arrived repeat the newest."""
    return [min(max(center - G // 2 + j, 0), newest) for j in range(G)]


def check_lookahead(lookahead, G):
    """-> the session's lookahead (None: G // 2 - 1, every window complete on its future side)."""
    if G < 2 or G % 2:
        raise StreamError("numGroupFrames must be even and >= 2, got %r" % (G,))
    if lookahead is None:
        return G // 2 - 1
    if isinstance(lookahead, bool) or not isinstance(lookahead, (int, np.integer)) or not 0 <= lookahead <= G // 2 - 1:
        raise LookaheadError("lookahead must be an integer in 0..%d for %d-frame windows, got %r" % (G // 2 - 1, G, lookahead))
    return int(lookahead)


def check_frames(adc_hori, adc_vert, lanes):
    """The two tensors of one push: int16 (lanes, 4, 192, 256, 2) each, on the same kind of device."""
    for name, t in (("adc_hori", adc_hori), ("adc_vert", adc_vert)):
        if not isinstance(t, torch.Tensor):
            raise FrameDtypeError("%s must be a torch int16 tensor, got %s" % (name, type(t).__name__))
        if t.dtype != torch.int16:
            raise FrameDtypeError("%s must be int16, got %s" % (name, t.dtype))
    if tuple(adc_hori.shape) != tuple(adc_vert.shape):
        raise FrameShapeError("hori / vert frames differ in shape: %r vs %r" % (tuple(adc_hori.shape), tuple(adc_vert.shape)))
    if tuple(adc_hori.shape) != (lanes,) + ADC_SHAPE:
        raise FrameShapeError("a pushed frame must be %r, got %r" % ((lanes,) + ADC_SHAPE, tuple(adc_hori.shape)))
    if adc_hori.is_cuda != adc_vert.is_cuda:
        raise FrameShapeError("hori / vert frames must both be host or both be device tensors")


class StreamSchedule:
    """The emission schedule as host arithmetic (the mirror of the device counters): which frame a push answers and from which
    source frames, and what a flush still owes."""

    def __init__(self, G, lookahead=None):
        self.G = G
        self.lookahead = check_lookahead(lookahead, G)
        self.reset()

    def reset(self):
        self.frames_pushed = 0
        self.frames_emitted = 0
        self.ended = False

    def push(self):
        """Count one pushed frame -> (center, window sources) of the pose it answers, or None during the first ``lookahead`` pushes."""
        if self.ended:
            raise StreamEndedError("flush() ended this sequence; reset() starts a new one")
        n = self.frames_pushed
        self.frames_pushed += 1
        c = n - self.lookahead
        if c < 0:
            return None
        self.frames_emitted += 1
        return c, stream_window_sources(c, n, self.G)

    def flush(self):
        """-> [(center, window sources)] of the min(lookahead, frames pushed) poses still owed; ends the sequence."""
        out = []
        newest = self.frames_pushed - 1
        while self.frames_emitted < self.frames_pushed:
            c = self.frames_emitted
            self.frames_emitted += 1
            out.append((c, stream_window_sources(c, newest, self.G)))
        self.ended = True
        return out


class _InterferenceFields:
    """The field a session with ``interference`` adds to every frame it emits (a base class of its own, for the same reason as the
    next one)."""
    __slots__ = ("interference",)


class _OccupancyFields(_InterferenceFields):
    """The two fields a session with ``presence`` adds to every frame it emits (a base class of their own, so that ``PoseFrame.__slots__``
    and ``TrackedPoseFrame.__slots__`` list what they always listed)."""
    __slots__ = ("present", "occupancy")


class PoseFrame(_OccupancyFields):
    """One emitted pose.  ``frame``: its number in the stream; ``keypoints`` (lanes, K, 2) fp32 image pixels (x, y) — the One-Euro
    filtered ones when the session smooths; ``scores`` (lanes, K) the GCN head's maxima; ``indices`` (lanes, K) int32 arg-max
    positions; ``heatmap`` (lanes, K, 1, H, W) and ``gcn_heatmap`` (lanes, 1, K, H, W); ``raw_keypoints`` the decoded keypoints in
    front of the filter (``keypoints`` itself without one); ``velocity`` (lanes, K, 2) image pixels per second, None without a
    filter; ``present`` (lanes,) int32, the presence gate's verdict on this frame, and ``occupancy`` (lanes, 8) fp32, the detector's
    summary of it (``functional.CFAR_SUMMARY``), both None in a session without ``presence``; ``interference`` (2 sensors, lanes, 2)
    int32, the samples the interference filter replaced and the chirps it touched in the frame PUSHED by the call that returned this
    pose — the newest frame of the window, ``lookahead`` frames after the emitted centre —, None in a session without
    ``interference`` and in the frames of a ``flush()``, which pushes nothing.  Device tensors owned by the session, valid until its
    next push / flush / reset."""
    __slots__ = ("frame", "keypoints", "scores", "indices", "heatmap", "gcn_heatmap", "raw_keypoints", "velocity")
    lagged = None                       # the fixed-lag pose that falls due with this frame: only a session with ``lag`` fills it

    def __init__(self, frame, keypoints, scores, indices, heatmap, gcn_heatmap, raw_keypoints=None, velocity=None, present=None,
                 occupancy=None, interference=None):
        self.frame, self.keypoints, self.scores, self.indices = frame, keypoints, scores, indices
        self.heatmap, self.gcn_heatmap = heatmap, gcn_heatmap
        self.raw_keypoints = keypoints if raw_keypoints is None else raw_keypoints
        self.velocity = velocity
        self.present, self.occupancy = present, occupancy
        self.interference = interference

    def _map(self, fn):
        """A frame of the same class with ``fn`` of every tensor: the fields are the ``__slots__`` along the MRO, and the constructors
        take them by those names."""
        fields = {k: getattr(self, k) for c in type(self).__mro__ for k in getattr(c, "__slots__", ())}
        each = lambda k, v: v if v is None or k == "frame" else v._map(fn) if k == "lagged" else fn(v)
        return type(self)(**{k: each(k, v) for k, v in fields.items()})

    def clone(self):
        return self._map(torch.clone)

    def cpu(self):
        """Host copies (synchronises)."""
        return self._map(lambda t: t.cpu())


class _CandidateFields(PoseFrame):
    """The four fields an associating tracking session adds to every frame it emits (a base class of their own, for the same reason)."""
    __slots__ = ("candidates", "candidate_scores", "candidate_count", "chosen")


class TrackedPoseFrame(_CandidateFields):
    """What a tracking session (``track=PoseTracking(...)``) emits.  ``keypoints`` are the Kalman-filtered ones, ``raw_keypoints`` the
    decoded ones, ``velocity`` the track's; ``covariance`` (lanes, K, 3) = (Pxx, Pxy, Pyy) of the filtered position in image pixels
    squared; ``forecast`` (lanes, K, 2) the position ``horizon_s`` ahead; ``status`` (lanes, K) int32, one of ``STATUS``'s codes.
    With ``PoseTracking(candidates=C > 1)`` or ``gate_on_presence`` also ``candidates`` (lanes, K, C, 2), the heat-map peaks every
    joint's track chose among, in image pixels (peak 0 is ``raw_keypoints``), ``candidate_scores`` (lanes, K, C) their heat-map
    values, ``candidate_count`` (lanes, K) int32 how many there are (the slots behind hold zeros) and ``chosen`` (lanes, K) int32,
    the peak that went into the track in this frame, -1 for none; all four None otherwise.  ``source`` is None here: a session with
    ``PoseTracking(pair_swap=True)`` emits ``PairedPoseFrame``s, which carry it."""
    __slots__ = ("covariance", "forecast", "status")
    STATUS = ("UPDATED", "COASTED_MISSING", "COASTED_GATED", "STARTED", "LOST")
    source = None

    def __init__(self, frame, keypoints, scores, indices, heatmap, gcn_heatmap, raw_keypoints, velocity, covariance, forecast, status,
                 present=None, occupancy=None, candidates=None, candidate_scores=None, candidate_count=None, chosen=None, interference=None):
        super().__init__(frame, keypoints, scores, indices, heatmap, gcn_heatmap, raw_keypoints, velocity, present, occupancy, interference)
        self.covariance, self.forecast, self.status = covariance, forecast, status
        self.candidates, self.candidate_scores, self.candidate_count, self.chosen = candidates, candidate_scores, candidate_count, chosen


class PairedPoseFrame(TrackedPoseFrame):
    """What a tracking session with ``PoseTracking(pair_swap=True)`` emits: a ``TrackedPoseFrame`` with its four candidate fields and
    ``source`` (lanes, K) int32, the heat-map the peak that went into the track stands in: 0 the joint's own, 1 its partner's
    (``chosen`` is then a peak of the partner's ``candidates``), -1 for none.  (A class of its own, so that the fields of a
    ``TrackedPoseFrame`` are what they always were.)"""
    __slots__ = ("source",)

    def __init__(self, *fields, source=None, **more):
        super().__init__(*fields, **more)
        self.source = source


class ManeuveringPoseFrame(TrackedPoseFrame):
    """What a tracking session with ``PoseTracking(accel_psd_moving=...)`` emits: a ``TrackedPoseFrame`` — keypoints, velocity,
    covariance and forecast are the mixture of the still and the moving model — with ``moving`` (lanes, K), the probability of the
    moving model, 0 for a joint without a live track.  (A class of its own, so that the fields of a ``TrackedPoseFrame`` are what they
    always were.)"""
    __slots__ = ("moving",)

    def __init__(self, *fields, moving=None, **more):
        super().__init__(*fields, **more)
        self.moving = moving


class LaggedPose:
    """The fixed-lag smoothed pose that falls due with an emitted frame of a session with ``lag=L`` (csrc/pose_lag.hip; the rule is
    stated beside hupr_pose_smooth_lag_f32 in include/hupr.h): the pose of ``frame`` = the emitted centre - L, smoothed backwards
    over the L poses emitted since.  ``keypoints`` (lanes, K, 2), ``velocity`` (lanes, K, 2) per second, ``covariance`` (lanes, K, 3)
    = (Pxx, Pxy, Pyy), ``flag`` (lanes, K) int32, one of ``functional.SMOOTH_*``; and what the filter gave for that frame:
    ``filtered`` its keypoints, ``raw_keypoints`` the decoded ones, ``status`` its status codes, ``scores`` the maxima.  Device
    tensors owned by the session, valid until its next push / flush / reset."""
    __slots__ = ("frame", "keypoints", "velocity", "covariance", "flag", "filtered", "raw_keypoints", "status", "scores")

    def __init__(self, frame, keypoints, velocity, covariance, flag, filtered, raw_keypoints, status, scores):
        self.frame, self.keypoints, self.velocity, self.covariance, self.flag = frame, keypoints, velocity, covariance, flag
        self.filtered, self.raw_keypoints, self.status, self.scores = filtered, raw_keypoints, status, scores

    def _map(self, fn):
        return LaggedPose(self.frame, *[fn(getattr(self, k)) for k in self.__slots__[1:]])

    def clone(self):
        return self._map(torch.clone)

    def cpu(self):
        """Host copies (synchronises)."""
        return self._map(lambda t: t.cpu())


class LaggedTrackedPoseFrame(TrackedPoseFrame):
    """What a tracking session with ``lag=L`` emits: a ``TrackedPoseFrame`` with ``lagged``, the ``LaggedPose`` of L frames ago, None
    in the first L frames of a sequence.  (A class of its own, so that the fields of a ``TrackedPoseFrame`` are what they always
    were.)"""
    __slots__ = ("lagged",)

    def __init__(self, *fields, lagged=None, **more):
        super().__init__(*fields, **more)
        self.lagged = lagged


class LaggedPairedPoseFrame(PairedPoseFrame):
    """The same for a session with ``PoseTracking(pair_swap=True)``: a ``PairedPoseFrame`` with ``lagged``."""
    __slots__ = ("lagged",)

    def __init__(self, *fields, lagged=None, **more):
        super().__init__(*fields, **more)
        self.lagged = lagged


def check_lag(lag, track):
    """The session's ``lag`` argument: None, or with ``track`` an integer in 1..``F_.MAX_LAG`` -> None or the int."""
    if lag is None:
        return None
    if track is None:
        raise TrackingError("lag needs track: the fixed-lag smoother runs over the tracker's states")
    if track.maneuvers:
        raise TrackingError("lag and PoseTracking.accel_psd_moving exclude each other: the smoother runs over a single model's states")
    try:
        return F_.check_lag(lag, "PoseStream: lag")
    except ValueError as e:
        raise TrackingError(str(e)) from None


class PoseStream:
    """Streaming session around a HuPRNet.  ``push(adc_hori, adc_vert)`` takes the new int16 frame of both sensors,
    (lanes, 4, 192, 256, 2) each — device tensors are used directly, host tensors go through the session's pinned staging and an
    asynchronous copy — and returns the ``PoseFrame`` that is due (None during the first ``lookahead`` pushes).  ``flush()`` returns the
    poses still owed at the end of a sequence (independent copies), ``reset()`` starts the next one.  ``lanes`` radars advance in lock
    step (the model's batch axis).  The precision mode is the model's ``math_mode`` or, without one, the calling thread's at
    construction; it holds for the session.  Weights changed between pushes are honoured: the packed copies are refreshed in front of
    the replay.  A push waits for the previous one to finish before it reuses the pinned staging.  Side effect: like ``engine.infer``,
    ``push`` and ``flush`` put a model that is in training mode into eval mode (``model.eval()``) and leave it there.  ``lanes = 2`` is
    the model at batch 2: bit-identical to the offline route on a batch of 2, not to two ``lanes = 1`` sessions (the existing kernels
    take other launch routes for a single sample).  ``decode="subpixel"`` refines every keypoint to sub-pixel
    position; ``smooth=PoseSmoothing(rate_hz, ...)`` filters the keypoints over time (the filter state is the session's, ``reset()``
    clears it) and adds ``PoseFrame.velocity``.  ``track=PoseTracking(rate_hz, ...)`` is the other temporal filter, in place of
    ``smooth``: a constant-velocity Kalman filter per joint whose measurement noise is read off the heat-map; the session then emits
    ``TrackedPoseFrame``s (filtered keypoints, velocity, position covariance, forecast, status), and with ``predict_now=True`` the
    forecast horizon is ``lookahead / rate_hz`` — where the joint is at the newest frame, not at the emitted one — whatever the
    tracker's own ``horizon_s``.  ``decode="integral"`` decodes the mass centroid of the window of ``decode_radius`` heat-map pixels
    around the peak (None: the targets' patch radius, 6 at 64 and 9 at 128; 0: the whole map), with ``smooth`` in the same launch and
    never with ``track``.  With the defaults the session decodes exactly as before, in the same two launches.
    ``tdm_compensation=True``: the FFT chain of every push compensates the TDM Doppler phase (``fft_chain_loader_means`` with
    ``tdm_compensation`` and no swap table, inside the same graph replay) — for weights trained with ``DATASET.tdmCompensation``.
    ``history=True`` (needs ``track``): after every push or flush that emits a pose the tracker's state and outputs are copied into a
    history on the device (tools/smooth.py: TrackHistory) — eager device-to-device copies on the session's stream, behind the graph
    replay and not inside it — and ``smoothed()`` returns the Rauch-Tung-Striebel smoothed poses emitted since the last ``reset()``
    in one launch of csrc/pose_smooth.hip.  The default adds nothing.
    ``presence=PresenceGate(...)``: scene occupancy.  Behind the window MNet of every push or flush that emits a pose, a CA-CFAR
    detector runs on the centre frame's horizontal mean planes, read from the ring, and a presence gate runs over its detections
    (csrc/cfar.hip: two launches, inside the graph replay); the emitted frame gains ``present`` and ``occupancy``, and ``reset()``
    clears the gate.  By itself the gate reports only: keypoints, scores and the tracker's input are what they are without it, bit
    for bit.  It composes with every other setting.
    ``track=PoseTracking(..., candidates=C)`` with C > 1: every joint's track chooses its measurement among up to C peaks of its
    heat-map (csrc/pose_assoc.hip: one launch in place of the tracker's, inside the same graph replay), and the emitted frame gains
    ``candidates``, ``candidate_scores``, ``candidate_count`` and ``chosen``.  ``PoseTracking(gate_on_presence=True)`` (needs
    ``presence``) hands that launch the gate's verdict on the emitted frame: a lane the gate calls empty has no measurement, its tracks
    coast and then report LOST.  With ``candidates=1`` and no coupling the session launches the plain tracker, as before.
    ``track=PoseTracking(..., pair_swap=True)``: the left / right partners of the skeleton (``pairs``, by default the ``L_*`` / ``R_*``
    names of ``DATASET.idxToJoints``) are assigned jointly (csrc/pose_pairs.hip: one launch in the tracker's place likewise, inside the
    same graph replay), so a left / right exchange by the network is followed; the session emits ``PairedPoseFrame``s: the four
    candidate fields and ``source``.  Off by default: see ``PoseTracking``.
    ``interference=InterferenceFilter(...)``: interference blanking of the pushed frames (preprocessing/interference.py,
    csrc/interference.hip: two launches between the upload and the FFT chain, inside the same graph replay, in place on the session's
    device copy of the frames — a caller's device tensors are left as they are).  Every frame a push emits gains ``interference``,
    the filter's counts on the frame that push brought in.  It composes with every other setting; the default adds nothing.
    ``lag=L`` (needs ``track``; an integer in 1..64): fixed-lag smoothing.  Behind the tracker's launch of every push or flush that
    emits a pose, one launch of csrc/pose_lag.hip, inside the same graph replay, files the tracker's state in a ring of L + 1 frames
    on the device and runs the Rauch-Tung-Striebel backward pass over that ring.  The session then emits ``LaggedTrackedPoseFrame``s
    (``LaggedPairedPoseFrame``s with ``pair_swap``): every frame gains ``lagged``, the ``LaggedPose`` of the frame L poses earlier —
    None in the first L emitted frames — and after ``flush()`` ``lag_tail()`` returns the L poses still owed.  The smoother reports
    only: the filter's own outputs are those of a session without ``lag``, bit for bit; ``reset()`` starts its ring anew.  It works
    with all three tracker launches and with ``history`` and ``presence``.  The default, None, adds nothing.
    ``measurements=True`` (needs ``track``): the session records what the tracker measured, so that its noise parameters can be fitted
    to the capture afterwards.  Behind the tracker's launch of every push or flush that emits a pose, one launch of
    csrc/pose_fit.hip (``functional.pose_measure``), inside the same graph replay, writes the frame's measurements — raw keypoint,
    score and covariance window, 32 bytes per joint — and an eager device-to-device copy behind the replay files them in a
    ``MeasurementRecord`` (tools/calibrate.py).  ``fit_tracking()`` then returns the maximum-likelihood ``accel_psd``, ``meas_std`` and
    ``heatmap_gain`` over everything recorded (``tools.calibrate.fit_tracking``); ``reset()`` keeps the record and marks the next
    pose as a sequence's first.  It reports only: the tracker's outputs are those of a session without it, bit for bit.  The default,
    False, adds nothing.
    ``track=PoseTracking(..., accel_psd_moving=Q)``: two motion models per joint, a still and a moving one (csrc/pose_imm.hip: one
    launch in the tracker's place likewise, inside the same graph replay, on a 32-float state per joint that ``reset()`` clears); the
    session emits ``ManeuveringPoseFrame``s, whose keypoints, velocity, covariance and forecast are the mixture of the two models and
    which carry ``moving``.  ``gate_on_presence`` and ``measurements`` compose (``fit_tracking()`` fits the single-model filter as
    ever and leaves both acceleration PSDs as they are); ``lag`` and ``history`` do not: their smoothers run over a single model's
    states.  Off by default: see ``PoseTracking``."""

    def __init__(self, model, cfg, lanes=1, lookahead=None, graph=True, device=None, decode="argmax", smooth=None, track=None,
                 predict_now=False, decode_radius=None, tdm_compensation=False, history=False, presence=None, interference=None,
                 lag=None, measurements=False):
        D = cfg.DATASET
        self.G = D.numGroupFrames
        self.schedule = StreamSchedule(self.G, lookahead)
        self.lookahead = self.schedule.lookahead
        self.decode_radius = check_decode(decode, smooth, decode_radius, D.heatmapSize)
        check_track(track, smooth, predict_now, decode, presence)
        self.decode, self.smooth, self.predict_now = decode, smooth, bool(predict_now)
        if not isinstance(tdm_compensation, bool):
            raise StreamError("tdm_compensation must be True or False, got %r" % (tdm_compensation,))
        self.tdm_compensation = tdm_compensation
        if not isinstance(history, bool):
            raise StreamError("history must be True or False, got %r" % (history,))
        if history and track is None:
            raise TrackingError("history needs track: it records the tracker's states for smoothed()")
        if history and track.maneuvers:
            raise TrackingError("history and PoseTracking.accel_psd_moving exclude each other: smoothed() runs over a single model's states")
        self.lag = check_lag(lag, track)
        if not isinstance(measurements, bool):
            raise StreamError("measurements must be True or False, got %r" % (measurements,))
        if measurements and track is None:
            raise TrackingError("measurements needs track: it records what the tracker measured for fit_tracking()")
        if track is not None:                                  # pair_swap: the partner table of this config's joints
            track = track.for_joints(getattr(D, "idxToJoints", range(D.numKeypoints)))
        self.track = track.with_horizon(self.lookahead / track.rate_hz) if predict_now else track
        self.presence = check_presence(presence)
        self.interference = check_interference(interference)
        if not isinstance(lanes, int) or lanes < 1:
            raise StreamError("lanes must be a positive integer, got %r" % (lanes,))
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        if self.device.type != "cuda":
            raise rt.HuprError("PoseStream needs a GPU model (no CPU fallback), got %s" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if (D.rangeSize, D.azimuthSize) != (64, 64) or (D.numFrames, model.numFilters) != (8, 32):
            raise StreamError("the FFT chain and the MNet kernels are specialised for 64 x 64 maps, 8 chirp steps and 32 filters")
        self.model, self.cfg, self.lanes, self.graph = model, cfg, lanes, bool(graph)
        self.mode = model.math_mode if model.math_mode is not None else F_.MATH
        with F_.math_mode(self.mode), F_.region("mnet"):
            self._bf16 = F_.act_bf16()
        self.K, self.H, self.W = D.numKeypoints, D.heatmapSize, D.heatmapSize
        self.ratio = float(D.imgSize) / float(D.heatmapSize)
        self.pixels = D.rangeSize * D.azimuthSize
        L, dev, G = rt.lib(), self.device, self.G
        with torch.cuda.device(dev):
            self._pinned = torch.empty((2, lanes) + ADC_SHAPE, dtype=torch.int16).pin_memory()
            self._adc = torch.empty((2, lanes) + ADC_SHAPE, dtype=torch.int16, device=dev)
            self._staging = torch.empty((2, lanes, 16, self.pixels), dtype=torch.float32, device=dev)
            self._ring = torch.zeros((2, lanes, G, 16, self.pixels), dtype=torch.float32, device=dev)
            self._state = torch.zeros(max(int(L.hupr_stream_state_bytes()), 16), dtype=torch.uint8, device=dev)
            self._ws = pre._workspace(2 * lanes, dev)[0]
            act = torch.bfloat16 if self._bf16 else torch.float32
            self._maps = tuple(torch.empty((lanes, G, D.rangeSize, D.azimuthSize, 32), dtype=act, device=dev) for _ in range(2))
            self._idx = torch.empty((lanes, self.K), dtype=torch.int32, device=dev)
            self._mx = torch.empty((lanes, self.K), dtype=torch.float32, device=dev)
            self._kp = torch.empty((lanes, self.K, 2), dtype=torch.float32, device=dev)
            # the one-launch decode (csrc/pose_decode.hip; csrc/pose_integral.hip for "integral") serves everything but the default; with
            # a filter _kp holds the filtered keypoints, _raw the decoded ones, _vel the velocity, _fstate the filter's state
            self._fused = decode != "argmax" or smooth is not None
            self._raw = self._vel = self._fstate = None
            if smooth is not None:
                self._raw, self._vel = torch.empty_like(self._kp), torch.empty_like(self._kp)
                self._fstate = F_.pose_filter_state(lanes * self.K, dev)
            # the tracking decode (csrc/pose_track.hip) likewise: _kp the filtered keypoints, _raw the decoded ones, _vel the track's
            # velocity, _cov / _fc / _status its covariance, forecast and status, _tstate its state
            self._cov = self._fc = self._status = self._tstate = None
            if track is not None:
                self._raw, self._vel, self._fc = torch.empty_like(self._kp), torch.empty_like(self._kp), torch.empty_like(self._kp)
                self._cov = torch.empty((lanes, self.K, 3), dtype=torch.float32, device=dev)
                self._status = torch.empty((lanes, self.K), dtype=torch.int32, device=dev)
                self._tstate = (F_.pose_imm_state if track.maneuvers else F_.pose_track_state)(lanes * self.K, dev)
            # the associating tracker (csrc/pose_assoc.hip) in its place: the candidates it chose among and its choice
            self._cxy = self._cscore = self._ccount = self._chosen = None
            if track is not None and track.associates:
                C = track.candidates
                self._cxy = torch.zeros((lanes, self.K, C, 2), dtype=torch.float32, device=dev)
                self._cscore = torch.zeros((lanes, self.K, C), dtype=torch.float32, device=dev)
                self._ccount = torch.zeros((lanes, self.K), dtype=torch.int32, device=dev)
                self._chosen = torch.full((lanes, self.K), -1, dtype=torch.int32, device=dev)
            # with pair_swap (csrc/pose_pairs.hip in its place): the map every choice came from
            self._source = torch.full((lanes, self.K), -1, dtype=torch.int32, device=dev) if track is not None and track.pair_swap else None
            # with accel_psd_moving (csrc/pose_imm.hip in its place): the probability of the moving model
            self._moving = torch.zeros((lanes, self.K), dtype=torch.float32, device=dev) if track is not None and track.maneuvers else None
            # the fixed-lag smoother behind it (csrc/pose_lag.hip): its ring and counters, and the tail of the last launch
            self._lstate = self._tail = None
            if self.lag is not None:
                self._lstate = F_.pose_lag_state(lanes * self.K, self.lag, dev)
                lead = (self.lag + 1, lanes, self.K)
                self._tail = tuple(torch.zeros(lead + tail, dtype=dtype, device=dev) for tail, dtype in
                                   (((2,), torch.float32), ((2,), torch.float32), ((3,), torch.float32), ((), torch.int32),
                                    ((2,), torch.float32), ((2,), torch.float32), ((), torch.int32), ((), torch.float32)))
            self._history = None
            if history:
                from .smooth import TrackHistory
                self._history = TrackHistory((lanes, self.K), dev)
            # the tracker's measurements alone (csrc/pose_fit.hip) behind it: the frame's record, the launch's own copy of the decode,
            # and the recording; _fresh: the next pose is the first of a sequence
            self._meas = self._meas_decode = self._record = None
            if measurements:
                from .calibrate import MeasurementRecord
                self._meas = torch.zeros((lanes, self.K, F_.MEAS_FLOATS), dtype=torch.float32, device=dev)
                self._meas_decode = (torch.empty_like(self._idx), torch.empty_like(self._mx), torch.empty_like(self._kp))
                self._record = MeasurementRecord((lanes, self.K), dev, ratio=self.ratio, extent=(self.W * self.ratio, self.H * self.ratio))
            self._fresh = True
            # scene occupancy (csrc/cfar.hip): the threshold table, the detector's summary, the gate's state and verdict
            self._alpha = self._occ = self._gstate = self._present = None
            if presence is not None:
                self._alpha = F_.cfar_table(presence.pfa, presence.guard, presence.train, dev)
                self._occ = torch.zeros((lanes, 8), dtype=torch.float32, device=dev)
                self._gstate = F_.presence_state(lanes, dev)
                self._present = torch.zeros(lanes, dtype=torch.int32, device=dev)
            # interference blanking (csrc/interference.hip): the counts per sensor-frame and per group, the former as the frames show them
            self._if = self._if_stats = None
            if interference is not None:
                self._if = F_.InterferenceStats(torch.zeros((2 * lanes, 2), dtype=torch.int32, device=dev),
                                                torch.zeros((2 * lanes, 12, 2), dtype=torch.int32, device=dev))
                self._if_stats = self._if.frames.view(2, lanes, 2)
            self._done = torch.cuda.Event()
        self._graphs = {}              # "host" / "device" input -> (CUDAGraph, (heatmap, gcn_heatmap))
        self._eager_emits = 0
        self._busy = False

    # -- counters (host mirrors of the device state) ---------------------------------------------------------------------------
    @property
    def frames_pushed(self):
        return self.schedule.frames_pushed

    @property
    def frames_emitted(self):
        return self.schedule.frames_emitted

    # -- launches -------------------------------------------------------------------------------------------------------------
    def _front(self, flush, emit=True):
        """FFT chain to means on the 2 x lanes new sensor-frames (not for a flush), the window MNet, with ``presence`` the detector
        and the gate on the centre frame (only where a pose is due: ``emit``), the state advance."""
        L, s = rt.lib(), rt.stream()
        if not flush:
            adc, f = self._adc.view((2 * self.lanes,) + ADC_SHAPE), self.interference
            if f is not None:                      # in place on the session's copy of the frames: a workgroup holds its group before it writes
                F_.adc_interference(adc, f.K, f.guard, f.fill, out=adc, stats=self._if)
            pre.fft_chain_loader_means(adc, ws=self._ws, out=self._staging.view(2 * self.lanes, 16, 64, 64),
                                       tdm_compensation=self.tdm_compensation)
        ra, re = self.model.RAchirpNet.temporalConvWx1x1, self.model.REchirpNet.temporalConvWx1x1
        fn = L.hupr_mnet_stream_bf16act if self._bf16 else L.hupr_mnet_stream_f32
        rt.check(fn(None if flush else rt.ptr(self._staging), rt.ptr(self._ring), rt.ptr(self._state), self.lookahead, int(flush),
                    rt.ptr(ra.weight), rt.ptr(ra.bias), rt.ptr(re.weight), rt.ptr(re.bias), rt.ptr(self._maps[0]),
                    rt.ptr(self._maps[1]), self.lanes, self.G, self.pixels, s))
        g = self.presence
        if g is not None and emit:                 # the centre frame is in the ring by now, and the counters still name it
            rt.check(L.hupr_cfar_ra_stream_f32(rt.ptr(self._ring), rt.ptr(self._state), self.lookahead, int(flush), self.lanes, self.G,
                                               g.guard, g.train, rt.ptr(self._alpha), self._alpha.numel(), None, None,
                                               rt.ptr(self._occ), s))
            F_.presence_update(self._occ, self._gstate, g.min_cells, g.confirm, g.hold, out=self._present)
        rt.check(L.hupr_stream_advance(rt.ptr(self._state), self.lookahead, int(flush), s))

    def _back(self):
        """Encoders, decoder, heads on the window maps; arg-max of the GCN head; keypoints in image pixels."""
        heat, gcn = self.model.forward_chirp_maps(*self._maps)
        rows, t, f = self.lanes * self.K, self.track, self.smooth
        maps, refine = gcn.reshape(self.lanes, self.K, self.H, self.W), self.decode == "subpixel"
        # without a filter the decoded keypoints are the emitted ones (_kp); with one, _raw beside the filtered _kp and its velocity
        out = (self._idx, self._mx, self._kp, None, None) if self._raw is None else (self._idx, self._mx, self._raw, self._kp, self._vel)
        if t is not None:                              # the presence launches of _front precede this one on the same stream
            out += (self._cov, self._fc, self._status) + ((self._cxy, self._cscore, self._ccount, self._chosen) if t.associates else ())
            out += (self._source,) if t.pair_swap else ()
            out += (self._moving,) if t.maneuvers else ()
            F_.pose_track(maps, self.ratio, refine, self._tstate, t, self._present if t.gate_on_presence else None, out=out)
            if self.lag is not None:                   # reads what the tracker left, writes its own ring and tail only
                F_.pose_smooth_lag(self._tstate, self._status, self._kp, self._raw, self._mx, self._lstate, t, self.lag, out=self._tail)
            if self._meas is not None:                 # reads the maps only, writes buffers of its own
                F_.pose_measure(maps, self.ratio, refine, out=self._meas_decode + (self._meas,))
        elif self.decode == "integral":
            F_.pose_decode_integral(maps, self.ratio, self.decode_radius, self._fstate, f, out=out)
        elif self._fused:
            F_.pose_decode(maps, self.ratio, refine, self._fstate, f, out=out)
        else:
            F_.argmax_rows(maps.view(rows, self.H * self.W), out=(self._idx.view(rows), self._mx.view(rows)))
            rt.check(rt.lib().hupr_stream_keypoints_f32(rt.ptr(self._idx), rt.ptr(self._mx), rt.ptr(self._kp), rows, self.W, self.ratio,
                                                        rt.stream()))
        return heat, gcn

    def _capture(self, kind):
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            if kind == "host":
                self._adc.copy_(self._pinned, non_blocking=True)
            self._front(False)
            out = self._back()
        self._graphs[kind] = (g, out)
        return self._graphs[kind]

    def _wait(self):
        if self._busy:
            self._done.synchronize()
            self._busy = False

    def _frame(self, center, out, pushed=True):
        if self._history is not None:                          # the emitted pose into the history: eager copies behind the launches
            self._history.append(self._tstate, self._status, self._kp, self._raw, self._mx)
        if self._record is not None:                           # likewise the emitted pose's measurements
            self._record.append(self._meas, start=self._fresh)
            self._fresh = False
        fields = dict(frame=center, keypoints=self._kp, scores=self._mx, indices=self._idx, heatmap=out[0], gcn_heatmap=out[1],
                      raw_keypoints=self._raw, velocity=self._vel, present=self._present, occupancy=self._occ,
                      interference=self._if_stats if pushed else None)
        if self.track is None:
            return PoseFrame(**fields)
        fields.update(covariance=self._cov, forecast=self._fc, status=self._status, candidates=self._cxy, candidate_scores=self._cscore,
                      candidate_count=self._ccount, chosen=self._chosen)
        if self._moving is not None:
            return ManeuveringPoseFrame(moving=self._moving, **fields)
        if self.lag is None:
            return TrackedPoseFrame(**fields) if self._source is None else PairedPoseFrame(source=self._source, **fields)
        lagged = self._lagged(center, self.lag) if center >= self.lag else None
        if self._source is None:
            return LaggedTrackedPoseFrame(lagged=lagged, **fields)
        return LaggedPairedPoseFrame(source=self._source, lagged=lagged, **fields)

    def _lagged(self, newest, j):
        """Tail slot ``j`` of the last launch, whose newest pose was number ``newest``, as a LaggedPose of views."""
        return LaggedPose(newest - j, *[t[j] for t in self._tail])

    # -- public ---------------------------------------------------------------------------------------------------------------
    def push(self, adc_hori, adc_vert):
        check_frames(adc_hori, adc_vert, self.lanes)
        if self.schedule.ended:
            raise StreamEndedError("flush() ended this sequence; reset() starts a new one")
        host = not adc_hori.is_cuda
        if self.model.training:
            self.model.eval()
        with torch.cuda.device(self.device), torch.no_grad(), F_.math_mode(self.mode):
            if host:
                self._wait()                                   # the previous upload has left the pinned staging
                self._pinned[0].copy_(adc_hori)
                self._pinned[1].copy_(adc_vert)
            else:
                self._adc[0].copy_(adc_hori, non_blocking=True)
                self._adc[1].copy_(adc_vert, non_blocking=True)
            emit = self.schedule.frames_pushed >= self.lookahead
            if self.graph and emit and self._eager_emits >= WARMUP_PUSHES:
                kind = "host" if host else "device"
                g, out = self._graphs.get(kind) or self._capture(kind)
                self.model._refresh_packed(self.device)        # weights changed since the last push: one table launch, in place
                g.replay()
            else:
                if host:
                    self._adc.copy_(self._pinned, non_blocking=True)
                self._front(False, emit)
                out = None
                if emit:
                    out = self._back()
                    self._eager_emits += 1
            if host:
                self._done.record()
                self._busy = True
            due = self.schedule.push()
            return None if due is None else self._frame(due[0], out)

    def flush(self):
        frames = []
        if self.model.training:
            self.model.eval()
        with torch.cuda.device(self.device), torch.no_grad(), F_.math_mode(self.mode):
            for center, _ in self.schedule.flush():
                self._front(True)
                frames.append(self._frame(center, self._back(), pushed=False).clone())
        return frames

    def reset(self):
        with torch.cuda.device(self.device):
            rt.check(rt.lib().hupr_stream_reset(rt.ptr(self._state), rt.stream()))
            if self._fstate is not None:
                self._fstate.zero_()                           # "never seen": the next valid sample of a joint starts its filter
            if self._tstate is not None:
                self._tstate.zero_()                           # likewise: the next usable measurement of a joint starts its track
            if self._gstate is not None:
                self._gstate.zero_()                           # absent, no hits, no misses
            if self._lstate is not None:
                self._lstate.zero_()                           # a new sequence: an empty ring, every row's counter at 0
        self.schedule.reset()
        if self._history is not None:
            self._history.clear()
        self._fresh = True                                     # the measurement record stays: a fit may span sequences

    def lag_tail(self):
        """After ``flush()``: the ``min(lag, poses emitted)`` fixed-lag poses still owed at the end of a sequence, oldest first -> a
        list of ``LaggedPose`` (independent copies), from the slots lag-1 .. 0 of the last launch's tail: each is smoothed with all
        the poses there are behind it, the last one is the filter's own.  It launches nothing; needs a session built with ``lag``."""
        if self.lag is None:
            raise TrackingError("lag_tail() needs a session built with track=... and lag=...")
        emitted = self.schedule.frames_emitted
        with torch.cuda.device(self.device):
            return [self._lagged(emitted - 1, j).clone() for j in range(min(self.lag, emitted) - 1, -1, -1)]

    def smoothed(self):
        """The poses emitted since the last ``reset()``, smoothed backwards over the tracker's recorded states -> a
        ``SmoothedSequence`` of (T, lanes, K, ...) device tensors, T = the number of poses emitted (tools/smooth.py).  One launch,
        no sync; needs ``history=True`` and at least one emitted pose."""
        if self._history is None:
            raise TrackingError("smoothed() needs a session built with track=... and history=True")
        with torch.cuda.device(self.device):
            return self._history.smooth(self.track)

    @property
    def measurements(self):
        """The session's ``MeasurementRecord`` (None without ``measurements=True``): one frame per pose emitted since construction."""
        return self._record

    def fit_tracking(self, fit=("accel_psd", "meas_std", "heatmap_gain"), rounds=3):
        """The maximum-likelihood tracker noise parameters on the poses recorded so far -> ``tools.calibrate.TrackingFit``, whose
        ``tracking`` is a copy of the session's with the fitted values (``tools.calibrate.fit_tracking``: ``rounds`` launches of
        csrc/pose_fit.hip and a host read-back each).  The session goes on with the parameters it was built with.  Needs
        ``measurements=True`` and at least one emitted pose."""
        if self._record is None:
            raise TrackingError("fit_tracking() needs a session built with track=... and measurements=True")
        from .calibrate import fit_tracking
        with torch.cuda.device(self.device):
            return fit_tracking(self._record, self.track, fit, rounds)


# ---- command ---------------------------------------------------------------------------------------------------------------------
def parse(argv=None):
    p = argparse.ArgumentParser(prog="python -m hupr_amd.tools.stream", description="stream a raw capture frame by frame")
    p.add_argument("--config", type=str, default="mscsa_prgcn.yaml", help="config file (under ./config if that exists)")
    p.add_argument("--dir", type=str, default="test", help="logs/<dir>/model_best.pth holds the weights")
    p.add_argument("--raw", type=str, required=True, help="directory holding hori/adc_data.bin and vert/adc_data.bin")
    p.add_argument("--lookahead", type=int, default=None, help="frames of look-ahead (default G/2 - 1; 0 = zero latency)")
    p.add_argument("--math", choices=("f32", "bf16"), default=None, help="precision mode (default: the process default)")
    p.add_argument("--no-graph", action="store_true", help="eager launches instead of one hipGraph replay per frame")
    p.add_argument("--out", type=str, default="poses.json")
    p.add_argument("--decode", choices=DECODES, default="argmax", help="argmax: the reference's decode; subpixel: refined peaks; "
                   "integral: the mass centroid of a window around the peak")
    p.add_argument("--decode-radius", type=int, default=None, help="with --decode integral: the window radius in heat-map pixels "
                   "(default: the targets' patch radius; 0 = the whole map)")
    p.add_argument("--smooth", action="store_true", help="One-Euro filter over the keypoints (needs --rate); adds the velocity")
    p.add_argument("--rate", type=float, default=None, help="frames per second of the capture (required with --smooth)")
    p.add_argument("--track", action="store_true", help="Kalman filter per joint (needs --rate, excludes --smooth); adds velocity, "
                   "covariance, forecast and status")
    p.add_argument("--predict-now", action="store_true", help="with --track: forecast every joint to the newest frame (lookahead / rate)")
    p.add_argument("--accel-psd", type=float, default=None, help="with --track: white-acceleration power, pixel^2 / s^3 (default 200)")
    p.add_argument("--gate", type=float, default=None, help="with --track: largest accepted squared Mahalanobis distance (default 13.816)")
    p.add_argument("--max-coast", type=int, default=None, help="with --track: frames a track survives without a measurement (default 5)")
    p.add_argument("--track-candidates", type=int, default=None, help="with --track: heat-map peaks every track chooses its measurement "
                   "among, 1..4 (default 1: the strongest)")
    p.add_argument("--track-separation", type=int, default=None, help="with --track: two peaks lie more than this many heat-map pixels "
                   "apart (default 3)")
    p.add_argument("--track-peak-ratio", type=float, default=None, help="with --track: a further peak is at least this fraction of the "
                   "strongest (default 0.25)")
    p.add_argument("--track-on-presence", action="store_true", help="with --track and --presence: no measurement while the presence gate "
                   "sees nobody")
    p.add_argument("--track-pairs", action="store_true", help="with --track: assign the L_* / R_* partner joints jointly, so a left / "
                   "right exchange by the network is followed; every record gains candidates, chosen and source")
    p.add_argument("--track-swap-cost", type=float, default=None, help="with --track-pairs: cost added to a peak from the partner's "
                   "heat-map (default 0)")
    p.add_argument("--track-moving-psd", type=float, default=None, help="with --track: a second, moving model per joint with this "
                   "white-acceleration power (>= --accel-psd), mixed with the still one (interacting multiple models); every record "
                   "gains moving")
    p.add_argument("--track-switch-prob", type=float, default=None, help="with --track-moving-psd: probability per frame of changing "
                   "between the two models, in [0, 0.5] (default 0.05)")
    p.add_argument("--track-moving-prior", type=float, default=None, help="with --track-moving-psd: probability of the moving model in "
                   "a new track, in [0, 1] (default 0.5)")
    p.add_argument("--track-lag", type=int, default=None, help="with --track: fixed-lag smoothing over this many frames, 1..64; every "
                   "record gains lagged, lagged_velocity, lagged_covariance and lagged_flag, N frames after its own pose")
    p.add_argument("--rts", action="store_true", help="with --track: after the flush, smooth the whole recording backwards (Rauch-Tung-"
                   "Striebel); every record gains smoothed, smoothed_velocity, smoothed_covariance and smoothed_flag")
    p.add_argument("--fit-tracker", action="store_true", help="with --track: record what the tracker measured and, after the flush, print "
                   "the PoseTracking(...) whose accel_psd, meas_std and heatmap_gain are the maximum-likelihood fit to this capture; "
                   "nothing is written for it")
    p.add_argument("--tdm-compensation", action="store_true", help="compensate the TDM Doppler phase in the FFT chain (weights trained "
                   "with DATASET.tdmCompensation)")
    p.add_argument("--presence", action="store_true", help="scene occupancy: CA-CFAR detection on the centre frame and a presence gate; "
                   "every record gains present and occupancy")
    p.add_argument("--pfa", type=float, default=None, help="with --presence: design false-alarm probability per cell (default 1e-5)")
    p.add_argument("--cfar-guard", type=int, default=None, help="with --presence: half-width of the guard area (default 2)")
    p.add_argument("--cfar-train", type=int, default=None, help="with --presence: half-width of the training area beyond it (default 4)")
    p.add_argument("--min-cells", type=int, default=None, help="with --presence: detections that make a frame a hit (default 3)")
    p.add_argument("--confirm", type=int, default=None, help="with --presence: consecutive hits until present (default 2)")
    p.add_argument("--hold", type=int, default=None, help="with --presence: consecutive misses that are bridged (default 20)")
    p.add_argument("--interference", action="store_true", help="interference blanking of every pushed frame in front of the FFT chain; "
                   "every record gains interference")
    p.add_argument("--interference-threshold", type=int, default=None, help="with --interference: power ratio K over the chirp's median "
                   "residual power, in [2, 1024] (default 32)")
    p.add_argument("--interference-guard", type=int, default=None, help="with --interference: samples flagged on each side of a flagged "
                   "one, in [0, 8] (default 2)")
    p.add_argument("--interference-fill", choices=("clutter", "zero"), default=None, help="with --interference: what replaces a flagged "
                   "sample (default clutter)")
    p.add_argument("--weights", choices=WEIGHTS, default="live", help="live: model_state_dict as trained; averaged: ema_state_dict "
                   "(a run with TRAINING.emaDecay)")
    args = p.parse_args(argv)
    if args.smooth and args.rate is None:
        p.error("--smooth needs --rate (frames per second)")
    if args.track and args.rate is None:
        p.error("--track needs --rate (frames per second)")
    if args.track and args.smooth:
        p.error("--track and --smooth exclude each other: a session has one temporal filter")
    if args.track and args.decode == "integral":
        p.error("--track and --decode integral exclude each other: the tracker's measurement is the sub-pixel decode's")
    if args.decode_radius is not None and args.decode != "integral":
        p.error("--decode-radius needs --decode integral")
    if args.decode_radius is not None and args.decode_radius < 0:
        p.error("--decode-radius must be 0 (the whole map) or a positive number of heat-map pixels")
    if args.track and args.track_on_presence and not args.presence:
        p.error("--track-on-presence needs --presence")
    if args.track_swap_cost is not None and not args.track_pairs:
        p.error("--track-swap-cost needs --track-pairs")
    for flag, dest in (("--track-switch-prob", "track_switch_prob"), ("--track-moving-prior", "track_moving_prior")):
        if getattr(args, dest) is not None and args.track_moving_psd is None:
            p.error("%s needs --track-moving-psd" % flag)
    if args.track_moving_psd is not None and (args.rts or args.track_lag is not None):
        p.error("--track-moving-psd excludes --rts and --track-lag: the smoothers run over a single model's states")
    if args.track_lag is not None and not 1 <= args.track_lag <= F_.MAX_LAG:
        p.error("--track-lag must be an integer in 1..%d frames" % F_.MAX_LAG)
    # a dependent flag (given: neither None nor False) needs its switch; with the switch the settings object must build
    for switch, flags, build, error in (("--track", TRACK_FLAGS, tracking_from_args, TrackingError),
                                        ("--presence", PRESENCE_FLAGS, presence_from_args, PresenceError),
                                        ("--interference", INTERFERENCE_FLAGS, interference_from_args, ValueError)):
        if not getattr(args, switch[2:]):
            for flag, dest in flags:
                if getattr(args, dest) is not None and getattr(args, dest) is not False:
                    p.error("%s needs %s" % (flag, switch))
        else:
            try:
                build(args)
            except error as e:
                p.error(str(e))
    return args


TRACK_FLAGS = (("--predict-now", "predict_now"), ("--accel-psd", "accel_psd"), ("--gate", "gate"), ("--max-coast", "max_coast"),
               ("--rts", "rts"), ("--track-candidates", "track_candidates"), ("--track-separation", "track_separation"),
               ("--track-peak-ratio", "track_peak_ratio"), ("--track-on-presence", "track_on_presence"),
               ("--track-pairs", "track_pairs"), ("--track-swap-cost", "track_swap_cost"), ("--track-lag", "track_lag"),
               ("--fit-tracker", "fit_tracker"), ("--track-moving-psd", "track_moving_psd"),
               ("--track-switch-prob", "track_switch_prob"), ("--track-moving-prior", "track_moving_prior"))
INTERFERENCE_FLAGS = (("--interference-threshold", "interference_threshold"), ("--interference-guard", "interference_guard"),
                      ("--interference-fill", "interference_fill"))


def interference_from_args(args):
    """The InterferenceFilter of a parsed command line (None without --interference)."""
    if not args.interference:
        return None
    from ..preprocessing.interference import InterferenceFilter
    names = {"interference_threshold": "K", "interference_guard": "guard", "interference_fill": "fill"}
    try:
        return InterferenceFilter(**{names[dest]: getattr(args, dest) for _, dest in INTERFERENCE_FLAGS if getattr(args, dest) is not None})
    except ValueError as e:
        raise InterferenceError("--interference: %s" % e) from None


PRESENCE_FLAGS = (("--pfa", "pfa"), ("--cfar-guard", "cfar_guard"), ("--cfar-train", "cfar_train"), ("--min-cells", "min_cells"),
                  ("--confirm", "confirm"), ("--hold", "hold"))


def presence_from_args(args):
    """The PresenceGate of a parsed command line (None without --presence)."""
    if not args.presence:
        return None
    names = {"cfar_guard": "guard", "cfar_train": "train"}
    return PresenceGate(**{names.get(dest, dest): getattr(args, dest) for _, dest in PRESENCE_FLAGS if getattr(args, dest) is not None})


def tracking_from_args(args):
    """The PoseTracking of a parsed command line (None without --track)."""
    if not args.track:
        return None
    kw = {k: getattr(args, k) for k in ("accel_psd", "gate", "max_coast") if getattr(args, k) is not None}
    for dest, k in (("track_candidates", "candidates"), ("track_separation", "min_separation"), ("track_peak_ratio", "peak_ratio"),
                    ("track_swap_cost", "swap_cost"), ("track_moving_psd", "accel_psd_moving"), ("track_switch_prob", "switch_prob"),
                    ("track_moving_prior", "moving_prior")):
        if getattr(args, dest) is not None:
            kw[k] = getattr(args, dest)
    return PoseTracking(args.rate, gate_on_presence=args.track_on_presence, pair_swap=args.track_pairs, **kw)


def add_smoothed(records, seq, lane=0):
    """--rts: the smoothed pose of ``lane`` of a SmoothedSequence into the records of the same frames, in place."""
    seq = seq.cpu()
    if len(seq) != len(records):
        raise ValueError("%d smoothed frames for %d records" % (len(seq), len(records)))
    for k, rec in enumerate(records):
        rec["smoothed"] = [[float(x), float(y)] for x, y in seq.keypoints[k, lane].numpy()]
        rec["smoothed_velocity"] = [[float(vx), float(vy)] for vx, vy in seq.velocity[k, lane].numpy()]
        rec["smoothed_covariance"] = [[float(v) for v in c] for c in seq.covariance[k, lane].numpy()]
        rec["smoothed_flag"] = [int(c) for c in seq.flag[k, lane].numpy()]
    return records


def add_lagged(records, lagged, lane=0):
    """--track-lag: ``lane`` of a LaggedPose into the record of its frame (records[k] is frame k), in place."""
    lp = lagged.cpu()
    rec = records[lp.frame]
    if rec["frame"] != lp.frame:
        raise ValueError("record %d holds frame %d" % (lp.frame, rec["frame"]))
    rec["lagged"] = [[float(x), float(y)] for x, y in lp.keypoints[lane].numpy()]
    rec["lagged_velocity"] = [[float(vx), float(vy)] for vx, vy in lp.velocity[lane].numpy()]
    rec["lagged_covariance"] = [[float(v) for v in c] for c in lp.covariance[lane].numpy()]
    rec["lagged_flag"] = [int(c) for c in lp.flag[lane].numpy()]
    return records


def load_model_best(model, log_dir, device, weights="live", tdm_compensation=False, interference=None):
    """``model_best.pth`` of ``log_dir`` into ``model``, the way Runner.loadModelWeight reads it for evaluation.  ``weights``:
    ``"live"`` = ``model_state_dict``, the parameters as trained; ``"averaged"`` = ``ema_state_dict``, their moving average, which
    only a run with ``TRAINING.emaDecay`` saved.  ``tdm_compensation``: what the session will run, compared with what
    ``preprocess.json`` says the weights were trained with; ``interference`` (None or an InterferenceFilter) likewise."""
    if weights not in WEIGHTS:
        raise ValueError("weights must be one of %s, got %r" % (", ".join(WEIGHTS), weights))
    path = os.path.join(log_dir, "model_best.pth")
    if not os.path.exists(path):
        raise FileNotFoundError("%s not found" % path)
    ck = torch.load(path, map_location=device)
    if weights == "averaged":
        if "ema_state_dict" not in ck:
            raise KeyError("%s holds no averaged weights (ema_state_dict): it was trained without TRAINING.emaDecay; use "
                           "--weights live" % path)
        model.load_state_dict(ck["ema_state_dict"])
        print("==========>Load the averaged weights (ema_state_dict, %d updates)" % ck.get("ema_updates", 0))
    else:
        model.load_state_dict(ck["model_state_dict"])
    side = os.path.join(log_dir, "preprocess.json")
    if os.path.exists(side):
        from .base import tdm_mismatch_warning
        with open(side) as fp:
            recorded = json.load(fp)
        trained = recorded.get("fft_zero_doppler")
        if trained and trained != pre.ZERO_DOPPLER:
            print("==========>WARNING: these weights were trained with HUPR_FFT_ZERO_DOPPLER=%s, this process runs %s" % (trained, pre.ZERO_DOPPLER))
        warn = tdm_mismatch_warning(recorded, tdm_compensation)
        if warn:
            print(warn)
        from ..preprocessing.interference import interference_mismatch_warning
        warn = interference_mismatch_warning(recorded, interference)
        if warn:
            print(warn)
    print("==========>Load the model weight from %s, saved at epoch %d" % (log_dir, ck["epoch"]))


def main(argv=None):
    from ..config_tree import load_config
    from ..models import HuPRNet
    from ..preprocessing.process_iwr1843 import dca1000_frames
    args = parse(argv)
    if not torch.cuda.is_available():
        raise rt.HuprError("the live stream needs a GPU (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = load_config(args.config, "./config" if os.path.isdir("./config") else None)
    model = HuPRNet(cfg).to(dev).eval()
    load_model_best(model, os.path.join("./logs", args.dir), dev, weights=args.weights, tdm_compensation=args.tdm_compensation,
                    interference=interference_from_args(args))
    if args.math is not None:
        model.math_mode = args.math
    frames = []
    for sensor in ("hori", "vert"):
        raw = torch.from_numpy(np.fromfile(os.path.join(args.raw, sensor, "adc_data.bin"), dtype=np.int16)).to(dev)
        frames.append(dca1000_frames(raw))                      # (frames, 4, 192, 256, 2) int16, de-interleaved on the GPU
    n = min(frames[0].shape[0], frames[1].shape[0])
    session = PoseStream(model, cfg, lanes=1, lookahead=args.lookahead, graph=not args.no_graph, device=dev, decode=args.decode,
                         smooth=PoseSmoothing(args.rate) if args.smooth else None, track=tracking_from_args(args),
                         predict_now=args.predict_now, decode_radius=args.decode_radius, tdm_compensation=args.tdm_compensation,
                         history=args.rts, presence=presence_from_args(args), interference=interference_from_args(args),
                         lag=args.track_lag, measurements=args.fit_tracker)
    records = []

    def record(pf):
        kp = np.concatenate([pf.keypoints.cpu().numpy()[0], pf.scores.cpu().numpy()[0][:, None]], axis=1)
        records.append({"frame": int(pf.frame), "keypoints": [[float(x), float(y), float(s)] for x, y, s in kp]})
        if pf.velocity is not None:
            records[-1]["velocity"] = [[float(vx), float(vy)] for vx, vy in pf.velocity.cpu().numpy()[0]]
        if isinstance(pf, TrackedPoseFrame):
            records[-1]["covariance"] = [[float(v) for v in c] for c in pf.covariance.cpu().numpy()[0]]
            records[-1]["forecast"] = [[float(x), float(y)] for x, y in pf.forecast.cpu().numpy()[0]]
            records[-1]["status"] = [int(c) for c in pf.status.cpu().numpy()[0]]
            if pf.chosen is not None:
                records[-1]["candidates"] = [[[float(x), float(y), float(v)] for (x, y), v in zip(xy[:n], sc[:n])] for xy, sc, n in
                                             zip(pf.candidates.cpu().numpy()[0], pf.candidate_scores.cpu().numpy()[0],
                                                 pf.candidate_count.cpu().numpy()[0])]
                records[-1]["chosen"] = [int(c) for c in pf.chosen.cpu().numpy()[0]]
            if pf.source is not None:
                records[-1]["source"] = [int(c) for c in pf.source.cpu().numpy()[0]]
            if isinstance(pf, ManeuveringPoseFrame):
                records[-1]["moving"] = [float(v) for v in pf.moving.cpu().numpy()[0]]
        if pf.present is not None:
            records[-1]["present"] = int(pf.present.cpu().numpy()[0])
            records[-1]["occupancy"] = [float(v) for v in pf.occupancy.cpu().numpy()[0]]
        if pf.interference is not None:              # (sensor, {samples replaced, chirps touched}) of the frame this push brought in
            records[-1]["interference"] = [[int(v) for v in row] for row in pf.interference.cpu().numpy()[:, 0]]
        if pf.lagged is not None:                    # the pose of --track-lag frames ago falls due: into that frame's record
            add_lagged(records, pf.lagged)

    for i in range(n):
        pf = session.push(frames[0][i:i + 1], frames[1][i:i + 1])
        if pf is not None:
            record(pf)
    for pf in session.flush():
        record(pf)
    if args.track_lag is not None:
        for lp in session.lag_tail():                # the last frames' answers, each smoothed with all the frames there are
            add_lagged(records, lp)
    if args.rts and records:
        add_smoothed(records, session.smoothed())
    with open(args.out, "w") as fp:
        json.dump(records, fp)
    print("%d frames -> %s" % (len(records), args.out))
    if args.fit_tracker and records:                 # printed, not written: the values are for the next run's --accel-psd and TEST.tracking
        fitted = session.fit_tracking()
        print(fitted.line())
        print(fitted.tracking)
    return records


if __name__ == "__main__":
    main()
