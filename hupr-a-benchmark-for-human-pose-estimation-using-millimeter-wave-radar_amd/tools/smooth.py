"""Offline smoothing of tracked pose sequences: the Kalman tracker of the live stream (csrc/pose_track.hip) run over a sequence with
its per-frame states kept on the device, then one launch of the fixed-interval Rauch-Tung-Striebel smoother (csrc/pose_smooth.hip;
Rauch, Tung & Striebel 1965; the rule is stated beside hupr_pose_smooth_rts_f32 in include/hupr.h).  The answer for frame k then uses
the frames after it too: a gap the filter coasted through becomes an interpolation instead of an extrapolation.

``TrackHistory`` is the device-side record (it grows by doubling), ``SequenceSmoother`` a tracker state plus its history,
``SmoothedSequence`` what ``smooth()`` returns.  ``PoseStream(track=..., history=True)`` keeps a ``TrackHistory`` of its own, and
``Runner.eval`` walks a labelled test set through a ``SequenceSmoother`` under ``TEST.temporal`` (``temporal_setting``,
``SequenceWalker``).  ``jitter`` is the metric both print.

``SequenceSmoother(..., lag=L)`` also runs the fixed-lag smoother of the live stream behind every tracked frame (csrc/pose_lag.hip,
hupr_pose_smooth_lag_f32: the backward pass over the last L + 1 frames only) and keeps its answers, ``smooth_lagged()`` returns them and
``TEST.temporal: lag`` scores them: what a live consumer that waits L frames would have seen.

``SequenceSmoother(..., measurements=True)`` also records every frame's measurements (csrc/pose_fit.hip, ``functional.pose_measure``)
for ``fit_tracking()``, the maximum-likelihood fit of the tracker's noise parameters (tools/calibrate.py); ``TEST.temporalFit`` asks
``Runner.eval`` for it.

The smoother is a latency-bound recurrence (one thread per row, T dependent steps); nothing here claims a speed."""
import math

import numpy as np
import torch

from .. import functional as F_
from .calibrate import FITTED, MeasurementRecord, fit_tracking
from .stream import PoseTracking, TrackingError

FLAGS = ("SMOOTHED", "END", "PASSTHROUGH", "DEGENERATE", "EMPTY")
TEMPORAL = ("off", "track", "rts", "lag")
DEFAULT_RATE_HZ = 10.0              # the HuPR capture rate
DEFAULT_LAG = 4                     # frames: 0.4 s at that rate (PAPERS.md has what the lag buys on the tracker tests' scenario)
SEQUENCE_STRIDE = 100000            # image_id = frame + 100000 * sequence (datasets/base.py)


class SmoothedSequence:
    """A tracked sequence and its smoothed version, T frames of ``lead`` rows each, device tensors: ``keypoints`` (T, *lead, 2) the
    smoothed keypoints, ``velocity`` (T, *lead, 2) per second, ``covariance`` (T, *lead, 3) = (Pxx, Pxy, Pyy), ``flag`` int32
    (T, *lead) one of ``FLAGS``' codes; and what the filter gave, frame by frame: ``filtered`` its keypoints, ``raw`` the decoded
    ones, ``status`` its status codes, ``scores`` the heat-map maxima."""
    __slots__ = ("keypoints", "velocity", "covariance", "flag", "filtered", "raw", "status", "scores")

    def __init__(self, keypoints, velocity, covariance, flag, filtered, raw, status, scores):
        self.keypoints, self.velocity, self.covariance, self.flag = keypoints, velocity, covariance, flag
        self.filtered, self.raw, self.status, self.scores = filtered, raw, status, scores

    def __len__(self):
        return int(self.status.shape[0])

    def cpu(self):
        """Host copies (synchronises)."""
        return SmoothedSequence(*[None if getattr(self, k) is None else getattr(self, k).cpu() for k in self.__slots__])


class TrackHistory:
    """The per-frame record of a tracker on the device: state snapshot (16 floats per row), status, filtered and raw keypoints and
    maxima of every appended frame.  ``lead`` is the shape of one frame's rows, e.g. (rows,) or (lanes, K).  The buffers start at
    ``capacity`` frames and double when full; ``append`` is five device-to-device copies on the current stream, no sync."""
    _FIELDS = (("states", (16,), torch.float32), ("status", (), torch.int32), ("filtered", (2,), torch.float32),
               ("raw", (2,), torch.float32), ("scores", (), torch.float32))

    def __init__(self, lead, device, capacity=64):
        self.lead = tuple(int(n) for n in lead)
        self.device = torch.device(device)
        self.length = 0
        self._capacity = 0
        self._buf = {}
        self._grow(max(int(capacity), 1))

    def _grow(self, capacity):
        for name, tail, dtype in self._FIELDS:
            new = torch.empty((capacity,) + self.lead + tail, dtype=dtype, device=self.device)
            if self.length:
                new[:self.length].copy_(self._buf[name][:self.length])
            self._buf[name] = new
        self._capacity = capacity

    def clear(self):
        self.length = 0

    def __len__(self):
        return self.length

    def append(self, state, status, filtered, raw, scores):
        """One frame: the tracker's state tensor right after the frame's launch and that launch's outputs."""
        self._append((state, status, filtered, raw, scores))

    def _append(self, values):
        """One frame: a tensor per entry of ``_FIELDS``, in that order."""
        if self.length == self._capacity:
            self._grow(2 * self._capacity)
        k = self.length
        for (name, _, _), t in zip(self._FIELDS, values):
            dst = self._buf[name][k]
            dst.copy_(t.reshape(dst.shape), non_blocking=True)
        self.length = k + 1

    def _views(self):
        if self.length < 1:
            raise ValueError("the history is empty: no frame has been tracked since it was cleared")
        return {name: self._buf[name][:self.length] for name, _, _ in self._FIELDS}

    def record(self):
        """What the filter gave, without the backward pass: a SmoothedSequence whose ``keypoints`` / ``velocity`` / ``covariance``
        / ``flag`` are None.  No launch but the copies."""
        b = self._views()
        return SmoothedSequence(None, None, None, None, b["filtered"].clone(), b["raw"].clone(), b["status"].clone(), b["scores"].clone())

    def smooth(self, tracking):
        """One launch over the whole history -> SmoothedSequence (independent of the history's buffers).  An empty history is an
        error: there is nothing to smooth."""
        b = self._views()
        kp, vel, cov, flag = F_.pose_smooth_rts(b["states"], b["status"], b["filtered"], tracking)
        return SmoothedSequence(kp, vel, cov, flag, b["filtered"].clone(), b["raw"].clone(), b["status"].clone(), b["scores"].clone())


class ManeuverHistory(TrackHistory):
    """The per-frame record of the two-model tracker (``PoseTracking.accel_psd_moving``): status, filtered and raw keypoints, maxima
    and ``moving``, the probability of the moving model.  No states: the smoothers run over a single model's, so ``smooth`` raises."""
    _FIELDS = TrackHistory._FIELDS[1:] + (("moving", (), torch.float32),)

    def append(self, state, status, filtered, raw, scores, moving):
        self._append((status, filtered, raw, scores, moving))

    def smooth(self, tracking):
        raise TrackingError("no smoothing with PoseTracking.accel_psd_moving: the Rauch-Tung-Striebel kernels smooth a single model's states")

    def moving_mean(self):
        """-> (the mean ``moving`` over the rows and frames with a live track (status not LOST), their number); synchronises."""
        b = self._views()
        live = b["status"] != F_.TRACK_LOST
        n = int(live.sum().item())
        return (float(b["moving"][live].double().mean().item()) if n else float("nan")), n


class LagRecord(TrackHistory):
    """The fixed-lag answers of the frames of a ``TrackHistory``, position by position: ``append(tail)`` takes a new frame with the
    tail of its launch (``functional.pose_smooth_lag``) — the frame enters with tail slot 0, the filter's own pose, and the frame
    ``lag`` positions back gets slot ``lag`` once ``due``; ``settle(tail, m)`` gives the last ``m`` frames the slots m-1 .. 0, what
    they are owed when nothing follows.  Device-to-device copies on the current stream, no sync."""
    _FIELDS = (("keypoints", (2,), torch.float32), ("velocity", (2,), torch.float32), ("covariance", (3,), torch.float32),
               ("flag", (), torch.int32))

    def append(self, tail, lag, due):
        self._append(tuple(t[0] for t in tail[:4]))
        if due:
            for (name, _, _), t in zip(self._FIELDS, tail):
                self._buf[name][self.length - 1 - lag].copy_(t[lag].reshape(self._buf[name].shape[1:]), non_blocking=True)

    def settle(self, tail, m):
        for (name, _, _), t in zip(self._FIELDS, tail):
            if m:
                dst = self._buf[name][self.length - m:self.length]
                dst.copy_(t[:m].flip(0).reshape(dst.shape), non_blocking=True)

    def views(self):
        return tuple(self._views()[name] for name, _, _ in self._FIELDS)


class SequenceSmoother:
    """A tracker (``functional.pose_track`` on a state of its own) that remembers: ``track(heat, ratio, refine)`` is one frame of
    ``rows`` heat-maps and returns ``pose_track``'s tuple (with ``tracking.candidates`` > 1 the associating tracker's twelve, with
    ``tracking.pair_swap`` — whose ``pairs`` must then fit the ``rows`` joints of a frame — those and ``source``);
    ``new_sequence()`` zeroes the state, so that the next frame starts new tracks and the smoother's chain breaks there by itself;
    ``smooth()`` smooths everything tracked so far in one launch.
    ``lag=L`` (an integer in 1..64; None, the default, adds nothing): ``track`` also runs the fixed-lag smoother's launch behind the
    tracker's (``functional.pose_smooth_lag`` on a lag state of its own) and keeps tail slot L, the answer for the frame L calls
    back; ``smooth_lagged()`` returns the fixed-lag answers of every frame tracked so far, those of a sequence's last L frames taken
    from the tail of its last launch; ``new_sequence()`` takes them before it zeroes the lag state too.
    ``measurements=True``: ``track`` also launches ``functional.pose_measure`` on the frame's maps and files its measurements in
    ``record``, a ``MeasurementRecord`` (tools/calibrate.py) that ``fit_tracking`` reads; the frame after ``new_sequence()`` is marked
    as a sequence's first.  The tracker's own launch and outputs are what they are without it.
    With ``tracking.accel_psd_moving`` the tracker is the two-model one (csrc/pose_imm.hip) on a state of 32 floats per row: ``track``
    returns its nine outputs, and ``history`` (a ``ManeuverHistory``) records keypoints, status, raw keypoints, scores and ``moving``;
    ``lag``, ``smooth()`` and ``smooth_lagged()`` raise, because the smoothers run over a single model's states."""

    def __init__(self, tracking, rows, device, lag=None, measurements=False):
        if not isinstance(tracking, PoseTracking):
            raise TrackingError("tracking must be a PoseTracking, got %r" % (tracking,))
        if tracking.gate_on_presence:
            raise TrackingError("PoseTracking.gate_on_presence needs a live session with presence: there is no gate to ask here")
        if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or rows < 1:
            raise ValueError("rows must be a positive integer, got %r" % (rows,))
        if tracking.pair_swap and (tracking.pairs is None or len(tracking.pairs) != rows):
            raise TrackingError("PoseTracking.pair_swap needs pairs for the %d rows of a frame (PoseTracking.for_joints), got %r"
                                % (rows, tracking.pairs))
        if tracking.maneuvers and lag is not None:
            raise TrackingError("lag and PoseTracking.accel_psd_moving exclude each other: the smoother runs over a single model's states")
        self.tracking, self.rows, self.device = tracking, int(rows), torch.device(device)
        self.state = (F_.pose_imm_state if tracking.maneuvers else F_.pose_track_state)(self.rows, self.device)
        self.history = (ManeuverHistory if tracking.maneuvers else TrackHistory)((self.rows,), self.device)
        self.lag = None if lag is None else F_.check_lag(lag, "SequenceSmoother: lag")
        if self.lag is not None:
            self.lag_state = F_.pose_lag_state(self.rows, self.lag, self.device)
            self.lagged = LagRecord((self.rows,), self.device)
            self._tail, self._run = None, 0                    # the last launch's tail; frames tracked in the current sequence
        if not isinstance(measurements, bool):
            raise ValueError("measurements must be True or False, got %r" % (measurements,))
        self.record = MeasurementRecord((self.rows,), self.device) if measurements else None
        self._first = True                                     # the next frame starts a sequence

    def __len__(self):
        return len(self.history)

    def track(self, heat, ratio, refine=True):
        out = F_.pose_track(heat, ratio, refine=refine, track_state=self.state, tracking=self.tracking)
        mx, raw, kp, status = out[1], out[2], out[3], out[7]
        self.history.append(self.state, status, kp, raw, mx, *out[8:9] if self.tracking.maneuvers else ())
        if self.record is not None:
            self.record.ratio, self.record.extent = float(ratio), (heat.shape[-1] * float(ratio), heat.shape[-2] * float(ratio))
            self.record.append(F_.pose_measure(heat, ratio, refine=refine)[3], start=self._first)
            self._first = False
        if self.lag is not None:
            lead = (self.rows,)
            self._tail = F_.pose_smooth_lag(self.state, status.reshape(lead), kp.reshape(lead + (2,)), raw.reshape(lead + (2,)),
                                            mx.reshape(lead), self.lag_state, self.tracking, self.lag, out=self._tail)
            self._run += 1
            self.lagged.append(self._tail, self.lag, self._run > self.lag)
        return out

    def _settle(self):
        """The current sequence's last frames get what the tail of its last launch owes them (again after every further frame)."""
        if self.lag is not None and self._run:
            self.lagged.settle(self._tail, min(self.lag, self._run))

    def new_sequence(self):
        self._settle()
        self.state.zero_()
        self._first = True
        if self.lag is not None:
            self.lag_state.zero_()
            self._run = 0

    def clear(self):
        """Forget the history, the measurements and the tracks."""
        self.state.zero_()
        self.history.clear()
        self._first = True
        if self.record is not None:
            self.record.clear()
        if self.lag is not None:
            self.lag_state.zero_()
            self.lagged.clear()
            self._run = 0

    def smooth(self):
        return self.history.smooth(self.tracking)

    def fit_tracking(self, fit=FITTED, rounds=3):
        """``tools.calibrate.fit_tracking`` on the measurements of every frame tracked so far -> TrackingFit; needs
        ``measurements=True``."""
        if self.record is None:
            raise TrackingError("fit_tracking() needs a SequenceSmoother built with measurements=True")
        return fit_tracking(self.record, self.tracking, fit, rounds)

    def smooth_lagged(self):
        """-> SmoothedSequence of the fixed-lag answers of every frame tracked so far: frame k smoothed over the ``lag`` frames behind
        it, or over those its sequence still had.  No launch but the copies; needs ``lag``."""
        if self.lag is None:
            raise TrackingError("smooth_lagged() needs a SequenceSmoother built with lag=...")
        self._settle()
        rec = self.history.record()
        return SmoothedSequence(*[t.clone() for t in self.lagged.views()], rec.filtered, rec.raw, rec.status, rec.scores)


def jitter(keypoints):
    """The rms second difference along time of ``keypoints`` (T, ..., 2) — an array, a tensor, or a list of them, one per sequence,
    whose second differences are pooled — over every frame, row and axis, in the keypoints' unit.  A steady motion has little of it, a
    decode that jumps from frame to frame much.  NaN where no sequence has three frames."""
    seqs = keypoints if isinstance(keypoints, (list, tuple)) else [keypoints]
    parts = []
    for k in seqs:
        k = k.detach().cpu().numpy() if isinstance(k, torch.Tensor) else np.asarray(k)
        k = k.astype(np.float64)
        if k.shape[0] >= 3:
            parts.append((k[2:] - 2.0 * k[1:-1] + k[:-2]).ravel())
    if not parts:
        return float("nan")
    return float(np.sqrt(np.mean(np.concatenate(parts) ** 2)))


# ---- Runner.eval under TEST.temporal -----------------------------------------------------------------------------------------------------
class TemporalSetting:
    """``TEST.temporal`` as read by ``temporal_setting``: ``mode`` "track", "rts" or "lag", ``tracking`` the PoseTracking of the run,
    ``lag`` the frames of ``TEST.temporalLag`` (read by "lag" only), ``fit`` whether ``TEST.temporalFit`` asks for the tracker's noise
    parameters to be fitted behind the walk (tools/calibrate.py)."""
    __slots__ = ("mode", "tracking", "lag", "fit")

    def __init__(self, mode, tracking, lag=DEFAULT_LAG, fit=False):
        self.mode, self.tracking, self.lag, self.fit = mode, tracking, lag, fit


def temporal_setting(cfg):
    """``TEST.temporal`` / ``TEST.temporalRate`` / ``TEST.temporalLag`` / ``TEST.tracking`` (no keys of the reference's YAML) -> None
    with ``temporal`` absent or ``off``, else a TemporalSetting.  ``temporal``: ``off``, ``track`` (the Kalman filter's keypoints
    are scored), ``rts`` (the smoothed ones) or ``lag`` (the fixed-lag smoothed ones, what a live consumer ``temporalLag`` frames
    late would see).  ``temporalRate``: the frame rate in Hz, a positive finite number, absent = 10.0, the HuPR capture rate.
    ``temporalLag``: an integer in 1..64 frames, absent = 4.  ``tracking``: a mapping of PoseTracking keyword arguments other than
    ``rate_hz``.  All four are checked whatever ``temporal`` says; anything else, and ``TEST.decode: integral`` beside ``track``,
    ``rts`` or ``lag`` (the tracker's measurement is the sub-pixel decode's, as in the live stream), raises here, where the config is
    read.  ``TEST.temporalFit`` (no key of the reference's YAML either): absent or ``false`` is off; ``true`` needs ``temporal`` to be
    something other than ``off`` and makes ``Runner.eval`` fit ``accel_psd``, ``meas_std`` and ``heatmap_gain`` to the walked frames'
    measurements and print them (``tools.calibrate.fit_tracking``); anything but a bool raises here.  ``tracking.accel_psd_moving``
    (with ``switch_prob`` and ``moving_prior``) turns the two-model tracker on: ``temporal: track`` scores it, ``rts`` and ``lag``
    beside it raise here."""
    from ..misc.metrics import decode_setting
    test = getattr(cfg, "TEST", None)
    mode = getattr(test, "temporal", "off")
    if mode is False:                                   # YAML reads a bare off as False
        mode = "off"
    if not isinstance(mode, str) or mode not in TEMPORAL:
        raise ValueError("TEST.temporal must be 'off', 'track', 'rts' or 'lag', got %r" % (mode,))
    rate = getattr(test, "temporalRate", DEFAULT_RATE_HZ)
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not math.isfinite(rate) or not rate > 0:
        raise ValueError("TEST.temporalRate must be a positive finite number (Hz), got %r" % (rate,))
    lag = getattr(test, "temporalLag", DEFAULT_LAG)
    if isinstance(lag, bool) or not isinstance(lag, (int, np.integer)) or not 1 <= lag <= F_.MAX_LAG:
        raise ValueError("TEST.temporalLag must be an integer in 1..%d (frames), got %r" % (F_.MAX_LAG, lag))
    kw = getattr(test, "tracking", None)
    if kw is None:
        kw = {}
    elif not isinstance(kw, dict):                      # config_tree.obj: a YAML mapping as attributes
        if not hasattr(kw, "__dict__") or isinstance(kw, type):
            raise ValueError("TEST.tracking must be a mapping of PoseTracking arguments, got %r" % (kw,))
        kw = vars(kw)
    known = tuple(k for k in PoseTracking.ARGUMENTS + PoseTracking.PAIR_ARGUMENTS + PoseTracking.MANEUVER_ARGUMENTS if k != "rate_hz")
    for k in kw:
        if k not in known:
            raise ValueError("TEST.tracking.%s is no PoseTracking argument (%s; the rate is TEST.temporalRate)" % (k, ", ".join(known)))
    try:
        tracking = PoseTracking(float(rate), **dict(kw))
        if tracking.pair_swap:                          # the partner table of this config's joints (None: their L_* / R_* names)
            tracking = tracking.for_joints(cfg.DATASET.idxToJoints)
    except TrackingError as e:
        raise ValueError("TEST.tracking: %s" % e) from None
    fit = getattr(test, "temporalFit", False)
    if not isinstance(fit, bool):
        raise ValueError("TEST.temporalFit must be true or false, got %r" % (fit,))
    if fit and mode == "off":
        raise ValueError("TEST.temporalFit: true needs TEST.temporal: track, rts or lag: the fit reads the frames that walk tracks")
    if mode == "off":
        return None
    if decode_setting(cfg) == "integral":
        raise ValueError("TEST.temporal: %s and TEST.decode: integral exclude each other: the tracker's measurement is the sub-pixel "
                         "decode's" % mode)
    if tracking.maneuvers and mode in ("rts", "lag"):
        raise ValueError("TEST.temporal: %s and TEST.tracking.accel_psd_moving exclude each other: the smoothers run over a single "
                         "model's states; TEST.temporal: track scores the two-model tracker" % mode)
    return TemporalSetting(mode, tracking, int(lag), fit)


def sequence_and_frame(image_id):
    """image_id = frame + 100000 * sequence -> (sequence, frame)."""
    image_id = int(image_id)
    if image_id < 0:
        raise ValueError("image_id must not be negative, got %r" % (image_id,))
    return image_id // SEQUENCE_STRIDE, image_id % SEQUENCE_STRIDE


class SequenceWalker:
    """Walks image ids in loader order: ``step(image_id)`` -> True where the tracker state has to be zeroed in front of this frame (the
    first frame, a new sequence, or a frame that is not its predecessor + 1).  ``starts`` lists the positions of those frames."""

    def __init__(self):
        self.last = None
        self.count = 0
        self.starts = []

    def step(self, image_id):
        seq, frame = sequence_and_frame(image_id)
        reset = self.last is None or self.last != (seq, frame - 1)
        if reset:
            self.starts.append(self.count)
        self.last = (seq, frame)
        self.count += 1
        return reset

    def segments(self):
        """-> [(first, end)] positions of the runs of consecutive frames walked so far."""
        ends = self.starts[1:] + [self.count]
        return list(zip(self.starts, ends))
