"""Offline smoothing of tracked pose sequences: the Kalman tracker of the live stream (csrc/pose_track.hip) run over a sequence with
its per-frame states kept on the device, then one launch of the fixed-interval Rauch-Tung-Striebel smoother (csrc/pose_smooth.hip;
Rauch, Tung & Striebel 1965; the rule is stated beside hupr_pose_smooth_rts_f32 in include/hupr.h).  The answer for frame k then uses
the frames after it too: a gap the filter coasted through becomes an interpolation instead of an extrapolation.

``TrackHistory`` is the device-side record (it grows by doubling), ``SequenceSmoother`` a tracker state plus its history,
``SmoothedSequence`` what ``smooth()`` returns.  ``PoseStream(track=..., history=True)`` keeps a ``TrackHistory`` of its own, and
``Runner.eval`` walks a labelled test set through a ``SequenceSmoother`` under ``TEST.temporal`` (``temporal_setting``,
``SequenceWalker``).  ``jitter`` is the metric both print.

The smoother is a latency-bound recurrence (one thread per row, T dependent steps); nothing here claims a speed."""
import math

import numpy as np
import torch

from .. import functional as F_
from .stream import PoseTracking, TrackingError

FLAGS = ("SMOOTHED", "END", "PASSTHROUGH", "DEGENERATE")
TEMPORAL = ("off", "track", "rts")
DEFAULT_RATE_HZ = 10.0              # the HuPR capture rate
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
        if self.length == self._capacity:
            self._grow(2 * self._capacity)
        k = self.length
        for name, t in (("states", state), ("status", status), ("filtered", filtered), ("raw", raw), ("scores", scores)):
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


class SequenceSmoother:
    """A tracker (``functional.pose_track`` on a state of its own) that remembers: ``track(heat, ratio, refine)`` is one frame of
    ``rows`` heat-maps and returns ``pose_track``'s tuple (with ``tracking.candidates`` > 1 the associating tracker's twelve, with
    ``tracking.pair_swap`` — whose ``pairs`` must then fit the ``rows`` joints of a frame — those and ``source``);
    ``new_sequence()`` zeroes the state, so that the next frame starts new tracks and the smoother's chain breaks there by itself;
    ``smooth()`` smooths everything tracked so far in one launch."""

    def __init__(self, tracking, rows, device):
        if not isinstance(tracking, PoseTracking):
            raise TrackingError("tracking must be a PoseTracking, got %r" % (tracking,))
        if tracking.gate_on_presence:
            raise TrackingError("PoseTracking.gate_on_presence needs a live session with presence: there is no gate to ask here")
        if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or rows < 1:
            raise ValueError("rows must be a positive integer, got %r" % (rows,))
        if tracking.pair_swap and (tracking.pairs is None or len(tracking.pairs) != rows):
            raise TrackingError("PoseTracking.pair_swap needs pairs for the %d rows of a frame (PoseTracking.for_joints), got %r"
                                % (rows, tracking.pairs))
        self.tracking, self.rows, self.device = tracking, int(rows), torch.device(device)
        self.state = F_.pose_track_state(self.rows, self.device)
        self.history = TrackHistory((self.rows,), self.device)

    def __len__(self):
        return len(self.history)

    def track(self, heat, ratio, refine=True):
        out = F_.pose_track(heat, ratio, refine=refine, track_state=self.state, tracking=self.tracking)
        mx, raw, kp, status = out[1], out[2], out[3], out[7]
        self.history.append(self.state, status, kp, raw, mx)
        return out

    def new_sequence(self):
        self.state.zero_()

    def clear(self):
        """Forget the history and the tracks."""
        self.state.zero_()
        self.history.clear()

    def smooth(self):
        return self.history.smooth(self.tracking)


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
    """``TEST.temporal`` as read by ``temporal_setting``: ``mode`` "track" or "rts", ``tracking`` the PoseTracking of the run."""
    __slots__ = ("mode", "tracking")

    def __init__(self, mode, tracking):
        self.mode, self.tracking = mode, tracking


def temporal_setting(cfg):
    """``TEST.temporal`` / ``TEST.temporalRate`` / ``TEST.tracking`` (no keys of the reference's YAML) -> None with ``temporal`` absent
    or ``off``, else a TemporalSetting.  ``temporal``: ``off``, ``track`` (the Kalman filter's keypoints are scored) or ``rts`` (the
    smoothed ones).  ``temporalRate``: the frame rate in Hz, a positive finite number, absent = 10.0, the HuPR capture rate.
    ``tracking``: a mapping of PoseTracking keyword arguments other than ``rate_hz``.  All three are checked whatever ``temporal``
    says; anything else, and ``TEST.decode: integral`` beside ``track`` or ``rts`` (the tracker's measurement is the sub-pixel
    decode's, as in the live stream), raises here, where the config is read."""
    from ..misc.metrics import decode_setting
    test = getattr(cfg, "TEST", None)
    mode = getattr(test, "temporal", "off")
    if mode is False:                                   # YAML reads a bare off as False
        mode = "off"
    if not isinstance(mode, str) or mode not in TEMPORAL:
        raise ValueError("TEST.temporal must be 'off', 'track' or 'rts', got %r" % (mode,))
    rate = getattr(test, "temporalRate", DEFAULT_RATE_HZ)
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not math.isfinite(rate) or not rate > 0:
        raise ValueError("TEST.temporalRate must be a positive finite number (Hz), got %r" % (rate,))
    kw = getattr(test, "tracking", None)
    if kw is None:
        kw = {}
    elif not isinstance(kw, dict):                      # config_tree.obj: a YAML mapping as attributes
        if not hasattr(kw, "__dict__") or isinstance(kw, type):
            raise ValueError("TEST.tracking must be a mapping of PoseTracking arguments, got %r" % (kw,))
        kw = vars(kw)
    known = tuple(k for k in PoseTracking.ARGUMENTS + PoseTracking.PAIR_ARGUMENTS if k != "rate_hz")
    for k in kw:
        if k not in known:
            raise ValueError("TEST.tracking.%s is no PoseTracking argument (%s; the rate is TEST.temporalRate)" % (k, ", ".join(known)))
    try:
        tracking = PoseTracking(float(rate), **dict(kw))
        if tracking.pair_swap:                          # the partner table of this config's joints (None: their L_* / R_* names)
            tracking = tracking.for_joints(cfg.DATASET.idxToJoints)
    except TrackingError as e:
        raise ValueError("TEST.tracking: %s" % e) from None
    if mode == "off":
        return None
    if decode_setting(cfg) == "integral":
        raise ValueError("TEST.temporal: %s and TEST.decode: integral exclude each other: the tracker's measurement is the sub-pixel "
                         "decode's" % mode)
    return TemporalSetting(mode, tracking)


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
