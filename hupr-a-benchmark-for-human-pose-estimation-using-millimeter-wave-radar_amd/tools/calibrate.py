"""Fitting the Kalman tracker's noise parameters to a recording by maximum likelihood, without labels (Bar-Shalom, Li & Kirubarajan
2001, ch. 5 and 11.6; Abbeel et al., "Discriminative Training of Kalman Filters", RSS 2005): the filter's innovations have a
likelihood, and the ``accel_psd``, ``meas_std`` and ``heatmap_gain`` that maximise it over the recording replace the guessed defaults
of ``PoseTracking``.

``MeasurementRecord`` is the device-side recording — per frame and row the eight floats of ``functional.pose_measure``, all the
tracker reads of a frame — and ``fit_tracking`` the search: a few rounds of one ``functional.pose_track_nll`` launch each (csrc/
pose_fit.hip; the rule is stated beside hupr_pose_track_nll_f32 in include/hupr.h), every launch the whole recording under 810
candidates at once.  ``SequenceSmoother(..., measurements=True)`` and ``PoseStream(track=..., measurements=True)`` keep such a record;
``Runner.eval`` fits behind its scored walk under ``TEST.temporalFit`` and ``python -m hupr_amd.tools.stream --fit-tracker`` after a
capture.

The search is a latency-bound recurrence per (candidate, row); nothing here claims a speed."""
import numpy as np
import torch

from .. import functional as F_
from .stream import PoseTracking, TrackingError

FITTED = ("accel_psd", "meas_std", "heatmap_gain")          # in the order of a candidate's three numbers
STEPS = 9                                                   # log-spaced values per fitted parameter and round
FIRST_STEP = 4.0                                            # round 1's factor between neighbours; every round takes its fourth root
_FALLBACK = dict(accel_psd=200.0, meas_std=1.0, heatmap_gain=1.0)       # where a value of 0 is searched around: PoseTracking's defaults


class MeasurementRecord:
    """The tracker's measurements of a run on the device: per appended frame the ``meas`` tensor of ``functional.pose_measure``
    (``lead`` + (8,) floats) and whether the frame starts a sequence.  ``lead`` is the shape of one frame's rows, e.g. (rows,) or
    (lanes, K); ``ratio`` the image pixels per heat-map pixel the measurements were taken with and ``extent`` = (W ratio, H ratio) the
    image they live in, both read by the fit.  The buffers start at ``capacity`` frames and double when full, like ``TrackHistory``;
    ``append`` is one device-to-device copy and a fill on the current stream, no sync."""

    def __init__(self, lead, device, ratio=None, extent=None, capacity=64):
        self.lead = tuple(int(n) for n in lead)
        self.device = torch.device(device)
        self.ratio, self.extent = ratio, extent
        self.length = 0
        self._capacity = 0
        self._meas = self._start = None
        self._grow(max(int(capacity), 1))

    def _grow(self, capacity):
        meas = torch.empty((capacity,) + self.lead + (F_.MEAS_FLOATS,), dtype=torch.float32, device=self.device)
        start = torch.zeros(capacity, dtype=torch.int32, device=self.device)
        if self.length:
            meas[:self.length].copy_(self._meas[:self.length])
            start[:self.length].copy_(self._start[:self.length])
        self._meas, self._start, self._capacity = meas, start, capacity

    def clear(self):
        self.length = 0

    def __len__(self):
        return self.length

    def append(self, meas, start=False):
        """One frame: ``pose_measure``'s ``meas`` of it; ``start``: it is the first of a sequence, the tracks begin anew in front of it."""
        if self.length == self._capacity:
            self._grow(2 * self._capacity)
        k = self.length
        self._meas[k].copy_(meas.reshape(self._meas[k].shape), non_blocking=True)
        self._start[k].fill_(1 if start else 0)
        self.length = k + 1

    def views(self):
        """-> (meas (T, *lead, 8), start int32 (T,)): views of the T frames appended since the last ``clear``."""
        if self.length < 1:
            raise ValueError("the record is empty: no frame has been measured since it was cleared")
        return self._meas[:self.length], self._start[:self.length]


class TrackingFit:
    """What ``fit_tracking`` returns: ``tracking``, a copy of the settings it was given with the fitted values in place;
    ``cost_per_measurement`` = (at the starting values, at the fitted ones), the summed cost over the frames scored; ``counts``, six
    ints at the fitted values, summed over the rows: the frames per TRACK_* status in code order and the frames scored; ``grid`` =
    (candidates (G, 3) = accel_psd, meas_std, heatmap_gain; their summed costs (G,)) of the last round, NumPy arrays, for who wants to
    see how flat the minimum is; ``start_counts``, the six ints at the starting values."""
    __slots__ = ("tracking", "cost_per_measurement", "counts", "grid", "start_counts")

    def __init__(self, tracking, cost_per_measurement, counts, grid, start_counts):
        self.tracking, self.cost_per_measurement, self.counts = tracking, cost_per_measurement, counts
        self.grid, self.start_counts = grid, start_counts

    def __repr__(self):
        return "TrackingFit(%s, cost_per_measurement=(%.4f, %.4f), counts=%r)" % (
            ", ".join("%s=%.6g" % (k, getattr(self.tracking, k)) for k in FITTED), *self.cost_per_measurement, self.counts)

    def line(self):
        """The one line ``Runner.eval`` and the stream command print."""
        names = ("updated", "missing", "gated", "started", "lost", "scored")
        return "tracker fit: %s | cost per measurement %.4f configured, %.4f fitted | %s" % (
            ", ".join("%s %.6g" % (k, getattr(self.tracking, k)) for k in FITTED), *self.cost_per_measurement,
            ", ".join("%s %d" % kv for kv in zip(names, self.counts)))


def check_fit(fit, rounds):
    """``fit`` -> the tuple of its names in ``FITTED``' order; ``rounds`` an integer >= 1.  Anything else is a TrackingError."""
    if isinstance(fit, str):
        fit = (fit,)
    try:
        names = tuple(fit)
    except TypeError:
        raise TrackingError("fit must name parameters among %r, got %r" % (FITTED, fit)) from None
    if not names or any(k not in FITTED for k in names) or len(set(names)) != len(names):
        raise TrackingError("fit must name one or more of %r, each once, got %r" % (FITTED, fit))
    if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or rounds < 1:
        raise TrackingError("rounds must be a positive integer, got %r" % (rounds,))
    return tuple(k for k in FITTED if k in names), int(rounds)


def candidate_axes(values, centres, fit, step):
    """The values tried per parameter in one round -> three 1-D float64 arrays in ``FITTED``' order.  A fitted parameter gets ``STEPS``
    log-spaced values, ``step`` apart as a factor, centred on its current value ``values[k]`` (on ``centres[k]`` where that is 0,
    with the 0 itself appended, so the current value is always among them); ``heatmap_gain`` gets 0 as a tenth value in any case.  A
    parameter not in ``fit`` keeps its one value."""
    axes = []
    for k in FITTED:
        v = float(values[k])
        if k not in fit:
            axes.append(np.array([v]))
            continue
        c = v if v > 0 else float(centres[k])
        a = c * float(step) ** np.arange(-(STEPS // 2), STEPS // 2 + 1, dtype=np.float64)
        a[STEPS // 2] = c                                   # the centre itself, not step^0 times it
        if k == "heatmap_gain" or v == 0:
            a = np.append(a, 0.0)
        axes.append(a)
    return axes


def candidate_grid(axes):
    """The product of ``candidate_axes``' three -> (G, 3) float64, accel_psd the slowest axis and heatmap_gain the fastest."""
    q, s, h = np.meshgrid(*axes, indexing="ij")
    return np.stack([q.ravel(), s.ravel(), h.ravel()], axis=1)


def search(evaluate, tracking, fit=FITTED, rounds=3):
    """The search of ``fit_tracking`` over any evaluation: ``evaluate(candidates (G, 3) float64)`` -> (summed costs (G,) float64,
    counts (G, 6) summed over the rows, the index of the smallest cost, the lowest on ties).  -> TrackingFit."""
    if not isinstance(tracking, PoseTracking):
        raise TrackingError("tracking must be a PoseTracking, got %r" % (tracking,))
    fit, rounds = check_fit(fit, rounds)
    values = {k: float(getattr(tracking, k)) for k in FITTED}
    centres = dict(_FALLBACK)
    step, before, start_counts = FIRST_STEP, None, None
    for _ in range(rounds):
        for k in FITTED:
            if values[k] > 0:
                centres[k] = values[k]
        axes = candidate_axes(values, centres, fit, step)
        grid = candidate_grid(axes)
        costs, counts, best = evaluate(grid)
        costs, counts, best = np.asarray(costs, dtype=np.float64), np.asarray(counts), int(best)
        if before is None:                                  # round 1 holds the starting values: the fit never costs more than they do
            at = int(np.flatnonzero((grid == np.array([values[k] for k in FITTED])).all(axis=1))[0])
            before, start_counts = costs[at] / max(int(counts[at, 5]), 1), tuple(int(c) for c in counts[at])
        values = dict(zip(FITTED, (float(v) for v in grid[best])))
        step = step ** 0.25
    if tracking.maneuvers:                                  # two models: the single-model accel_psd fits neither, both stay as given
        values["accel_psd"] = float(tracking.accel_psd)
    fitted = tracking._copy(**values)
    after = costs[best] / max(int(counts[best, 5]), 1)
    return TrackingFit(fitted, (float(before), float(after)), tuple(int(c) for c in counts[best]), (grid, costs), start_counts)


def fit_tracking(record, tracking, fit=FITTED, rounds=3):
    """Maximum-likelihood values of the tracker's noise parameters on a recording -> TrackingFit.  ``record`` a MeasurementRecord with
    its ``ratio`` and ``extent``; ``tracking`` the PoseTracking the search starts from and whose other settings (``rate_hz``, ``gate``,
    ``max_coast``, ``init_speed_std``, ``min_score``) every candidate shares; ``fit`` which of ``accel_psd``, ``meas_std`` and
    ``heatmap_gain`` to fit, the others stay fixed.  Per round, 9 log-spaced values per fitted parameter centred on the current ones
    — a factor of 4 apart in round 1, 4^(1/4) in round 2, 4^(1/16) in round 3, so every round spans one step of the one before on
    both sides — and ``heatmap_gain`` = 0 as a tenth value: 810 candidates with all three, one launch.  A candidate's cost is the
    sum over rows and frames of min(d2 + ln det S, outlier cost) (``functional.pose_track_nll``), summed over the rows in fp64 on the
    device; the smallest wins, the lowest index on ties.  Round 1 contains the starting values, so the fitted cost is never above the
    starting cost.  One host read-back per round.
    The fit is defined for the plain tracker's measurement, the arg-max peak: a ``tracking`` with ``candidates`` > 1, ``pair_swap`` or
    ``gate_on_presence`` is fitted as the plain tracker — one candidate, no partner rows, no presence flags — and the three fitted
    numbers are carried over into the copy, whose other settings stay.  A ``tracking`` with ``accel_psd_moving`` is fitted as the
    plain single-model tracker too, and only ``meas_std`` and ``heatmap_gain`` are carried over: ``accel_psd`` and
    ``accel_psd_moving`` stay as given (fitting the two models by likelihood is not built)."""
    if not isinstance(record, MeasurementRecord):
        raise TrackingError("record must be a MeasurementRecord, got %r" % (record,))
    if record.ratio is None or record.extent is None:
        raise TrackingError("the record needs its ratio and extent: the image the measurements live in")
    meas, start = record.views()

    def evaluate(grid):
        nll, counts, _ = F_.pose_track_nll(meas, start, tracking, grid, record.extent, record.ratio)
        G = grid.shape[0]
        costs = nll.reshape(G, -1).sum(dim=1)                                           # fp64, on the device
        best = torch.argmin(costs)                                                      # the first of equal minima
        total = counts.reshape(G, -1, 6).sum(dim=1)
        return costs.cpu().numpy(), total.cpu().numpy(), int(best.item())

    return search(evaluate, tracking, fit, rounds)
