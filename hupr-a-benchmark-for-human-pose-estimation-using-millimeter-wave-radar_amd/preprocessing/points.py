"""Radar point cloud, offline: the CA-CFAR detections of both sensors thinned to local power maxima, refined to sub-cell (range,
azimuth) points, paired across the sensors and turned into metres (csrc/radar_points.hip; the rules are stated beside
hupr_radar_peaks_f32 and hupr_radar_points_fuse_f32 in include/hupr.h).  The stage between "7 x 64 x 64 flags" and "where are the
movers".  The separations and gates default to guesses, as the detector's settings do: nobody has run this on a real capture.
"""
import math

import numpy as np
import torch

from .cfar import CFAR_DEFAULTS, check_cfar

POINT_DEFAULTS = {"sep_range": 1, "sep_azimuth": 4, "range_gate": 1.5, "doppler_gate": 1, "max_points": 64}
POINT_LIMITS = {"sep_range": (0, 4), "sep_azimuth": (0, 8), "doppler_gate": (0, 7), "max_points": (1, 256)}      # csrc/radar_points_host.h


def check_points(**settings):
    """Any of ``sep_range``, ``sep_azimuth``, ``range_gate``, ``doppler_gate``, ``max_points`` -> a dict of the same keys with plain
    int / float values; ValueError for an unknown key, a value of the wrong kind (a bool, a float where an integer is asked for) or one
    outside its limits: 0 <= sep_range <= 4, 0 <= sep_azimuth <= 8, range_gate finite and >= 0, 0 <= doppler_gate <= 7,
    1 <= max_points <= 256."""
    out = {}
    for k, v in settings.items():
        if k == "range_gate":
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v < 0:
                raise ValueError("range_gate must be a finite number >= 0, got %r" % (v,))
            out[k] = float(v)
        elif k in POINT_LIMITS:
            lo, hi = POINT_LIMITS[k]
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError("%s must be an integer in %d..%d, got %r" % (k, lo, hi, v))
            out[k] = int(v)
        else:
            raise ValueError("check_points: unknown setting %r" % (k,))
    return out


class PointCloudSettings:
    """The settings of ``radar_point_cloud`` (frozen).  The detector's three (``pfa``, ``guard``, ``train``: see ``check_cfar``); the
    peak rule's separations ``sep_range`` and ``sep_azimuth`` (a point dominates the cells that close around it; 4 azimuth cells are
    half the 8-antenna main lobe); the association's ``range_gate`` (range bins) and ``doppler_gate`` (Doppler bins); ``max_points``
    rows per frame.  All eight defaults are guesses: nobody has run this on a real capture."""
    __slots__ = ("pfa", "guard", "train", "sep_range", "sep_azimuth", "range_gate", "doppler_gate", "max_points")

    def __init__(self, pfa=CFAR_DEFAULTS["pfa"], guard=CFAR_DEFAULTS["guard"], train=CFAR_DEFAULTS["train"],
                 sep_range=POINT_DEFAULTS["sep_range"], sep_azimuth=POINT_DEFAULTS["sep_azimuth"], range_gate=POINT_DEFAULTS["range_gate"],
                 doppler_gate=POINT_DEFAULTS["doppler_gate"], max_points=POINT_DEFAULTS["max_points"]):
        pfa, guard, train = check_cfar(pfa, guard, train)
        vals = dict(pfa=pfa, guard=guard, train=train)
        vals.update(check_points(sep_range=sep_range, sep_azimuth=sep_azimuth, range_gate=range_gate, doppler_gate=doppler_gate,
                                 max_points=max_points))
        for k in self.__slots__:
            object.__setattr__(self, k, vals[k])

    def __setattr__(self, name, value):
        raise AttributeError("PointCloudSettings is frozen")

    def __delattr__(self, name):
        raise AttributeError("PointCloudSettings is frozen")

    def __eq__(self, other):
        return isinstance(other, PointCloudSettings) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, k) for k in self.__slots__))

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__))


def radar_geometry(model):
    """A ``simulate.RadarModel`` -> the tuple the fuse entry takes: (range_bin_m, doppler_mps_per_bin, a_h, o_h, a_v, o_v), with
    ``doppler_mps_per_bin = wavelength / (64 * 6 * chirp_period_s)`` (the inverse of ``RadarModel.expected_cell``'s formula), a_s the
    sensor's array axis (``rotation[:, 0]``) and o_s its origin, fp64 3-vectors."""
    _, _, rot_h, org_h = model.sensors["hori"]
    _, _, rot_v, org_v = model.sensors["vert"]
    return (float(model.range_bin_m), float(model.wavelength) / (64.0 * 6.0 * float(model.chirp_period_s)),
            np.array(rot_h[:, 0], dtype=np.float64), np.array(org_h, dtype=np.float64),
            np.array(rot_v[:, 0], dtype=np.float64), np.array(org_v, dtype=np.float64))


def geometry_vector(geometry):
    """The tuple of ``radar_geometry`` -> the 14 fp64 values the library reads; ValueError for another layout.  The values themselves
    (unit and orthogonal axes, positive scalars) are the library's to refuse."""
    try:
        rb, dv, a_h, o_h, a_v, o_v = geometry
        vec = np.concatenate([[float(rb), float(dv)]] + [np.asarray(v, dtype=np.float64).reshape(-1) for v in (a_h, o_h, a_v, o_v)])
    except (TypeError, ValueError):
        raise ValueError("geometry must be (range_bin_m, doppler_mps_per_bin, a_h, o_h, a_v, o_v), as radar_geometry returns it") from None
    if vec.shape != (14,):
        raise ValueError("geometry: the four vectors must have three components each")
    return np.ascontiguousarray(vec)


def radar_point_cloud(adc_hori, adc_vert, model=None, settings=None, tdm_compensation=False, interference=None):
    """Both sensors' int16 ADC cubes (n, 4, 192, 256, 2) on the GPU -> ``functional.RadarCloud``: per frame up to
    ``settings.max_points`` rows (x, y, z, radial velocity, snr_h, snr_v, row_h, row_v), with the two sensors' ``RadarPeaks`` as
    ``peaks_h`` and ``peaks_v``.  Per sensor ``fft_chain_loader_means`` (``tdm_compensation`` / ``interference`` as there), ``cfar_ra``
    (mask and SNR) and ``radar_peaks``, then one ``radar_points_fuse``.  ``model``: a ``simulate.RadarModel`` (None: its defaults);
    ``settings``: a ``PointCloudSettings`` (None: its defaults).  The model's chirp constants are the simulator's GUESSES (the reference
    carries no chirp configuration), so on a real capture the metres and metres per second are guesses too.  Device tensors, no sync."""
    from .. import functional as F_
    from ..simulate import RadarModel
    from .process_iwr1843 import fft_chain_loader_means
    settings = PointCloudSettings() if settings is None else settings
    if not isinstance(settings, PointCloudSettings):
        raise ValueError("settings must be a PointCloudSettings or None, got %s" % type(settings).__name__)
    model = RadarModel() if model is None else model
    if not isinstance(model, RadarModel):
        raise ValueError("model must be a simulate.RadarModel or None, got %s" % type(model).__name__)
    for name, t in (("adc_hori", adc_hori), ("adc_vert", adc_vert)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int16 or t.dim() != 5 or tuple(t.shape[1:]) != (4, 192, 256, 2):
            raise ValueError("%s must be int16 (n, 4, 192, 256, 2), got %s %r" % (name, getattr(t, "dtype", type(t).__name__),
                                                                                tuple(getattr(t, "shape", ()))))
    if adc_hori.shape[0] != adc_vert.shape[0]:
        raise ValueError("the sensors' frame counts differ: %d and %d" % (adc_hori.shape[0], adc_vert.shape[0]))
    if not adc_hori.is_cuda or not adc_vert.is_cuda:
        raise F_.rt.HuprError("radar_point_cloud needs GPU cubes (no CPU fallback), got %s and %s" % (adc_hori.device, adc_vert.device))
    peaks = []
    for adc in (adc_hori, adc_vert):
        planes = fft_chain_loader_means(adc, tdm_compensation=tdm_compensation, interference=interference)
        det = F_.cfar_ra(planes, settings.pfa, settings.guard, settings.train, want_mask=True, want_snr=True)
        peaks.append(F_.radar_peaks(planes, det.mask, det.snr, settings.max_points, settings.sep_range, settings.sep_azimuth))
    return F_.radar_points_fuse(peaks[0], peaks[1], radar_geometry(model), settings.range_gate, settings.doppler_gate)
