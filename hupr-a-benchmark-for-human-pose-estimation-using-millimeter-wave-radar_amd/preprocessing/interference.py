"""Interference blanking of the raw ADC cube in front of the FFT chain (csrc/interference.hip; the rule is stated in section (a15) of
include/hupr.h).  Two FMCW radars that share a band — every HuPR capture runs two IWR1843 at once — put short high-amplitude bursts
into each other's chirps wherever their ramps cross inside the IF bandwidth; the range transform smears one burst over all 64 range
bins and ``Normalize`` then scales the frame by a standard deviation the burst has inflated.  The filter finds the bursts on the
clutter-removed residual of every (sensor-frame, rx, tx) group, against each chirp's own median power, and puts the group's clutter
estimate (or zero) in their place.  A cube without a flagged sample passes through bit for bit.

Off by default everywhere.  ``threshold`` (the power ratio K), ``guard`` and ``fill`` default to guesses: nobody has measured whether
the published HuPR captures contain interference, what the filter does to AP and MPJPE, or which values are good.

It commutes with the left/right mirror (``tools.augment.adc_mirror``), which permutes whole groups; where both run, the filter runs
first.
"""
import numpy as np

FILLS = {"clutter": 0, "zero": 1}                  # include/hupr.h HUPR_INTERFERENCE_FILL_*
INTERFERENCE_DEFAULTS = {"K": 32, "guard": 2, "fill": "clutter"}
K_RANGE, GUARD_RANGE = (2, 1024), (0, 8)

INTERFERENCE_NEEDS_ADC = ("DATASET.interference is set, but this dataset reads stored cubes: the filter works on the raw ADC samples in "
                          "front of the FFT chain, which a stored cube no longer has.  Cubes written with "
                          "processRadarDataHoriVert(interference=...) are already filtered and are used with the key off")


def check_interference(K, guard, fill):
    """The filter's three settings -> (int K, int guard, str fill); ValueError for a ``K`` outside [2, 1024], a ``guard`` outside
    [0, 8], a ``fill`` that is neither "clutter" nor "zero", or a value of the wrong kind."""
    for name, v, (lo, hi) in (("K", K, K_RANGE), ("guard", guard, GUARD_RANGE)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("%s must be an integer in [%d, %d], got %r" % (name, lo, hi, v))
    if not isinstance(fill, str) or fill not in FILLS:
        raise ValueError("fill must be 'clutter' or 'zero', got %r" % (fill,))
    return int(K), int(guard), fill


class InterferenceFilter:
    """The filter's settings (frozen): ``K`` the power ratio of the threshold over the chirp's median residual power, an integer in
    [2, 1024]; ``guard`` the samples flagged on each side of a flagged one, in [0, 8]; ``fill`` what replaces a flagged sample,
    "clutter" (the group's mean over the loops not flagged there, rounded half up) or "zero".  The three defaults are guesses."""
    __slots__ = ("K", "guard", "fill")

    def __init__(self, K=INTERFERENCE_DEFAULTS["K"], guard=INTERFERENCE_DEFAULTS["guard"], fill=INTERFERENCE_DEFAULTS["fill"]):
        for k, v in zip(self.__slots__, check_interference(K, guard, fill)):
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError("InterferenceFilter is frozen")

    def __delattr__(self, name):
        raise AttributeError("InterferenceFilter is frozen")

    def __eq__(self, other):
        return isinstance(other, InterferenceFilter) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, k) for k in self.__slots__))

    def __repr__(self):
        return "InterferenceFilter(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)

    def sidecar(self):
        """What ``preprocess.json`` records under ``"adc_interference"``."""
        return {"threshold": self.K, "guard": self.guard, "fill": self.fill}


def check_filter(interference):
    """An ``interference=`` argument: None or an InterferenceFilter."""
    if interference is not None and not isinstance(interference, InterferenceFilter):
        raise ValueError("interference must be an InterferenceFilter or None, got %r" % (interference,))
    return interference


_KEYS = {"threshold": "K", "guard": "guard", "fill": "fill"}


def interference_setting(cfg):
    """``DATASET.interference`` (no key of the reference's YAML) -> None with the key absent or ``false``, ``InterferenceFilter()`` with
    ``true``, an InterferenceFilter of the given values with a mapping of any of ``threshold``, ``guard``, ``fill``.  Anything else
    raises here, where the config is read."""
    v = getattr(getattr(cfg, "DATASET", None), "interference", None)
    if v is None or v is False:
        return None
    if v is True:
        return InterferenceFilter()
    if not isinstance(v, dict):                         # config_tree.obj: a YAML mapping as attributes
        if not hasattr(v, "__dict__") or isinstance(v, type):
            raise ValueError("DATASET.interference must be true, false or a mapping of threshold / guard / fill, got %r" % (v,))
        v = vars(v)
    for k in v:
        if k not in _KEYS:
            raise ValueError("DATASET.interference.%s is no setting of the filter (%s)" % (k, ", ".join(_KEYS)))
    try:
        return InterferenceFilter(**{_KEYS[k]: x for k, x in v.items()})
    except ValueError as e:
        raise ValueError("DATASET.interference: %s" % e) from None


def interference_mismatch_warning(side, now):
    """-> the warning line when the weights beside sidecar dict ``side`` were trained under another ``DATASET.interference`` setting
    than ``now`` (None or an InterferenceFilter) that this process runs, else None.  A sidecar without the key means off."""
    trained = side.get("adc_interference")
    running = now.sidecar() if now is not None else None
    if trained == running:
        return None
    return ("==========>WARNING: these weights were trained with DATASET.interference %s, this process runs it %s"
            % (trained if trained is not None else "off", running if running is not None else "off"))


def adc_interference(adc, interference=None, out=None, want_mask=False):
    """int16 GPU cubes (n, 4, 192, 256, 2) through the filter ``interference`` (an InterferenceFilter; None = the defaults) ->
    ``(cube, stats, mask)`` as ``functional.adc_interference`` returns them."""
    from .. import functional as F_
    f = check_filter(interference) or InterferenceFilter()
    return F_.adc_interference(adc, f.K, f.guard, f.fill, out=out, want_mask=want_mask)


def filtered(adc, interference):
    """The cube the FFT chain reads: ``adc`` itself with ``interference`` None, else a new filtered tensor (the caller's cube is left
    as it is)."""
    if check_filter(interference) is None:
        return adc
    return adc_interference(adc, interference)[0]
