"""Host-side mirror of the reference's preprocessing operator.

``RadarObject().generateHeatmap(frame)`` keeps the reference contract
(preprocessing/process_iwr1843.py:106,173): ``frame`` complex ndarray (4,192,256) ->
complex ndarray (16,64,64,8); the arithmetic runs in the gfx950 FFT-chain kernels
(csrc/fft_chain.hip) in complex64 and is widened to complex128 on return.

The batched device entry points (`fft_chain`, `fft_chain_loader`) are what the training
loader uses: int16 I/Q cubes resident in HBM in, complex64 cubes or normalised fp32 network
input out.
"""
import os

import numpy as np
import torch

from .. import runtime as rt
from .interference import filtered as _interference_filtered

NUM_RX, NUM_CHIRP, NUM_SAMPLE = 4, 192, 256


def _workspace(n_sf, device):
    nbytes = rt.lib().hupr_fft_chain_ws_bytes(n_sf)
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device), nbytes


def _check_adc(adc_iq):
    if adc_iq.dtype != torch.int16 or tuple(adc_iq.shape[1:]) != (NUM_RX, NUM_CHIRP, NUM_SAMPLE, 2):
        raise ValueError("adc_iq must be int16 (n,4,192,256,2), got %s %r" % (adc_iq.dtype, tuple(adc_iq.shape)))


HANN_RANGE, HANN_DOPPLER, MAGNITUDE, ZERO_DOPPLER_EXACT, RANGE_FIRST = 1, 2, 4, 8, 16      # include/hupr.h HUPR_FFT_*

# What the zero-Doppler bin (Doppler index 8, loader slot f = 4) holds — include/hupr.h, "The zero-Doppler bin":
#   "dither"      (default) a frame-keyed stand-in for the reference's fp64 rounding residue, normalised like every other bin,
#                 so an unmodified reference Normalize / a reference-trained checkpoint sees what it was trained on;
#   "exact"       exactly zero (round 3's chain; the loader emits zeros in slot f = 4);
#   "range_first" the rounds-1/2 kernel order, whose own fp32 rounding residue fills the bin (slower).
# Under a window: "dither" and "exact" hold as stated with window=None and window="range" (the same unwindowed dither; exact zeros). With
# the Doppler window ("doppler", "hann") the bin is ordinary leakage, computed like every other bin; the two conventions are accepted and
# change nothing.
# HUPR_FFT_ZERO_DOPPLER selects the process default; tools.Runner records the mode in `preprocess.json` next to its checkpoints and
# warns when weights trained under one convention are loaded under another.
ZERO_DOPPLER_MODES = {"dither": 0, "exact": ZERO_DOPPLER_EXACT, "range_first": RANGE_FIRST}
ZERO_DOPPLER = os.environ.get("HUPR_FFT_ZERO_DOPPLER", "dither")
if ZERO_DOPPLER not in ZERO_DOPPLER_MODES:
    raise ValueError("HUPR_FFT_ZERO_DOPPLER must be one of %s, got %r" % (sorted(ZERO_DOPPLER_MODES), ZERO_DOPPLER))


def _flags(window, magnitude, zero_doppler=None):
    """window: None / False (the reference: rectangular), "hann" / True (range + Doppler), "range", "doppler";
    zero_doppler: None (the process default ZERO_DOPPLER) or a key of ZERO_DOPPLER_MODES."""
    table = {None: 0, False: 0, "none": 0, True: 3, "hann": 3, "range": 1, "doppler": 2}
    if window not in table:
        raise ValueError("window must be one of None, 'hann', 'range', 'doppler'; got %r" % (window,))
    zd = ZERO_DOPPLER if zero_doppler is None else zero_doppler
    if zd not in ZERO_DOPPLER_MODES:
        raise ValueError("zero_doppler must be one of %s, got %r" % (sorted(ZERO_DOPPLER_MODES), zd))
    return table[window] | (MAGNITUDE if magnitude else 0) | ZERO_DOPPLER_MODES[zd]


# Doppler phase compensation for the TDM-MIMO virtual array (include/hupr.h, hupr_fft_chain_tdm).  Slot of the transmitter behind
# virtual antenna v in the chain's workspace order: TX0 fires first (v = 0..3), TX1 — the elevated row, v = 8..11 — second, TX2
# (v = 4..7) third; the ADC mirror of tools/augment.py exchanges TX0 and TX2 and with them their slots ("swapped").
TDM_SLOTS = (0, 0, 0, 0, 2, 2, 2, 2, 1, 1, 1, 1)
TDM_SLOTS_SWAPPED = (2, 2, 2, 2, 0, 0, 0, 0, 1, 1, 1, 1)


def tdm_phase_table(swapped=False):
    """The compensation factors ``exp(-2 pi j d k(v) / 192)`` as a complex128 ``(12 virtual antennas, 16 kept Doppler indices)``
    array in fp64: ``d = i - 8`` the signed Doppler bin, ``k(v)`` the slot of the antenna's transmitter (``TDM_SLOTS``, or
    ``TDM_SLOTS_SWAPPED`` for a mirrored sensor-frame).  A factor with ``d == 0`` or ``k == 0`` is exactly 1.  The device multiplies by
    the fp32 roundings of these cosines and sines (csrc/fft_chain.hip, ``kTdmFactor``).  A Doppler bin aliased past +-32 gets the
    wrong sign, as in every TDM-MIMO pipeline: the compensation knows the bin, not the velocity."""
    k = np.asarray(TDM_SLOTS_SWAPPED if swapped else TDM_SLOTS, dtype=np.int64)[:, None]
    d = np.arange(16, dtype=np.int64)[None, :] - 8
    ang = 2.0 * np.pi * (d * k).astype(np.float64) / 192.0
    return np.cos(ang) - 1j * np.sin(ang)


def _tdm_table(tx_swapped, frames_per_flag, n):
    """-> (pointer or None, n_swapped, frames_per_flag) of hupr_fft_chain_tdm for ``n`` sensor-frames."""
    if not isinstance(frames_per_flag, int) or isinstance(frames_per_flag, bool) or frames_per_flag < 1:
        raise ValueError("frames_per_flag must be a positive int, got %r" % (frames_per_flag,))
    if tx_swapped is None:
        return None, 0, frames_per_flag
    if tx_swapped.dtype != torch.uint8 or tx_swapped.dim() != 1 or tx_swapped.numel() * frames_per_flag < n or tx_swapped.numel() == 0:
        raise ValueError("tx_swapped must be a uint8 (ceil(n / frames_per_flag),) device tensor, got %s %r for %d frames, %d per flag"
                         % (tx_swapped.dtype, tuple(tx_swapped.shape), n, frames_per_flag))
    return rt.ptr(tx_swapped), tx_swapped.numel(), frames_per_flag


def _refuse_swap_without_tdm(tdm_compensation, tx_swapped):
    if tx_swapped is not None and not tdm_compensation:
        raise ValueError("tx_swapped only means something with tdm_compensation=True")


_PLAIN_ENTRIES = ("hupr_fft_chain_c64", "hupr_fft_chain_loader_f32", "hupr_fft_chain_loader_means_f32")       # by loader code


def _chain(adc_iq, loader, shape, dtype, flags, ws, out, tdm_compensation, tx_swapped, frames_per_flag, interference):
    """The launch behind the three public functions.  ``loader``: 0 the complex cube, 1 the loader tensor, 2 its elevation means;
    ``shape`` and ``dtype``: the output behind the sensor-frame axis, for a new tensor or to hold a given ``out`` to before any launch
    (functional._outputs).  With TDM compensation the entry is hupr_fft_chain_tdm, with ``flags == 0`` the plain one of ``loader``,
    otherwise hupr_fft_chain_opts."""
    from ..functional import _outputs
    _check_adc(adc_iq)
    _refuse_swap_without_tdm(tdm_compensation, tx_swapped)
    n, dev = adc_iq.shape[0], adc_iq.device
    out, = _outputs("fft_chain", None if out is None else (out,), (n,), dev, ((shape, dtype),))
    adc_iq = _interference_filtered(adc_iq, interference)
    if ws is None:
        ws = _workspace(n, dev)[0]
    table = _tdm_table(tx_swapped, frames_per_flag, n) if tdm_compensation else None
    head = (rt.ptr(adc_iq), n, rt.ptr(out))
    tail = (rt.ptr(ws), ws.numel() * ws.element_size(), rt.stream())        # the library asks only that the buffer is large enough
    L = rt.lib()
    if tdm_compensation:
        rt.check(L.hupr_fft_chain_tdm(*head, flags, loader, *table, *tail))
    elif flags == 0:
        rt.check(getattr(L, _PLAIN_ENTRIES[loader])(*head, *tail))
    else:
        rt.check(L.hupr_fft_chain_opts(*head, flags, loader, *tail))
    return out


def fft_chain(adc_iq, ws=None, window=None, magnitude=False, zero_doppler=None, tdm_compensation=False, tx_swapped=None,
              frames_per_flag=1, interference=None):
    """adc_iq: int16 GPU tensor (n,4,192,256,2) -> complex64 GPU tensor (n,16,64,64,8).
    Opt-in (defaults = the reference: no window, complex output): ``window="hann"`` applies np.hanning windows over the
    range samples and the chirp loops, ``magnitude=True`` returns |X| as fp32.  ``zero_doppler``: see ZERO_DOPPLER_MODES.
    ``tdm_compensation=True`` multiplies the range-Doppler map by ``tdm_phase_table`` in front of the angle transform
    (hupr_fft_chain_tdm); ``tx_swapped``: uint8 device tensor, one flag per ``frames_per_flag`` sensor-frames, non-zero = that
    group's transmitters 0 and 2 were exchanged (``tools.augment.adc_mirror``); None = none.  Reference-trained weights expect the
    default, off.  ``interference``: an ``InterferenceFilter`` runs the interference blanking of preprocessing/interference.py on the
    cube first (two more launches, into a new buffer: ``adc_iq`` is left as it is); None, the default, is today's launches."""
    return _chain(adc_iq, 0, (16, 64, 64, 8), torch.float32 if magnitude else torch.complex64, _flags(window, magnitude, zero_doppler), ws,
                  None, tdm_compensation, tx_swapped, frames_per_flag, interference)


def fft_chain_loader(adc_iq, ws=None, out=None, window=None, zero_doppler=None, tdm_compensation=False, tx_swapped=None,
                     frames_per_flag=1, interference=None):
    """adc_iq: int16 GPU tensor (n,4,192,256,2) -> fp32 GPU tensor (n, 8, 2, 64, 64, 8):
    Doppler bins 4..11, re/im split, per-elevation Normalize (datasets glue fused in).  ``window`` / ``zero_doppler`` /
    ``tdm_compensation`` / ``tx_swapped`` / ``frames_per_flag`` / ``interference``: see fft_chain (the statistics are those of the
    compensated values).  ``out``: a tensor of that shape to write."""
    return _chain(adc_iq, 1, (8, 2, 64, 64, 8), torch.float32, _flags(window, False, zero_doppler), ws, out, tdm_compensation,
                  tx_swapped, frames_per_flag, interference)


def fft_chain_loader_means(adc_iq, ws=None, zero_doppler=None, tdm_compensation=False, tx_swapped=None, frames_per_flag=1,
                           interference=None, out=None):
    """adc_iq: int16 GPU tensor (n,4,192,256,2) -> fp32 GPU tensor (n, 16, 64, 64): the loader tensor of ``fft_chain_loader``
    averaged over its elevation axis, plane index 2 f + c — what ``HuPRNet.forward`` computes first (models/networks.py:26-27).
    The fused training loader hands these planes to the model instead of the 8x larger (n,8,2,64,64,8) tensor.
    ``tdm_compensation`` / ``tx_swapped`` / ``frames_per_flag`` / ``interference``: see fft_chain; ``out``: see fft_chain_loader."""
    return _chain(adc_iq, 2, (16, 64, 64), torch.float32, _flags(None, False, zero_doppler), ws, out, tdm_compensation, tx_swapped,
                  frames_per_flag, interference)


def loader_normalize(cube):
    """cube: complex64 GPU tensor (n,16,64,64,8) -> fp32 (n,8,2,64,64,8) (dataset.py:144-150)."""
    if cube.dtype != torch.complex64 or tuple(cube.shape[1:]) != (16, 64, 64, 8):
        raise ValueError("cube must be complex64 (n,16,64,64,8)")
    n = cube.shape[0]
    out = torch.empty((n, 8, 2, 64, 64, 8), dtype=torch.float32, device=cube.device)
    rt.check(rt.lib().hupr_loader_normalize_c64(rt.ptr(cube), n, rt.ptr(out), rt.stream()))
    return out


def dca1000_frames(raw):
    """raw: int16 GPU tensor (whole adc_data.bin stream) -> int16 GPU tensor (n_frames,4,192,256,2), the FFT-chain
    input layout (reference getadcDataFromDCA1000 :54-83 + the per-frame slicing of :190-191)."""
    if raw.dtype != torch.int16 or raw.dim() != 1:
        raise ValueError("raw must be a flat int16 tensor")
    per_frame = NUM_RX * NUM_CHIRP * NUM_SAMPLE * 2
    n_frames = raw.numel() // per_frame
    out = torch.empty((n_frames, NUM_RX, NUM_CHIRP, NUM_SAMPLE, 2), dtype=torch.int16, device=raw.device)
    rt.check(rt.lib().hupr_dca1000_deinterleave(rt.ptr(raw), rt.ptr(out), n_frames, rt.stream()))
    return out


class RadarObject:
    """Same constants and operator surface as the reference class (process_iwr1843.py:8-34).  ``numGroup`` / ``root`` /
    ``saveRoot`` / ``rawRoot`` parametrise the directory lists the reference hard-codes in ``initialize`` (:36-46); the
    defaults reproduce its paths."""

    def __init__(self, device="cuda", numGroup=276, root="HuPR", saveRoot="HuPR", rawRoot="raw_data/iwr1843", dataRoot="../data"):
        self.root, self.saveRoot, self.sensorType = root, saveRoot, "iwr1843"
        self.radarDataFileNameGroup = [[os.path.join(rawRoot, root, "single_%d" % i, "hori"), os.path.join(rawRoot, root, "single_%d" % i, "vert")]
                                       for i in range(1, numGroup + 1)]
        self.saveDirNameGroup = [os.path.join(dataRoot, saveRoot, "single_%d" % i) for i in range(1, numGroup + 1)]
        self.numADCSamples = 256
        self.adcRatio = 4
        self.numAngleBins = self.numADCSamples // self.adcRatio
        self.numEleBins = 8
        self.numRX = 4
        self.numLanes = 2
        self.framePerSecond = 10
        self.duration = 60
        self.numFrame = self.framePerSecond * self.duration
        self.numChirp = 64 * 3
        self.idxProcChirp = 64
        self.numGroupChirp = 4
        self.numKeypoints = 14
        self.device = device

    def getadcDataFromDCA1000(self, fileName):
        """<fileName>/adc_data.bin -> complex128 ndarray (4, n_chirps, 256), like the reference; the de-interleave
        runs on the GPU.  Use ``dca1000_frames`` directly to keep the cube on the device for ``fft_chain``."""
        raw = np.fromfile(os.path.join(fileName, "adc_data.bin"), dtype=np.int16)
        fr = dca1000_frames(torch.from_numpy(raw).to(self.device)).cpu().numpy()      # (F,4,192,256,2)
        z = fr[..., 0].astype(np.float64) + 1j * fr[..., 1].astype(np.float64)
        return np.ascontiguousarray(z.transpose(1, 0, 2, 3).reshape(self.numRX, -1, self.numADCSamples))

    def saveRadarData(self, matrix, dirName, idxFrame):
        """``<dirName>/<idxFrame:09d>.npy`` (reference :180-182)."""
        np.save(os.path.join(dirName, "%09d.npy" % idxFrame), matrix)

    def processRadarDataHoriVert(self, frames_per_call=64, tdm_compensation=False, interference=None):
        """The reference's offline driver (:184-196): every sequence's two captures -> one complex128 ``(16,64,64,8)`` cube per
        frame and sensor under ``<saveDir>/{hori,vert}/%09d.npy``.  Here a capture goes to the GPU once, is de-interleaved there
        and transformed ``frames_per_call`` frames at a time (the reference parses 115 200 chirps and runs ~200 000 tiny FFT calls
        per frame in Python).  Training does not need these files: ``datasets.HuPRRawADC`` feeds the network straight from
        the captures.  ``tdm_compensation=True`` writes Doppler-compensated cubes (see ``fft_chain``); a dataset that reads them runs with
        ``DATASET.tdmCompensation`` off, since the cubes already are.  ``interference``: an ``InterferenceFilter`` blanks interference in the
        raw cubes first (see ``fft_chain``); a dataset that reads such cubes runs with ``DATASET.interference`` off."""
        for names, save_dir in zip(self.radarDataFileNameGroup, self.saveDirNameGroup):
            for sensor, name in zip(("hori", "vert"), names):
                out_dir = os.path.join(save_dir, sensor)
                os.makedirs(out_dir, exist_ok=True)
                raw = np.fromfile(os.path.join(name, "adc_data.bin"), dtype=np.int16)
                frames = dca1000_frames(torch.from_numpy(raw).to(self.device))
                n = min(frames.shape[0], self.numFrame)
                for f0 in range(0, n, frames_per_call):
                    cubes = fft_chain(frames[f0:min(n, f0 + frames_per_call)], tdm_compensation=tdm_compensation,
                                      interference=interference).cpu().numpy().astype(np.complex128)
                    for k, cube in enumerate(cubes):
                        self.saveRadarData(cube, out_dir, f0 + k)
                print("%s, finished %d frames" % (name, n))

    def generateHeatmap(self, frame, window=None, magnitude=False, tdm_compensation=False, interference=None):
        """frame: complex ndarray (4,192,256) -> complex128 ndarray (16,64,64,8) (float64 with ``magnitude``).
        ``window`` / ``magnitude`` / ``tdm_compensation`` / ``interference`` are opt-in extras (see ``fft_chain``); the defaults are the reference's
        arithmetic."""
        frame = np.asarray(frame)
        if frame.shape != (self.numRX, self.numChirp, self.numADCSamples):
            raise ValueError("frame must be (4,192,256), got %r" % (frame.shape,))
        iq = np.stack([frame.real, frame.imag], axis=-1)
        if not np.all(np.abs(iq) <= 32767) or not np.array_equal(iq, np.rint(iq)):
            raise ValueError("generateHeatmap expects integer-valued 16-bit ADC samples")
        dev = torch.from_numpy(iq.astype(np.int16)[None]).to(self.device)
        out = fft_chain(dev, window=window, magnitude=magnitude, tdm_compensation=tdm_compensation, interference=interference)
        return out[0].cpu().numpy().astype(np.float64 if magnitude else np.complex128)
