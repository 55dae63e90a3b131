"""The fp64 statement of the radar scene simulator (include/hupr.h section (a16), csrc/radar_scene.hip), for the tests.  Written here:
the reference project has no simulator.  It states the kernel's RULE, not only the physics: geometry and the two phase fractions in
fp64, operation by operation as the header orders them, each rounded to a 32-bit fraction of a turn, and the phase of sample n as
phi0 + n * dphi in wrapping uint32 arithmetic.  From there on it is exact where the kernel is fp32: the sine, the cosine and the sum
over scatterers are fp64."""
import numpy as np

NUM_RX, NUM_CHIRP, NUM_SAMPLE = 4, 192, 256
_M32 = np.uint64(0xFFFFFFFF)


def _turn_u32(turns):
    f = turns - np.floor(turns)
    return (np.rint(f * 4294967296.0).astype(np.uint64) & _M32).astype(np.uint32)


def _dist(p, q):
    d = p - q
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def scene_terms(pos, vel, amp, tx, rx, wavelength, range_bin_m, chirp_period_s):
    """pos, vel (frames, S, 3), amp (frames, S) -> per (frame, receiver, chirp, scatterer): phi0, dphi uint32 and the received
    amplitude a / (|p - tx| |p - rx|) as fp64 (0 where the scatterer is hidden)."""
    pos, vel = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    amp = np.asarray(amp, dtype=np.float32)
    tx, rx = np.asarray(tx, dtype=np.float64), np.asarray(rx, dtype=np.float64)
    c = np.arange(NUM_CHIRP)
    t = c.astype(np.float64) * np.float64(chirp_period_s)
    with np.errstate(all="ignore"):
        p = pos[:, None, :, :] + vel[:, None, :, :] * t[None, :, None, None]                  # (F, 192, S, 3)
        dt = _dist(p, tx[c % 3][None, :, None, :])                                            # (F, 192, S)
        dr = _dist(p[:, None], rx[None, :, None, None, :])                                    # (F, 4, 192, S)
        dt = np.broadcast_to(dt[:, None], dr.shape)
        a = np.broadcast_to(amp[:, None, None, :], dr.shape)
        live = (a > 0) & np.isfinite(a) & np.isfinite(dt) & np.isfinite(dr) & (dt != 0) & (dr != 0)
        path = np.where(live, dt + dr, 1.0)
        phi0 = _turn_u32(path / np.float64(wavelength))
        dphi = _turn_u32(path / (512.0 * np.float64(range_bin_m)))
        A = np.where(live, a.astype(np.float64) / np.where(live, dt * dr, 1.0), 0.0)
    return np.where(live, phi0, 0).astype(np.uint32), np.where(live, dphi, 0).astype(np.uint32), A


def radar_scene_ref(pos, vel, amp, tx, rx, wavelength, range_bin_m, chirp_period_s, add=None, physics=False):
    """-> (cube complex128 (frames, 4, 192, 256), A (frames, 4, 192): the row's sum of received amplitudes).  ``physics``: the model
    without the 32-bit phase rounding (fp64 phases throughout), for the tests that are about the geometry."""
    pos, vel = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    F, S = pos.shape[:2]
    n = np.arange(NUM_SAMPLE)
    out = np.zeros((F, NUM_RX, NUM_CHIRP, NUM_SAMPLE), dtype=np.complex128)
    if physics:
        tx_, rx_ = np.asarray(tx, dtype=np.float64), np.asarray(rx, dtype=np.float64)
        c = np.arange(NUM_CHIRP)
        t = c * float(chirp_period_s)
        p = pos[:, None, :, :] + vel[:, None, :, :] * t[None, :, None, None]
        dt = _dist(p, tx_[c % 3][None, :, None, :])[:, None]
        dr = _dist(p[:, None], rx_[None, :, None, None, :])
        path = dt + dr
        A = np.asarray(amp, dtype=np.float64)[:, None, None, :] / (dt * dr)
        for s in range(S):
            ph = path[..., s, None] / wavelength + n * path[..., s, None] / (512.0 * range_bin_m)
            out += A[..., s, None] * np.exp(2j * np.pi * ph)
        return out, A.sum(axis=-1)
    phi0, dphi, A = scene_terms(pos, vel, amp, tx, rx, wavelength, range_bin_m, chirp_period_s)
    n64 = n.astype(np.uint64)
    for s in range(S):
        ph = ((phi0[..., s, None].astype(np.uint64) + n64 * dphi[..., s, None].astype(np.uint64)) & _M32).astype(np.uint32)
        x = ph.view(np.int32).astype(np.float64) * (2.0 * np.pi / 4294967296.0)
        out += A[..., s, None] * (np.cos(x) + 1j * np.sin(x))
    if add is not None:
        add = np.asarray(add, dtype=np.float64)
        out += add[..., 0] + 1j * add[..., 1]
    return out, A.sum(axis=-1)


def quantise(z):
    """complex (...) -> int16 (..., 2): rint (ties to even), clipped."""
    return np.stack([np.clip(np.rint(z.real), -32768, 32767), np.clip(np.rint(z.imag), -32768, 32767)], axis=-1).astype(np.int16)
