"""Radar scene simulator: a walking stick figure of point scatterers, seen by both IWR1843 arrays, as raw DCA1000 captures.

NOT real data.  Scatterers are isotropic points of fixed amplitude; there is no multipath, no occlusion, no clothing, no antenna
pattern, and the body is a stick figure.  Whatever a network learns from these recordings says nothing about AP on HuPR.  What they
are for: a physically coherent multi-frame input, in metres and metres per second, on which the whole chain (``adc_data.bin`` ->
``HuPRRawADC`` -> FFT chain -> CFAR -> ``PoseStream`` -> ``Runner``) runs unchanged.

The signal model is stated beside ``hupr_radar_scene_i16`` in include/hupr.h and computed by csrc/radar_scene.hip
(``functional.radar_scene``): one launch per sensor and block of frames, no CPU fallback.  Coordinates: x to the right of the radar,
y along its boresight, z up; the horizontal sensor's first transmitter is the origin.

The chirp parameters below are GUESSES: the reference carries no chirp configuration.  They were chosen so that a person 1.2 to 3.5 m
away falls into the range bins the chain keeps (31 to 94)."""
import json
import os

import numpy as np

from . import synth

DEFAULT_WAVELENGTH = 3.9e-3            # metres (77 GHz); a guess, as the three below
DEFAULT_RANGE_BIN_M = 0.0375           # metres per bin of the 256-point range transform
DEFAULT_CHIRP_PERIOD_S = 1e-4          # seconds between two chirps (any transmitter)
DEFAULT_FRAME_RATE_HZ = 10.0
DEFAULT_VERT_ORIGIN = (0.0, 0.0, -0.10)    # the vertical sensor sits below the horizontal one; a guess

QUARTER_TURN = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])      # about the boresight y: x -> z, z -> -x


def iwr1843_array(wavelength, rotation=None, origin=(0.0, 0.0, 0.0)):
    """The antenna positions of one IWR1843, metres -> (tx (3, 3), rx (4, 3)) fp64.  In the array's own frame, with h = wavelength / 2:
    rx[k] = -k h x, tx[0] = 0, tx[2] = -4 h x, tx[1] = -2 h x - h z.  These signs make the far field of the model the scene of
    ``synth.point_target_scene(tdm=True)`` (tests/test_radar_scene_cpu.py; with the elevated transmitter at +z the agreement is lost).
    ``rotation``: a 3 x 3 matrix applied to those positions (None: identity; ``QUARTER_TURN`` for the vertical sensor), then
    ``origin`` is added."""
    h = 0.5 * float(wavelength)
    if not (np.isfinite(h) and h > 0):
        raise ValueError("iwr1843_array: wavelength must be positive and finite, got %r" % (wavelength,))
    tx = np.array([[0.0, 0.0, 0.0], [-2.0 * h, 0.0, -h], [-4.0 * h, 0.0, 0.0]])
    rx = np.array([[-k * h, 0.0, 0.0] for k in range(4)])
    R = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64)
    o = np.asarray(origin, dtype=np.float64)
    if R.shape != (3, 3) or o.shape != (3,):
        raise ValueError("iwr1843_array: rotation must be 3 x 3 and origin a 3-vector")
    return tx @ R.T + o, rx @ R.T + o


class RadarModel:
    """The three chirp scalars, both sensors' arrays and the frame rate.  ``sensors`` = {"hori": (tx, rx, rotation, origin), "vert":
    ...}.  The defaults are guesses (see the module docstring)."""

    def __init__(self, wavelength=DEFAULT_WAVELENGTH, range_bin_m=DEFAULT_RANGE_BIN_M, chirp_period_s=DEFAULT_CHIRP_PERIOD_S,
                 frame_rate_hz=DEFAULT_FRAME_RATE_HZ, vert_origin=DEFAULT_VERT_ORIGIN, vert_rotation=QUARTER_TURN):
        for k, v in (("wavelength", wavelength), ("range_bin_m", range_bin_m), ("chirp_period_s", chirp_period_s),
                     ("frame_rate_hz", frame_rate_hz)):
            if not (isinstance(v, (int, float, np.floating)) and np.isfinite(v) and v > 0):
                raise ValueError("RadarModel: %s must be positive and finite, got %r" % (k, v))
        self.wavelength, self.range_bin_m = float(wavelength), float(range_bin_m)
        self.chirp_period_s, self.frame_rate_hz = float(chirp_period_s), float(frame_rate_hz)
        if 192 * self.chirp_period_s > 1.0 / self.frame_rate_hz:
            raise ValueError("RadarModel: a burst of 192 chirps (%g s) does not fit a frame (%g s)"
                             % (192 * self.chirp_period_s, 1.0 / self.frame_rate_hz))
        self.sensors = {}
        for name, rot, org in (("hori", np.eye(3), (0.0, 0.0, 0.0)), ("vert", vert_rotation, vert_origin)):
            tx, rx = iwr1843_array(self.wavelength, rot, org)
            self.sensors[name] = (tx, rx, np.asarray(rot, dtype=np.float64), np.asarray(org, dtype=np.float64))

    def array(self, sensor):
        """-> (tx, rx) of "hori" or "vert"."""
        return self.sensors[sensor][:2]

    def expected_cell(self, sensor, p, v=(0.0, 0.0, 0.0)):
        """Where the chain puts a scatterer at ``p`` moving at ``v``, far field: (range index, azimuth index, signed Doppler bin) as
        floats, in the indexing of the chain's output (range index = 94 - range bin, azimuth index = 31 - azimuth bin, Doppler plane
        = bin + 8).  The sensor's "azimuth" is the direction cosine along its own x axis."""
        _, _, rot, org = self.sensors[sensor]
        d = np.asarray(p, dtype=np.float64) - org
        r = float(np.linalg.norm(d))
        u = d / r
        az_bin = 32.0 * float(u @ rot[:, 0])
        doppler_bin = 64.0 * float(np.asarray(v, dtype=np.float64) @ u) * 6.0 * self.chirp_period_s / self.wavelength
        return 94.0 - r / self.range_bin_m, 31.0 - az_bin, doppler_bin


# ---- the body -----------------------------------------------------------------------------------------------------------------------------
# joints in cfg.DATASET.idxToJoints order: R_Hip, R_Knee, R_Ankle, L_Hip, L_Knee, L_Ankle, Neck, Head, L_Shoulder, L_Elbow, L_Wrist,
# R_Shoulder, R_Elbow, R_Wrist.  The person faces the radar, so their right is the radar's left (-x).
HIP_HALF, THIGH, SHANK = 0.10, 0.44, 0.42
NECK_UP, HEAD_UP, SHOULDER_HALF, SHOULDER_UP = 0.52, 0.18, 0.19, 0.50
UPPER_ARM, FOREARM = 0.29, 0.26
PELVIS_Z = -0.08                       # pelvis height relative to the radar (mounted about 1 m above the floor)
POINTS_PER_BONE = 2
CHEST_UP = 0.6                         # the chest plate sits 60 % of the way from the pelvis to the neck
TORSO_OFFSETS = tuple((dx, dz) for dz in (-0.03, 0.03) for dx in (-0.04, 0.0, 0.04))     # metres: a compact plate, about one cell wide
TORSO_POINTS = len(TORSO_OFFSETS)
S_BODY = 14 + 13 * POINTS_PER_BONE + TORSO_POINTS        # 46 scatterers


class Body:
    """``walking_body``'s result: ``joints3d`` (frames, 14, 3) metres; the scatterer set ``pos``, ``vel`` (frames, S, 3) fp64 and ``amp``
    (frames, S) fp32 at the start of each frame's burst; ``torso`` the indices of the torso scatterers; ``rate_hz``."""
    __slots__ = ("joints3d", "pos", "vel", "amp", "torso", "rate_hz")

    def __init__(self, joints3d, pos, vel, amp, torso, rate_hz):
        self.joints3d, self.pos, self.vel, self.amp, self.torso, self.rate_hz = joints3d, pos, vel, amp, torso, rate_hz

    def with_amp(self, amp):
        """The same body with other amplitudes (zeros: an empty room with the same geometry)."""
        return Body(self.joints3d, self.pos, self.vel, np.ascontiguousarray(np.broadcast_to(amp, self.amp.shape), dtype=np.float32),
                    self.torso, self.rate_hz)


def _limb(root, a1, l1, a2, l2):
    """Two segments hanging from ``root`` (..., 3), swung in the (y, z) plane: pitch ``a1`` of the first (positive = towards -y, the
    radar), ``a2`` of the second -> (middle joint, end joint)."""
    mid = root + l1 * np.stack([np.zeros_like(a1), -np.sin(a1), -np.cos(a1)], -1)
    end = mid + l2 * np.stack([np.zeros_like(a2), -np.sin(a2), -np.cos(a2)], -1)
    return mid, end


def _joints_at(t, par):
    """(n,) seconds -> (n, 14, 3): the template skeleton translated along its walk, legs and arms swung about hips and shoulders.
    Every bone is a rigid segment or part of the rigid trunk, so its length does not depend on t."""
    t = np.asarray(t, dtype=np.float64)
    s = par["scale"]
    pelvis = np.stack([par["x0"] + par["xa"] * np.sin(2 * np.pi * t / par["x_period"] + par["x_phase"]),
                       par["y0"] + par["ya"] * np.sin(2 * np.pi * t / par["y_period"] + par["y_phase"]),
                       PELVIS_Z * s + 0.02 * s * np.cos(4 * np.pi * par["stride_hz"] * t + 2 * par["gait_phase"])], -1)
    g = 2 * np.pi * par["stride_hz"] * t + par["gait_phase"]
    leg, arm = par["leg_swing"] * np.sin(g), par["arm_swing"] * np.sin(g)
    flex_r, flex_l = par["knee_flex"] * 0.5 * (1 - np.cos(g)), par["knee_flex"] * 0.5 * (1 + np.cos(g))
    x = np.array([1.0, 0.0, 0.0])
    z = np.array([0.0, 0.0, 1.0])
    J = np.empty(t.shape + (14, 3))
    J[..., 0, :] = pelvis - HIP_HALF * s * x
    J[..., 3, :] = pelvis + HIP_HALF * s * x
    J[..., 1, :], J[..., 2, :] = _limb(J[..., 0, :], leg, THIGH * s, leg - flex_r, SHANK * s)
    J[..., 4, :], J[..., 5, :] = _limb(J[..., 3, :], -leg, THIGH * s, -leg - flex_l, SHANK * s)
    J[..., 6, :] = pelvis + NECK_UP * s * z
    J[..., 7, :] = J[..., 6, :] + HEAD_UP * s * z
    J[..., 8, :] = pelvis + SHOULDER_UP * s * z + SHOULDER_HALF * s * x
    J[..., 11, :] = pelvis + SHOULDER_UP * s * z - SHOULDER_HALF * s * x
    J[..., 9, :], J[..., 10, :] = _limb(J[..., 8, :], arm, UPPER_ARM * s, arm + par["elbow_bend"], FOREARM * s)
    J[..., 12, :], J[..., 13, :] = _limb(J[..., 11, :], -arm, UPPER_ARM * s, -arm + par["elbow_bend"], FOREARM * s)
    return J


def _scatterers_at(t, par):
    """(n,) -> (n, S_BODY, 3): the joints, POINTS_PER_BONE interior points on each of the 13 bones, TORSO_POINTS on a small chest plate."""
    from .datasets.base import SKELETON
    J = _joints_at(t, par)
    pts = [J]
    for u, v in SKELETON:
        a, b = J[..., u - 1, :], J[..., v - 1, :]
        for k in range(1, POINTS_PER_BONE + 1):
            w = k / (POINTS_PER_BONE + 1.0)
            pts.append(((1 - w) * a + w * b)[..., None, :])
    chest = 0.5 * (J[..., 0, :] + J[..., 3, :]) * (1 - CHEST_UP) + CHEST_UP * J[..., 6, :]
    for dx, dz in TORSO_OFFSETS:
        pts.append((chest + np.array([dx, 0.0, dz]))[..., None, :])
    return np.concatenate(pts, axis=-2)


def walking_body(frames, rate_hz=DEFAULT_FRAME_RATE_HZ, seed=0, amplitude=150.0, torso_gain=4.0, y_range=(1.6, 3.1), dt=1e-3):
    """A person walking back and forth in front of the radar for ``frames`` frames at ``rate_hz`` -> a ``Body``.  The pelvis moves
    sinusoidally in depth inside ``y_range`` (metres; the default stays inside the range bins the chain keeps) and sways sideways; legs
    and arms swing at the stride frequency, the knee flexes during its leg's swing.  Scale, walk and gait phases are drawn from
    ``seed``.  Velocities are central differences of the positions over ``2 dt``.  ``amplitude`` is a joint's amplitude at 1 m / 1 m
    (received: amplitude / (|p - tx| |p - rx|) ADC units); a torso point has ``torso_gain`` times that."""
    frames = int(frames)
    if frames < 0 or not rate_hz > 0:
        raise ValueError("walking_body: frames >= 0 and rate_hz > 0, got %r, %r" % (frames, rate_hz))
    u = synth.uniform01(12, "walking_body", int(seed))
    lo, hi = float(y_range[0]), float(y_range[1])
    scale = 0.9 + 0.2 * u[0]
    reach = 0.45 * scale                                           # how far a hand or foot gets ahead of the pelvis
    if hi - lo <= 2 * reach + 0.1:
        raise ValueError("walking_body: y_range %r is too narrow for the body" % (y_range,))
    par = dict(scale=scale, x0=-0.3 + 0.6 * u[1], xa=0.10 + 0.15 * u[2], x_period=5.0 + 4.0 * u[3], x_phase=2 * np.pi * u[4],
               y0=0.5 * (lo + hi), ya=0.5 * (hi - lo) - reach, y_period=4.0 + 2.0 * u[5], y_phase=2 * np.pi * u[6],
               stride_hz=0.8 + 0.3 * u[7], gait_phase=2 * np.pi * u[8], leg_swing=0.35 + 0.15 * u[9], arm_swing=0.35 + 0.2 * u[10],
               knee_flex=0.5 + 0.3 * u[11], elbow_bend=0.3)
    t = np.arange(frames, dtype=np.float64) / float(rate_hz)
    pos = _scatterers_at(t, par)
    vel = (_scatterers_at(t + dt, par) - _scatterers_at(t - dt, par)) / (2.0 * dt)
    a = np.full(S_BODY, amplitude, dtype=np.float32)
    torso = np.arange(S_BODY - TORSO_POINTS, S_BODY)
    a[torso] *= np.float32(torso_gain)
    amp = np.ascontiguousarray(np.broadcast_to(a, (frames, S_BODY)))
    return Body(np.ascontiguousarray(pos[:, :14]), np.ascontiguousarray(pos), np.ascontiguousarray(vel), amp, torso, float(rate_hz))


# ---- the camera ---------------------------------------------------------------------------------------------------------------------------
DEFAULT_CAMERA = dict(position=(0.1, 0.0, 0.0), focal_px=110.0, centre=(128.0, 128.0), size=256)


def project_joints(joints3d, camera=None):
    """(..., 3) metres -> (..., 2) label-image pixels (x to the right, y down) through a pinhole camera beside the radar looking along
    +y: x = cx + f (X - Xc) / (Y - Yc), y = cy - f (Z - Zc) / (Y - Yc), clipped to the image [0, size - 1].  ``camera``: a dict with
    the keys of ``DEFAULT_CAMERA`` (None: that one, whose focal length keeps a person 1.4 m away inside the 256 x 256 image)."""
    cam = dict(DEFAULT_CAMERA, **(camera or {}))
    j = np.asarray(joints3d, dtype=np.float64) - np.asarray(cam["position"], dtype=np.float64)
    depth = j[..., 1]
    if (depth <= 0).any():
        raise ValueError("project_joints: a joint is behind the camera")
    f, (cx, cy), top = float(cam["focal_px"]), cam["centre"], float(cam["size"]) - 1.0
    return np.stack([np.clip(cx + f * j[..., 0] / depth, 0.0, top), np.clip(cy - f * j[..., 2] / depth, 0.0, top)], -1)


def annotations(joints3d, camera=None, margin=8.0):
    """One sequence's block list in the layout of ``synth.tiny_annotations``: {image, joints (14 x [x, y]), bbox [x0, y0, x1, y1]}."""
    uv = project_joints(joints3d, camera)
    top = float(dict(DEFAULT_CAMERA, **(camera or {}))["size"]) - 1.0
    out = []
    for fr in range(uv.shape[0]):
        lo, hi = np.clip(uv[fr].min(0) - margin, 0.0, top), np.clip(uv[fr].max(0) + margin, 0.0, top)
        out.append({"image": "%09d.jpg" % fr, "joints": uv[fr].tolist(), "bbox": [float(lo[0]), float(lo[1]), float(hi[0]), float(hi[1])]})
    return out


# ---- cubes and data sets ------------------------------------------------------------------------------------------------------------------
def simulate_sequence(model, body, noise_std=2.0, seed=0, device="cuda", block=64):
    """Both sensors' int16 cubes (frames, 4, 192, 256, 2) of ``body`` on ``device`` -> (hori, vert).  ``noise_std``: receiver noise per
    I / Q component in ADC units, drawn from a torch generator on the device seeded with ``seed`` (the draws do not depend on the
    body, so the same seed with all amplitudes zero is the empty room under the same noise); 0 adds none.  Frames go through the
    kernel ``block`` at a time to bound the noise tensor."""
    import torch
    from . import functional as F_
    dev = torch.device(device)
    if dev.type != "cuda":
        raise F_.rt.HuprError("simulate_sequence needs a GPU (no CPU fallback), got %s" % dev)
    frames = body.pos.shape[0]
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    pos, vel, amp = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (body.pos, body.vel, body.amp))
    out = []
    for sensor in ("hori", "vert"):
        tx, rx = model.array(sensor)
        cube = torch.empty((frames, 4, 192, 256, 2), dtype=torch.int16, device=dev)
        for f0 in range(0, frames, block):
            f1 = min(frames, f0 + block)
            add = None
            if noise_std > 0:
                add = torch.randn((f1 - f0, 4, 192, 256, 2), generator=gen, device=dev, dtype=torch.float32) * float(noise_std)
            cube[f0:f1] = F_.radar_scene(pos[f0:f1], vel[f0:f1], amp[f0:f1], tx, rx, model.wavelength, model.range_bin_m,
                                         model.chirp_period_s, add=add)
        out.append(cube)
    return out[0], out[1]


def sequence_seed(seed, seq):
    """The seed of sequence ``seq`` of a data set made with ``seed`` (body and noise)."""
    return int(synth.raw_u64(1, "simulated_sequence", int(seed), int(seq))[0] >> np.uint64(33))


def sequence_names(sequences):
    """``sequences``: an int N (N training sequences single_1 .. single_N and single_<N + 1> for both val and test) or a mapping
    phase -> sequence numbers -> {phase: [numbers]}."""
    if isinstance(sequences, (int, np.integer)) and not isinstance(sequences, bool):
        if sequences < 1:
            raise ValueError("sequences must be at least 1, got %d" % sequences)
        n = int(sequences)
        return {"train": list(range(1, n + 1)), "val": [n + 1], "test": [n + 1]}
    if not isinstance(sequences, dict) or not sequences:
        raise ValueError("sequences must be a positive int or a mapping phase -> sequence numbers, got %r" % (sequences,))
    return {str(ph): [int(s) for s in seqs] for ph, seqs in sequences.items()}


def write_simulated_dataset(root, sequences, frames, seed, model=None, noise_std=2.0, interference=False, camera=None, simulate=None,
                            device="cuda"):
    """A HuPR tree of simulated recordings under ``root``: per sequence ``single_<n>/{hori,vert}/adc_data.bin`` (through
    ``synth.dca1000_encode``) and per phase ``hrnet_annot_<phase>.json`` (the layout of ``synth.tiny_annotations``), which
    ``HuPRRawADC``, ``Runner`` and ``python -m hupr_amd.tools.stream`` read as they read a capture.  ``sequences``: see
    ``sequence_names``; every sequence is ``walking_body(frames, model.frame_rate_hz, sequence_seed(seed, n))`` under noise of the same
    seed.  ``interference``: pass every cube through ``synth.interference_bursts`` (six chirps drawn per sequence).  ``simulate``: the
    function making the two cubes (None: ``simulate_sequence``, which needs the GPU).  -> ``root``."""
    model = model or RadarModel()
    names = sequence_names(sequences)
    simulate = simulate or (lambda m, b, noise_std, seed: simulate_sequence(m, b, noise_std=noise_std, seed=seed, device=device))
    os.makedirs(root, exist_ok=True)
    bodies = {}
    for phase, seqs in names.items():
        for seq in seqs:
            if seq not in bodies:
                s = sequence_seed(seed, seq)
                body = bodies[seq] = walking_body(frames, model.frame_rate_hz, s)
                cubes = simulate(model, body, noise_std=noise_std, seed=s)
                for si, (sensor, cube) in enumerate(zip(("hori", "vert"), cubes)):
                    cube = cube.cpu().numpy() if hasattr(cube, "cpu") else np.asarray(cube)
                    if interference:
                        chirps = sorted(set(int(c) for c in synth.randint((6,), 0, 192, "simulated_interference", s, si)))
                        cube, _ = synth.interference_bursts(cube, chirps, seed=s + si)
                    d = os.path.join(root, "single_%d" % seq, sensor)
                    os.makedirs(d, exist_ok=True)
                    synth.dca1000_encode(cube).tofile(os.path.join(d, "adc_data.bin"))
        with open(os.path.join(root, "hrnet_annot_%s.json" % phase), "w") as fp:
            json.dump([annotations(bodies[seq].joints3d, camera) for seq in seqs], fp)
    return root
