"""``python -m hupr_amd.tools.points --data DIR --seq NAME [--frames A:B] --out FILE.npz [--ply DIR] [--tdm-compensation] [--pfa ...]``:
the radar point cloud of one recording (preprocessing/points.py).  Reads ``DIR/NAME/{hori,vert}/adc_data.bin`` as
``python -m hupr_amd.tools.stream --raw DIR/NAME`` does (the ``HuPRRawADC`` layout, hence also a tree written by
``python -m hupr_amd.tools.simulate``), writes ``cloud`` (frames, max_points, 8), ``counts`` (frames,) and both sensors' ``points_h`` /
``points_v`` (frames, max_points, 6) with their ``counts_h`` / ``counts_v`` (frames, 2) to FILE.npz, and with ``--ply`` one ASCII
``%09d.ply`` per frame.  The metres rest on the simulator's guessed chirp constants: on a real capture they are guesses."""
import argparse
import os
import sys

import numpy as np

PLY_FIELDS = ("x", "y", "z", "velocity", "snr_h", "snr_v")


def _frames(text):
    """"A:B" (either side may be empty) -> (A or 0, B or None)."""
    try:
        lo, hi = text.split(":")
        lo, hi = (int(lo) if lo else 0), (int(hi) if hi else None)
    except ValueError:
        raise argparse.ArgumentTypeError("frames must be A:B, got %r" % text) from None
    if lo < 0 or (hi is not None and hi < lo):
        raise argparse.ArgumentTypeError("frames A:B needs 0 <= A <= B, got %r" % text)
    return lo, hi


def parse(argv=None):
    from ..preprocessing.points import PointCloudSettings
    p = argparse.ArgumentParser(prog="python -m hupr_amd.tools.points", description=__doc__)
    p.add_argument("--data", required=True, help="directory holding the sequences")
    p.add_argument("--seq", required=True, help="sequence name, e.g. single_1: DATA/SEQ/{hori,vert}/adc_data.bin")
    p.add_argument("--frames", type=_frames, default=(0, None), help="A:B, the frames A <= f < B (default: all)")
    p.add_argument("--out", required=True, help="the .npz file to write")
    p.add_argument("--ply", default=None, help="directory for one ASCII .ply per frame (created)")
    p.add_argument("--tdm-compensation", action="store_true", help="compensate the TDM Doppler phase in the FFT chain")
    p.add_argument("--pfa", type=float, default=None, help="design false-alarm probability per cell (default 1e-5)")
    p.add_argument("--cfar-guard", type=int, default=None, help="half-width of the guard area (default 2)")
    p.add_argument("--cfar-train", type=int, default=None, help="half-width of the training area beyond it (default 4)")
    p.add_argument("--sep-range", type=int, default=None, help="a point dominates the cells this many ranges around it (default 1)")
    p.add_argument("--sep-azimuth", type=int, default=None, help="... and this many azimuth cells around it (default 4)")
    p.add_argument("--range-gate", type=float, default=None, help="largest range difference of a pair, range bins (default 1.5)")
    p.add_argument("--doppler-gate", type=int, default=None, help="largest Doppler difference of a pair, bins (default 1)")
    p.add_argument("--max-points", type=int, default=None, help="rows per frame, 1..256 (default 64)")
    p.add_argument("--block", type=int, default=64, help="frames per pass (default 64)")
    a = p.parse_args(argv)
    if a.block < 1:
        p.error("--block must be at least 1")
    try:
        a.settings = settings_from_args(a)
    except ValueError as e:
        p.error(str(e))
    assert isinstance(a.settings, PointCloudSettings)
    return a


def settings_from_args(a):
    from ..preprocessing.points import PointCloudSettings
    given = dict(pfa=a.pfa, guard=a.cfar_guard, train=a.cfar_train, sep_range=a.sep_range, sep_azimuth=a.sep_azimuth,
                 range_gate=a.range_gate, doppler_gate=a.doppler_gate, max_points=a.max_points)
    return PointCloudSettings(**{k: v for k, v in given.items() if v is not None})


def write_ply(path, rows):
    """``rows`` (k, 8) of one frame's cloud -> an ASCII PLY of k vertices with the float properties of ``PLY_FIELDS``."""
    with open(path, "w") as fp:
        fp.write("ply\nformat ascii 1.0\ncomment radar point cloud: metres, metres per second (receding positive), SNR per sensor\n")
        fp.write("element vertex %d\n" % len(rows))
        for name in PLY_FIELDS:
            fp.write("property float %s\n" % name)
        fp.write("end_header\n")
        for row in rows:
            fp.write(" ".join("%.9g" % float(v) for v in row[:len(PLY_FIELDS)]) + "\n")


def main(argv=None):
    a = parse(argv)
    import torch
    from .. import runtime as rt
    from ..preprocessing.points import radar_point_cloud
    from ..preprocessing.process_iwr1843 import dca1000_frames
    if not torch.cuda.is_available():
        raise rt.HuprError("the point cloud needs a GPU (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    cubes = []
    for sensor in ("hori", "vert"):
        raw = torch.from_numpy(np.fromfile(os.path.join(a.data, a.seq, sensor, "adc_data.bin"), dtype=np.int16)).to(dev)
        cubes.append(dca1000_frames(raw))
    n = min(cubes[0].shape[0], cubes[1].shape[0])
    lo, hi = a.frames[0], n if a.frames[1] is None else min(a.frames[1], n)
    parts = {k: [] for k in ("cloud", "counts", "points_h", "counts_h", "points_v", "counts_v")}
    for f0 in range(lo, hi, a.block):
        f1 = min(hi, f0 + a.block)
        rc = radar_point_cloud(cubes[0][f0:f1], cubes[1][f0:f1], settings=a.settings, tdm_compensation=a.tdm_compensation)
        for k, t in (("cloud", rc.cloud), ("counts", rc.counts), ("points_h", rc.peaks_h.points), ("counts_h", rc.peaks_h.counts),
                     ("points_v", rc.peaks_v.points), ("counts_v", rc.peaks_v.counts)):
            parts[k].append(t.cpu().numpy())
    mp = a.settings.max_points
    empty = dict(cloud=(0, mp, 8), counts=(0,), points_h=(0, mp, 6), counts_h=(0, 2), points_v=(0, mp, 6), counts_v=(0, 2))
    out = {k: (np.concatenate(v) if v else np.zeros(empty[k], np.int32 if k.startswith("counts") else np.float32)) for k, v in parts.items()}
    np.savez(a.out, frames=np.arange(lo, max(hi, lo)), **out)
    if a.ply:
        os.makedirs(a.ply, exist_ok=True)
        for k, f in enumerate(range(lo, hi)):
            write_ply(os.path.join(a.ply, "%09d.ply" % f), out["cloud"][k, :out["counts"][k]])
    frames = len(out["counts"])
    mean = float(out["counts"].mean()) if frames else 0.0
    none = float((out["counts"] == 0).mean()) if frames else 0.0
    print("point cloud of %s: %d frames, %.2f points per frame, %.1f %% of the frames without a point; metres on guessed chirp constants"
          % (os.path.join(a.data, a.seq), frames, mean, 100.0 * none))
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
