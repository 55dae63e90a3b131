"""Device time of functional.radar_scene for one 600-frame sensor sequence of the default walking body (46 scatterers), and for
context the host time of the numpy fp64 statement (tests/radar_scene_ref.py) on a few frames scaled to 600.  The figures of DESIGN.md
section 6 come from this script:  python scripts/radar_scene_time.py [--frames 600] [--reps 10] [--rounds 3] [--ref-frames 2]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=600)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--ref-frames", type=int, default=2)
    a = p.parse_args(argv)
    import radar_scene_ref as R
    from hupr_amd import functional as F_
    from hupr_amd import simulate as sim
    assert torch.cuda.is_available(), "needs the GPU: a CPU run gives no time"
    m = sim.RadarModel()
    body = sim.walking_body(a.frames, m.frame_rate_hz, 0)
    tx, rx = m.array("hori")
    pos, vel, amp = (torch.from_numpy(x).cuda() for x in (body.pos, body.vel, body.amp))
    S = body.pos.shape[1]
    exps = a.frames * 4 * 192 * 256 * S
    args = (pos, vel, amp, tx, rx, m.wavelength, m.range_bin_m, m.chirp_period_s)
    for dtype in (torch.int16, torch.float32):
        for _ in range(2):
            F_.radar_scene(*args, out_dtype=dtype)
        torch.cuda.synchronize()
        for r in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                F_.radar_scene(*args, out_dtype=dtype)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            print("%s out, %d frames, S = %d, round %d: %.3f ms per call (%d calls), %.2f us per sensor-frame, %.3e complex exponentials/s"
                  % (str(dtype).split(".")[1], a.frames, S, r, ms, a.reps, 1e3 * ms / a.frames, exps / (ms * 1e-3)))
    n = a.ref_frames
    t0 = time.perf_counter()
    R.radar_scene_ref(body.pos[:n], body.vel[:n], body.amp[:n], tx, rx, m.wavelength, m.range_bin_m, m.chirp_period_s)
    dt = time.perf_counter() - t0
    print("numpy fp64 statement: %.2f s for %d frames = %.2f s per frame, %.0f s scaled to %d frames" % (dt, n, dt / n, dt / n * a.frames, a.frames))


if __name__ == "__main__":
    main()
