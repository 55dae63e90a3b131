"""Device time of functional.radar_peaks and functional.radar_points_fuse on 64 frames: both sensors' planes of the default walking
body through the FFT chain and the detector, then the two launches timed with device events.  The figure of DESIGN.md section 6 comes
from this script:  python scripts/radar_points_time.py [--frames 64] [--reps 20]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=64)
    p.add_argument("--reps", type=int, default=20)
    a = p.parse_args(argv)
    from hupr_amd import functional as F_
    from hupr_amd import preprocessing
    from hupr_amd import simulate as sim
    from hupr_amd.preprocessing.points import radar_geometry
    assert torch.cuda.is_available(), "needs the GPU: a CPU run gives no time"
    m = sim.RadarModel()
    cubes = sim.simulate_sequence(m, sim.walking_body(a.frames, m.frame_rate_hz, 0), noise_std=2.0, seed=1)
    dets = []
    for cube in cubes:
        planes = preprocessing.fft_chain_loader_means(cube, tdm_compensation=True)
        dets.append((planes, F_.cfar_ra(planes, want_mask=True, want_snr=True)))
    geo = radar_geometry(m)

    def peaks():
        return [F_.radar_peaks(planes, det.mask, det.snr) for planes, det in dets]

    pk = peaks()
    cloud = F_.radar_points_fuse(pk[0], pk[1], geo)
    torch.cuda.synchronize()
    print("%d frames: %.1f and %.1f points per frame in the two sensors (%.1f and %.1f detected cells), %.1f fused"
          % (a.frames, pk[0].count.float().mean(), pk[1].count.float().mean(), dets[0][1].count.mean(), dets[1][1].count.mean(),
             cloud.counts.float().mean()))
    for name, fn in (("radar_peaks, one sensor", lambda: F_.radar_peaks(dets[0][0], dets[0][1].mask, dets[0][1].snr)),
                     ("radar_points_fuse", lambda: F_.radar_points_fuse(pk[0], pk[1], geo))):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        print("%s: %.4f ms per launch of %d frames (%d launches back to back, one measurement)" % (name, ms, a.frames, a.reps))


if __name__ == "__main__":
    main()
