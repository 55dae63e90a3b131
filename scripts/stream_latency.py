"""Per-frame latency of the live stream against the window-per-frame route, in one process, interleaved.

  (a)  PoseStream.push from pinned host frames, graph=True: one hipGraph replay per frame — upload of the 2 new sensor-frames, FFT
       chain, window MNet from the ring, encoders / decoder / heads, arg-max, keypoints.
  (b)  the route without a session: the pinned 16-sensor-frame window of the frame -> upload -> FFT chain to means on all 16 ->
       graph-captured forward (MNet .. heads) + arg-max.  The window is assembled in pinned memory once, outside the timing (the
       12.6 MB host gather a caller pays per frame is not counted against this route).
  (b1) the same with upload and FFT chain inside the graph as well (the most a caller could do without the session).

Device events around every frame, a host clock around every block (ending in a synchronise); the routes alternate block by block.
Medians over all frames, and the spread of (a) as the range of its block medians.

--decode subpixel and / or --smooth (a One-Euro filter at --rate frames per second) put the one-launch decode of
csrc/pose_decode.hip at the tail of route (a) in place of arg-max + keypoints; run once without and once with them to compare.

usage: python scripts/stream_latency.py [--frames 512] [--blocks 8] [--math bf16|f32] [--out profiles/stream_latency.txt]
                                        [--decode argmax|subpixel] [--smooth [--rate 10]]
       python scripts/stream_latency.py --trace-frames 64        (eager session only: the run to put under
                                                                  rocprofv3 --kernel-trace --stats for hupr_k_mnet_stream)"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hupr_amd import runtime as rt, synth
from hupr_amd.config_tree import load_config
from hupr_amd.models import HuPRNet
from hupr_amd.tools.stream import ADC_SHAPE, PoseSmoothing, PoseStream, stream_window_sources

p = argparse.ArgumentParser()
p.add_argument("--frames", type=int, default=512)
p.add_argument("--blocks", type=int, default=8)
p.add_argument("--math", choices=("f32", "bf16"), default="bf16")
p.add_argument("--trace-frames", type=int, default=0)
p.add_argument("--out", type=str, default=None)
p.add_argument("--decode", choices=("argmax", "subpixel"), default="argmax")
p.add_argument("--smooth", action="store_true")
p.add_argument("--rate", type=float, default=10.0)
args = p.parse_args()
decode_kw = dict(decode=args.decode, smooth=PoseSmoothing(args.rate) if args.smooth else None)
if not torch.cuda.is_available():
    raise SystemExit("stream_latency.py measures on the GPU; none is visible")

dev = torch.device("cuda", 0)
cfg = load_config()
G, K, H = cfg.DATASET.numGroupFrames, cfg.DATASET.numKeypoints, cfg.DATASET.heatmapSize
model = HuPRNet(cfg).to(dev).eval()
model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.hupr_state(1, gain=1.4).items()})
model.math_mode = args.math
POOL = 24                                              # distinct synthetic frames, cycled (the content does not change the work)
pool = [[torch.from_numpy(synth.adc_cube_int16(9, frame=f, sensor=s)).pin_memory() for s in range(2)] for f in range(POOL)]

if args.trace_frames:
    s = PoseStream(model, cfg, graph=False, **decode_kw)
    for n in range(args.trace_frames):
        s.push(pool[n % POOL][0], pool[n % POOL][1])
    s.flush()
    torch.cuda.synchronize()
    print("traced %d eager pushes" % args.trace_frames)
    raise SystemExit(0)

L = rt.lib()
session = PoseStream(model, cfg, graph=True, **decode_kw)

# (b) / (b1): static buffers, the window gathered on the host into pinned memory the way a caller without a session would
win_pinned = torch.empty((2, G) + ADC_SHAPE, dtype=torch.int16).pin_memory()
win_dev = torch.empty((2, G) + ADC_SHAPE, dtype=torch.int16, device=dev)
means = torch.empty((2, 1, G, 16, 64, 64), dtype=torch.float32, device=dev)
ws_bytes = int(L.hupr_fft_chain_ws_bytes(2 * G))
ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
am = torch.empty(K, dtype=torch.int32, device=dev)
mx = torch.empty(K, dtype=torch.float32, device=dev)


def b_front():
    win_dev.copy_(win_pinned, non_blocking=True)
    rt.check(L.hupr_fft_chain_loader_means_f32(rt.ptr(win_dev), 2 * G, rt.ptr(means), rt.ptr(ws), ws_bytes, rt.stream()))


def b_back():
    heat, gcn = model(means[0], means[1])
    rt.check(L.hupr_argmax_rows_f32(rt.ptr(gcn), K, H * H, rt.ptr(am), rt.ptr(mx), rt.stream()))
    return heat, gcn


def gather(n):
    for j, f in enumerate(stream_window_sources(n - session.lookahead, n, G)):
        win_pinned[0, j].copy_(pool[f % POOL][0][0])
        win_pinned[1, j].copy_(pool[f % POOL][1][0])


with torch.no_grad():
    gather(0)
    for _ in range(2):
        b_front()
        b_back()
    torch.cuda.synchronize()
    g_back, g_all = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_back):
        keep_b = b_back()
    with torch.cuda.graph(g_all):
        b_front()
        keep_b1 = b_back()


def run_a(n):
    session.push(pool[n % POOL][0], pool[n % POOL][1])


def run_b(n):
    b_front()
    model._refresh_packed(dev)
    g_back.replay()


def run_b1(n):
    model._refresh_packed(dev)
    g_all.replay()


routes = {"a": run_a, "b": run_b, "b1": run_b1}
for n in range(16):                                   # warm-up: the session captures its graph here
    for fn in routes.values():
        fn(n)
torch.cuda.synchronize()
assert session._graphs, "the session did not reach its graph"

per_block = args.frames // args.blocks
dev_ms = {k: [] for k in routes}
host_ms = {k: [] for k in routes}
block_medians = {k: [] for k in routes}
n = 16
for b in range(args.blocks):
    for name, fn in routes.items():
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(per_block)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(per_block):
            ev[i][0].record()
            fn(n + i)
            ev[i][1].record()
            ev[i][1].synchronize()                    # a live stream answers a frame before the next one arrives
        torch.cuda.synchronize()
        host_ms[name].append((time.perf_counter() - t0) * 1e3 / per_block)
        t = [a.elapsed_time(z) for a, z in ev]
        dev_ms[name].extend(t)
        block_medians[name].append(statistics.median(t))
    n += per_block

lines = ["stream_latency.py --frames %d --blocks %d --math %s --decode %s%s   (lanes 1, G %d, lookahead %d; %s)"
         % (args.frames, args.blocks, args.math, args.decode, " --smooth --rate %g" % args.rate if args.smooth else "", G,
            session.lookahead, torch.cuda.get_device_name(0)),
         "route  frames  device-event median ms  [block medians min .. max]  host clock ms/frame (mean of blocks)"]
label = {"a": "(a)  PoseStream.push, one graph replay", "b": "(b)  window upload + FFT eager, graph forward + arg-max",
         "b1": "(b1) window upload + FFT + forward + arg-max in one graph"}
for k in routes:
    lines.append("%-58s %5d  %8.3f  [%.3f .. %.3f]  %8.3f" % (label[k], len(dev_ms[k]), statistics.median(dev_ms[k]),
                                                              min(block_medians[k]), max(block_medians[k]), statistics.mean(host_ms[k])))
spread = max(block_medians["a"]) - min(block_medians["a"])
lines.append("run-to-run spread of (a): %.3f ms between block medians; (b) - (a) = %.3f ms, (b1) - (a) = %.3f ms (device-event medians)"
             % (spread, statistics.median(dev_ms["b"]) - statistics.median(dev_ms["a"]), statistics.median(dev_ms["b1"]) - statistics.median(dev_ms["a"])))
text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as fp:
        fp.write(text + "\n")
