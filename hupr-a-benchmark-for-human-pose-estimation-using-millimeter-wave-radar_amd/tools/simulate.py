"""``python -m hupr_amd.tools.simulate --out DIR --sequences N --frames F --seed S [--noise X] [--interference]``: write a HuPR tree
of SIMULATED recordings (hupr_amd.simulate: a walking stick figure of point scatterers seen by both sensors — not real data) that the
raw-capture dataset, the runner and ``python -m hupr_amd.tools.stream --raw DIR/single_<n>`` read as they read a capture."""
import argparse
import sys


def parse(argv=None):
    p = argparse.ArgumentParser(prog="python -m hupr_amd.tools.simulate", description=__doc__)
    p.add_argument("--out", required=True, help="directory to write (created)")
    p.add_argument("--sequences", type=int, required=True, help="N training sequences single_1 .. single_N; single_<N + 1> serves val and test")
    p.add_argument("--frames", type=int, required=True, help="frames per sequence (cfg.DATASET.duration of the tree)")
    p.add_argument("--seed", type=int, required=True)
    p.add_argument("--noise", type=float, default=2.0, help="receiver noise per I / Q component, ADC units (default 2; 0: none)")
    p.add_argument("--interference", action="store_true", help="pass the cubes through synth.interference_bursts")
    p.add_argument("--device", default="cuda")
    a = p.parse_args(argv)
    if a.sequences < 1:
        p.error("--sequences must be at least 1")
    if a.frames < 1:
        p.error("--frames must be at least 1")
    if not a.noise >= 0:
        p.error("--noise must be >= 0")
    return a


def main(argv=None):
    a = parse(argv)
    from .. import simulate as sim
    root = sim.write_simulated_dataset(a.out, a.sequences, a.frames, a.seed, noise_std=a.noise, interference=a.interference, device=a.device)
    names = sim.sequence_names(a.sequences)
    print("simulated (not real) data: %d sequences of %d frames under %s; DATASET.trainName %r valName %r testName %r duration %d"
          % (a.sequences + 1, a.frames, root, names["train"], names["val"], names["test"], a.frames))
    return root


if __name__ == "__main__":
    main(sys.argv[1:])
