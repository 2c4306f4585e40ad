"""Dead-sample sweep of the headline step (bench.py --mode step: B=12 192x640 --temporal --distil, cold regime).

Times the graph-replayed step, rotating over 6 batches as bench.py does, with every batch's augmentation tensor overwritten
to all-zero (nothing to skip), left at the benchmark's own values (about half the samples augmented) and set to all-one
(everything skipped), under option "student_overlap" 1 (a launch per forked pass, every sample computed) and 2 (one launch,
augmented samples skipped) -- the latter under "side_order" 0 and 1.  The schedules are captured once each over the same
batches and workspaces and then timed alternately, --reps times, so that drift of the box hits all of them alike.

    python scripts/aug_skip_sweep.py [--steps 1200] [--reps 5] [--dead K ...] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=6)
    ap.add_argument("--dead", type=int, nargs="*", default=[], help="also: exactly K augmented samples in every batch (the first K)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aug_skip_sweep.py needs a HIP device")
    import bench
    from mal_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    R = args.rotate
    rot = bench.Rotation(dev, 1234, "step", R, graph=False)
    own = [s.aug.clone() for s in rot.steps]
    schedules = {"overlap1": {"student_overlap": 1, "side_order": 0}, "overlap2": {"student_overlap": 2, "side_order": 0},
                 "overlap2_side1": {"student_overlap": 2, "side_order": 1}}
    graphs = {}
    for name, opts in schedules.items():
        for k, v in opts.items():
            _lib.check(lib.mal_set_option(k.encode(), v), "mal_set_option(%s)" % k)
        rot.capture()
        if rot.graphs is None:
            raise SystemExit("graph capture failed: %s" % rot.note)
        graphs[name] = rot.graphs
    patterns = {"all_zero": lambda a: torch.zeros_like(a), "bench": lambda a: a, "all_one": lambda a: torch.ones_like(a)}
    dead = {"all_zero": 0, "bench": int(sum(float(a.sum()) for a in own)), "all_one": R * int(own[0].numel())}
    for k in args.dead:
        patterns["dead_%d" % k] = lambda a, k=k: (torch.arange(a.numel(), device=a.device) < k).to(a.dtype).reshape(a.shape)
        dead["dead_%d" % k] = R * k

    def timed(gs):
        for i in range(10 * R):
            gs[i % R].replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            gs[i % R].replay()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    t_ramp = time.perf_counter()  # sustained clocks first
    while time.perf_counter() - t_ramp < 0.3:
        timed(graphs["overlap1"])
    ms = {(p, s): [] for p in patterns for s in schedules}
    for _ in range(args.reps):
        for p, f in patterns.items():
            for s_, a in zip(rot.steps, own):
                s_.aug.copy_(f(a))
            for s in schedules:
                ms[(p, s)].append(timed(graphs[s]))
    out = {"steps": args.steps, "reps": args.reps, "samples": R * int(own[0].numel()), "dead_samples": dead, "ms_per_step": {}}
    print("%-9s %-15s %8s %8s %8s   (ms per step: median, min, max of %d)" % ("pattern", "schedule", "median", "min", "max", args.reps))
    for (p, s), v in ms.items():
        out["ms_per_step"]["%s/%s" % (p, s)] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}
        print("%-9s %-15s %8.4f %8.4f %8.4f" % (p, s, statistics.median(v), min(v), max(v)))
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
