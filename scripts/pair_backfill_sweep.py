"""Per-live-count sweep of the headline step (bench.py --mode step: B=12 192x640 --temporal --distil, cold regime) for option
"side_order" (0: the merged launch's arrangement A forced, 2: the device chooses between A and B from the live samples).

Times the graph-replayed step, rotating over 6 batches as bench.py does, with every batch's augmentation tensor left at the
benchmark's own values ("bench") or overwritten so that exactly K samples are augmented (--dead K ...).  One process times
ONE library (MAL_HIP_LIB selects another build of the same ABI, e.g. the parent commit's: give it --orders 0 only, it reads
any non-zero "side_order" as 1); scripts/pair_backfill_ab.sh alternates processes.  Inside a process the schedules are
captured once each over the same batches and timed alternately.

    python scripts/pair_backfill_sweep.py --arm NAME [--orders 0 2] [--dead 0 3 4 5 6] [--steps 1200] [--reps 1] [--out FILE]

Appends one JSON line per run to --out: {"arm", "orders", "ms_per_step": {"<pattern>/side<order>": [..reps..]}}.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", required=True)
    ap.add_argument("--orders", type=int, nargs="+", default=[0, 2])
    ap.add_argument("--dead", type=int, nargs="*", default=[0, 3, 4, 5, 6])
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--rotate", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_backfill_sweep.py needs a HIP device")
    import bench
    from mal_amd import _lib, build
    if not os.environ.get("MAL_HIP_LIB"):
        build.build(verbose=False)
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    R = args.rotate
    rot = bench.Rotation(dev, 1234, "step", R, graph=False)
    own = [s.aug.clone() for s in rot.steps]
    graphs = {}
    for order in args.orders:
        _lib.check(lib.mal_set_option(b"side_order", order), "mal_set_option(side_order)")
        rot.capture()
        if rot.graphs is None:
            raise SystemExit("graph capture failed: %s" % rot.note)
        graphs[order] = rot.graphs
    patterns = {"bench": lambda a: a}
    for k in args.dead:
        patterns["dead_%d" % k] = lambda a, k=k: (torch.arange(a.numel(), device=a.device) < k).to(a.dtype).reshape(a.shape)

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
        timed(graphs[args.orders[0]])
    ms = {"%s/side%d" % (p, o): [] for p in patterns for o in args.orders}
    for _ in range(args.reps):
        for p, f in patterns.items():
            for s_, a in zip(rot.steps, own):
                s_.aug.copy_(f(a))
            for o in args.orders:
                ms["%s/side%d" % (p, o)].append(timed(graphs[o]))
    for k, v in ms.items():
        print("%-10s %-16s %s" % (args.arm, k, " ".join("%.4f" % x for x in v)))
    line = json.dumps({"arm": args.arm, "orders": args.orders, "steps": args.steps, "lib": os.path.basename(os.environ.get("MAL_HIP_LIB", "default")),
                       "ms_per_step": ms})
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
