#!/usr/bin/env python
"""The forked window of the --temporal step, batch by batch, from a rocprofv3 kernel trace (..._kernel_trace.csv): for each of
the last ROTATE replayed steps (bench.py rotates over 6 batches) the start and end of march_pair_kernel and of the producer
chain (dyn_extents16, dyn_synth_fwd4, the fused sweep photo_march_*), in microseconds relative to the END of the marching
pass that precedes the window (the last march_* dispatch that ends before march_pair_kernel starts).
    python scripts/pair_window_timeline.py <kernel_trace.csv> [rotate=6]"""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
R = int(sys.argv[2]) if len(sys.argv) > 2 else 6
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
first = [i for i, r in enumerate(rows) if "pack_identity_kernel" in r["Kernel_Name"]]
if len(first) < 2 * R + 1:
    sys.exit("too few steps in the trace")
WATCH = ("march_pair_kernel", "dyn_extents", "dyn_synth_fwd", "photo_march")
print("%-5s %-34s %8s %8s %8s" % ("step", "kernel", "start", "end", "us"))
for n, (i0, i1) in enumerate(zip(first[-R - 1:-1], first[-R:])):
    step = rows[i0:i1]
    pair = next((r for r in step if "march_pair_kernel" in r["Kernel_Name"]), None)
    if pair is None:
        print(n, "no march_pair_kernel in this step")
        continue
    before = [r for r in step if "march_" in r["Kernel_Name"] and "photo_march" not in r["Kernel_Name"] and
              int(r["End_Timestamp"]) <= int(pair["Start_Timestamp"])]
    t0 = max(int(r["End_Timestamp"]) for r in before) if before else int(pair["Start_Timestamp"])
    for r in step:
        name = r["Kernel_Name"].replace("void mal::", "").replace("mal::", "")
        if any(w in name for w in WATCH) and int(r["Start_Timestamp"]) >= t0 - 1000:
            s, e = (int(r["Start_Timestamp"]) - t0) / 1e3, (int(r["End_Timestamp"]) - t0) / 1e3
            print("%-5d %-34s %8.1f %8.1f %8.1f" % (n, name.split("(")[0][:34], s, e, e - s))
    print("%-5d %-34s %8.1f" % (n, "step (first kernel to the next step's)", (int(rows[i1]["Start_Timestamp"]) - int(rows[i0]["Start_Timestamp"])) / 1e3))
