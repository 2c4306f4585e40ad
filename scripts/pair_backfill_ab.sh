#!/bin/bash
# A/B of option "side_order" 2 (march_pair_kernel's arrangement chosen on the device) against the parent commit's library.
# Needs other builds of the same ABI as mal_amd/lib/<name>.so (scripts/build_variant.py, or a copy of another checkout's
# libmal_hip.so): "parent" = the parent commit, "p1only" = this tree with the parent's mal_dyn.hip (the synthesis kernel at
# its old register count).  One process per arm and repetition, alternating; every GPU step under its own time limit, the
# first failure ends the script.
#   1. per-live-count table: scripts/pair_backfill_sweep.py, 1200 steps x REPS
#   2. headline: python bench.py --gpus 1 --no-cpu-baseline --train-steps 0, parent / this tree with side_order 2 x REPS
#   3. timelines of the forked window, parent and side_order 2 (rocprofv3 kernel trace, cold regime)
# BUDGET (seconds, default none): no new process is started once the script has run that long.
# OUT: the directory that receives sweep.jsonl, headline.txt and timeline_<arm>.txt (default build/pair_backfill, git-ignored).
set -o pipefail
REPS=${REPS:-5}
BUDGET=${BUDGET:-0}
spent() { [ $BUDGET -gt 0 ] && [ $SECONDS -gt $BUDGET ]; }
out=${OUT:-build/pair_backfill}
mkdir -p $out
R=$PWD
lib() { if [ "$1" = default ]; then unset MAL_HIP_LIB; else export MAL_HIP_LIB=$R/mal_amd/lib/$1.so; fi; }


: > $out/sweep.jsonl
for rep in $(seq $REPS); do
  for arm in parent p1only default; do
    if spent; then echo "budget spent in the sweep, rep $rep"; break 2; fi
    lib $arm
    if [ $arm = parent ]; then orders="0"; else orders="0 2"; fi
    timeout -k 10 180 python scripts/pair_backfill_sweep.py --arm $arm --orders $orders --dead 0 3 4 5 6 --out $out/sweep.jsonl \
      2>/dev/null | grep -v amdgpu.ids || { echo "sweep $arm failed"; exit 1; }
  done
done

: > $out/headline.txt
for rep in $(seq $REPS); do
  for arm in parent side2; do
    if spent; then echo "budget spent in the headline, rep $rep"; break 2; fi
    if [ $arm = parent ]; then lib parent; opt=""; else lib default; opt="--opt side_order=2"; fi
    line=$(timeout -k 10 300 python bench.py --gpus 1 --no-cpu-baseline --train-steps 0 $opt 2>/dev/null | tail -1) || { echo "bench $arm failed"; exit 1; }
    echo "$line" | python -c "
import sys, json
d = json.loads(sys.stdin.read())
print('$arm', 'rep', $rep, 'ms_per_step %.4f' % d['ms_per_step'], 'warm %.4f' % d.get('warm_ms_per_step', float('nan')))" | tee -a $out/headline.txt
  done
done

for arm in parent side2; do
  if spent; then echo "budget spent before the timelines"; exit 0; fi
  if [ $arm = parent ]; then lib parent; opt=""; else lib default; opt="--opt side_order=2"; fi
  timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d $out/tl_$arm -o tl -- python3 bench.py --mode step $opt \
    --regime cold --no-cpu-baseline --train-steps 0 --steps 60 > $out/tl_$arm.log 2>&1 || { echo "trace $arm failed"; tail -5 $out/tl_$arm.log; exit 1; }
  python scripts/pair_window_timeline.py "$(find $out/tl_$arm -name '*kernel_trace.csv' | head -1)" > $out/timeline_$arm.txt || exit 1
  rm -rf $out/tl_$arm
done
echo "timelines done"
