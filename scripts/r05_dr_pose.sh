#!/bin/bash
# DualRefine one-call step with / without the pose-update losses, and the operator route: r05_dr_pose.sh OUTDIR
set -e
O=${1:?usage: r05_dr_pose.sh OUTDIR}
mkdir -p $O
python -m pytest tests/test_gpu_decisions.py -x -q -k "pose_update" > $O/pu_tests.txt 2>&1
for v in "" "--dr-pose-update" "--dr-pose-update --dr-default-scales" "--dr-default-scales"; do
  tag=$(echo "dr$v" | tr -d ' ' | tr '-' '_')
  python bench.py --full --mode dualrefine $v --no-cpu-baseline --train-steps 0 2>/dev/null | tail -1 > $O/$tag.json
done
python bench.py --full --mode dualrefine_ops --dr-pose-update --no-cpu-baseline --train-steps 0 2>/dev/null | tail -1 > $O/dr_ops_pose_update.json
python bench.py --full --mode dualrefine_ops --no-cpu-baseline --train-steps 0 2>/dev/null | tail -1 > $O/dr_ops.json
python - $O <<'PY'
import json,glob,os,sys
for f in sorted(glob.glob(os.path.join(sys.argv[1], 'dr*.json'))):
    d=json.loads(open(f).read())
    print(f.split('/')[-1], 'cold', round(d['ms_per_step'],4), 'warm', round(d.get('warm_ms_per_step',0),4))
PY
