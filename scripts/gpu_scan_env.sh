#!/bin/bash
# C2 bench under a list of environment settings (SCAN="VAR=val VAR2=val;VAR=val ..."), one line each;
# logs go to $OUT (default bench_out/)
set -o pipefail
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
IFS=';' read -ra SETS <<< "$SCAN"
i=0
for s in "${SETS[@]}"; do
  i=$((i+1))
  # --full: the summary line below reads the roofline's launch time
  env $s timeout -k 10 300 python bench.py --full --steps ${STEPS:-5} --warmup ${WARM:-8} --no-cpu-baseline ${BENCH_ARGS} > "$OUT/scan_$i.log" 2>&1 || { echo "SCAN [$s] FAILED"; tail -5 "$OUT/scan_$i.log"; exit 1; }
  python3 -c "
import json,sys
d=json.loads(open('$OUT/scan_$i.log').read().strip().splitlines()[-1])
print('[$s]', d['value'], d['ms_per_step'], d['config']['fused_stream_wg'], d['roofline']['avg_launch_us'])"
done
