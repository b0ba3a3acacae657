#!/bin/bash
# Interleaved bench runs per environment setting ("-" = none; settings joined by ","):
#   tools/env_sweep.sh REPS "- LDG_DEPTH=4 LDG_PROBE=1,LDG_DEPTH=4" BENCH-ARGS...
# (the runs' stderr goes to $OUT/env_sweep.err, default bench_outputs/)
set -e
REPS=$1; SETS=$2; shift 2
OUT=${OUT:-bench_outputs}
for i in $(seq 1 $REPS); do
  for e in $SETS; do
    envs=(); [ "$e" != "-" ] && IFS=, read -ra envs <<< "$e"
    mkdir -p $OUT
    out=$(env "${envs[@]}" timeout -k 10 600 python bench.py --full "$@" 2>>$OUT/env_sweep.err | tail -1)
    echo "$e $(python -c "import json,sys; d=json.loads(sys.argv[1]); c=d.get('checks', {}); i = c.get('demod_issue') or {}; print(d['value'], d['ms_per_step'], d['roofline']['avg_launch_ms'], c.get('reads_decoded'), c.get('vcut_redo'), 'host_late', i.get('host_late'), 'idle_ms', i.get('idle_ms'))" "$out")"
  done
done
