#!/bin/bash
# Multi-step bench lines (>= 8 timed steps, 2 warmup) of the BASELINE configs on one GPU, one run each:
#   TAG=r03a CONFIGS="cornell cfg3 cfg4 cfg5" bash scripts/gpu_bench_cfgs.sh
# Lines land in $OUT/bench_<config>_<TAG>.log; stops at the first failure.
export OUT=${OUT:-bench_out}  # where logs and profiles land (relative to the repository root)
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=/tmp
TAG=${TAG:-r03}
STEPS=${STEPS:-8}
mkdir -p "$OUT"
for c in ${CONFIGS:-cornell cfg3 cfg4 cfg5}; do
  timeout -k 10 400 python -u bench.py --full --config $c --steps $STEPS --warmup 2 --no-cpu-baseline \
    > $OUT/bench_${c}_$TAG.log 2>&1
  rc=$?; [ $rc -ne 0 ] && { echo "$c rc=$rc"; tail -5 $OUT/bench_${c}_$TAG.log; exit $rc; }
  python3 -c "
import json
d=json.loads([x for x in open('$OUT/bench_${c}_$TAG.log') if x.startswith('{')][-1])
print('$c', d['value'], d['ms_per_step'], d['stage_ms'])"
done
exit 0
