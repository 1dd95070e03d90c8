#!/bin/bash
# Quick GPU perf probe: path-mode bench (no CPU baseline) + the GPU parity suite, stage times only.
export OUT=${OUT:-bench_out}  # where logs and profiles land (relative to the repository root)
cd "$(dirname "$0")/.." || exit 1
mkdir -p "$OUT"
timeout -k 10 600 python bench.py --full --steps ${BENCH_STEPS:-4} --warmup 1 --no-cpu-baseline ${BENCH_ARGS:-} > $OUT/quick.log 2>&1
rc=$?; echo "bench rc=$rc"; [ $rc -ne 0 ] && exit $rc
if [ -n "$WITH_TESTS" ]; then
  timeout -k 10 900 python -m pytest tests -m gpu -q > $OUT/pytest_gpu.log 2>&1
  rc=$?; echo "pytest rc=$rc"; tail -2 $OUT/pytest_gpu.log
fi
python3 - <<'PY'
import json, os
l=[x for x in open(os.environ['OUT'] + '/quick.log') if x.startswith('{')][-1]
d=json.loads(l)
print('VALUE', d['value'], 'ms/step', d['ms_per_step'], d['stage_ms'], 'roofline', d['roofline']['frac'])
PY
