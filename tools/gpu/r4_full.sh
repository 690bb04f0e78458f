#!/bin/bash
export TMPDIR=/tmp
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
timeout 2400 python -m pytest tests -x -q -m gpu 2>&1 | tail -15
timeout 600 python bench.py --full --no-cpu-baseline --other-configs 0 > $OUT/bench_angle.json 2> $OUT/bench_angle.err
python - <<PY
import json
d=json.load(open('$OUT/bench_angle.json'))
print({k:d[k] for k in ('value','ms_per_step') if k in d}, d.get('eager_launches'), d.get('replayed_steps'))
PY
