#!/bin/bash
# A/B of the fused input-gradient + weight-gradient pass (csrc/gemm_dw.hip) inside the headline step, same box, alternating
cd "$GRAFT_REPO_ROOT" 2>/dev/null || true
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for i in 1 2; do
  for v in 1 0; do
    ALIGNN_AMD_DW_FUSED=$v timeout 400 python bench.py --full --no-cpu-baseline --no-micro --other-configs 0 --streamed-steps 0 --steps 20 > $OUT/r6_ab_dw_${v}_$i.json 2> $OUT/r6_ab_dw_${v}_$i.err
    python - <<PY
import json
d=json.load(open("$OUT/r6_ab_dw_${v}_$i.json"))
print("DW_FUSED=$v run $i:", d["step_launch"], d["ms_per_step"], "replay", (d.get("replayed_steps") or {}).get("ms_per_step"), "eager", (d.get("eager_launches") or {}).get("ms_per_step"))
r=d.get("roofline",{}).get("in_step") or {}
print("   ", {k:(v["launches"], v["ms_per_launch"]) for k,v in r.items() if isinstance(v,dict) and "launches" in v})
PY
  done
done
