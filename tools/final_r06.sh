#!/bin/bash
# the last visit of round 6: the default line once more on the committed code (traffic quoted from profiles/r06_pmc_traffic.json), one rank over RCCL
cd "$(dirname "$0")/.."; OUT=${1:?usage: tools/final_r06.sh <output dir>}; mkdir -p "$OUT"
timeout 900 python bench.py --full 2> "$OUT/bench.err" > "$OUT/bench.json.log"
ANI_BENCH_FORCE_DIST=1 timeout 600 python bench.py --full --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline --no-e2e 2> "$OUT/dist1.err" > "$OUT/dist1.json.log"
python - "$OUT" <<'PY'
import json, sys
for f in ("bench", "dist1"):
    d = json.loads([l for l in open("%s/%s.json.log" % (sys.argv[1], f)) if l.startswith("{")][-1])
    r = d["roofline"]
    print(f, d["value"], d["ms_per_step"], d["stage_ms_per_step_rank0"], "frac", r["frac"], "traffic", r.get("traffic"), r.get("traffic_note"), "e2e", (d.get("end_to_end") or {}).get("seconds"), "parity", (d.get("parity_timed_rows") or {}).get("ok"))
    print({k: v.get("counter_traffic_ratio") for k, v in r["stages"].items()})
PY
