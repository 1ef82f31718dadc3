#!/bin/bash
# One GPU-box pass over the current build: the GPU test suite, the --full bench line and the bf16 share of configs[4] (eager).
#   bash tools/round_check.sh <tag>     -> ${RESULTS_DIR:-results}/<tag>_gputests.log, <tag>_bench.json, <tag>_cars_bf16.json
tag=${1:-check}
out=${RESULTS_DIR:-results}
mkdir -p "$out" "$out/$(dirname "$tag")"
timeout -k 10 900 python3 -m pytest tests -m gpu -x -q > "$out/${tag}_gputests.log" 2>&1; echo "pytest rc=$?" >> "$out/${tag}_gputests.log"
tail -4 "$out/${tag}_gputests.log"
timeout -k 10 400 python3 bench.py --steps 20 --full --no-cpu-baseline > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err"
timeout -k 10 200 python3 bench.py --gan cars --batch 4 --precision bf16 > "$out/${tag}_cars_bf16.json" 2>> "$out/${tag}_bench.err"
python3 - "$out" "$tag" <<'PY'
import json, sys
out, tag = sys.argv[1], sys.argv[2]
d = json.load(open("%s/%s_bench.json" % (out, tag)))
print("ffhq b8 fp32: %.1f pairs/s  runs %s  oracle %s" % (d["value"], d["runs"], d["output"]["matches_oracle"]))
print("secondary:", [(s["workload"][9:30], s["value"], s["graph"][:8]) for s in d["secondary"]], " generate job %.1f pairs/s" % d["end_to_end"]["generate_job_pairs_per_s"])
c = json.load(open("%s/%s_cars_bf16.json" % (out, tag)))
print("cars b4 bf16 eager: %.1f pairs/s  runs %s" % (c["value"], c["runs"]))
PY
