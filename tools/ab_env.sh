#!/bin/bash
# A/B of environment switches on ONE box: `bench.py --full --layers` once per setting, summary through tools/blayers.py.
#   tools/ab_env.sh <tag> <layer filter> VAR=a VAR=b VAR=c,OTHER=d ...   -> ${RESULTS_DIR:-results}/<tag>_<setting>.log/.err  (a setting may hold several VAR=value, comma-separated)
tag=$1; flt=$2; shift 2
out=${RESULTS_DIR:-results}
mkdir -p "$out" "$out/$(dirname "$tag")"
for kv in "$@"; do
  env ${kv//,/ } python3 bench.py --steps 20 --warmup 3 --repeats 3 --full --layers --no-cpu-baseline --no-secondary > "$out/${tag}_${kv}.log" 2> "$out/${tag}_${kv}.err" || { echo "FAILED $kv"; tail -5 "$out/${tag}_${kv}.err"; exit 1; }
  echo "== $kv"
  python3 tools/blayers.py "$out/${tag}_${kv}.log" "$out/${tag}_${kv}.err" "$flt"
done
