#!/bin/bash
# Collects PMC counters for the bench in separate passes (run on the GPU box).
#   tools/pmc.sh [outdir under ${RESULTS_DIR:-results}/] [extra bench.py arguments...]
set -o pipefail
out=${1:-pmc}; shift
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
dir=${RESULTS_DIR:-results}/$out
mkdir -p $dir
# --full: tools/pmc_report.py keeps the last of the 5 steps (warm-up 1, 2 timed, 2 of the roofline pass)
run() { name=$1; shift; GSA_SIDE_LEVELS=0 timeout -k 10 280 rocprofv3 --pmc "$@" --kernel-trace --output-format csv -d $dir -o $name -- python bench.py --steps 2 --warmup 1 --settle-steps 0 --repeats 1 --full --no-cpu-baseline --no-secondary $EXTRA > $dir/$name.json 2> $dir/$name.err; echo "$name rc=$?"; }
EXTRA="$*"
run sq1 SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT GRBM_GUI_ACTIVE &&
run fetch FETCH_SIZE &&
run write WRITE_SIZE
ls $dir | head -20
