#!/bin/bash
# k_octave investigation: kernel trace of a 1-step bench + PMC passes.
cd "$GRAFT_REPO_ROOT" || exit 2
OUT=${OUT:-bench_out}  # where the logs go
mkdir -p "$OUT"; export TMPDIR=/tmp
rm -rf $OUT/octtr
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/octtr -o run --output-format csv -- python3 bench.py --full --steps 1 --warmup 1 --frames 32 --no-cpu-baseline --no-latency > $OUT/octtr.log 2>&1 || exit 1
PMC_OUT=$OUT/pmcb bash tools/pmc_bench.sh k_octave 32 || exit 1
python3 tools/pmc_summary.py k_octave $OUT/pmcb/p*/*/*counter_collection.csv > $OUT/oct_pmc.txt 2>&1 || python3 tools/pmc_summary.py k_octave $(find $OUT/pmcb -name "*counter_collection.csv") > $OUT/oct_pmc.txt
cat $OUT/oct_pmc.txt
