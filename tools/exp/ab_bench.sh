#!/bin/bash
# A/B of env variants on the default bench (no configs / cpu baseline) and the
# single-frame probe.  usage: bash tools/exp/ab_bench.sh "TAG1:ENV=.. ENV2=..[|bench args]" "TAG2:..." ...
cd "$GRAFT_REPO_ROOT" || exit 2
OUT=${OUT:-bench_out}  # where the logs go
mkdir -p $OUT/ab
for spec in "$@"; do
  tag=${spec%%:*}; rest=${spec#*:}; envs=${rest%%|*}; args=""
  [[ $rest == *"|"* ]] && args=${rest#*|}
  env $envs timeout -k 10 200 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-configs $args > $OUT/ab/$tag.log 2>&1 || { echo "$tag bench failed"; exit 1; }
  [ -n "$NO_SINGLE" ] && continue
  env $envs TAG=$tag timeout -k 10 120 python tools/exp/single.py >> $OUT/ab/single.log 2>&1 || { echo "$tag single failed"; exit 1; }
done
python3 tools/exp/bench_cmp.py $OUT/ab/*.log
[ -f $OUT/ab/single.log ] && cat $OUT/ab/single.log
exit 0
