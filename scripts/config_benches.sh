#!/bin/bash
# Config 3 / config 5 bench lines with their CPU baselines (numpy restatement), into $OUT/cfg.
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${OUT:-$R/results}
mkdir -p $OUT/cfg
cd $R
timeout -k 10 300 python -u bench.py --full --workload phylo --steps 200 --warmup 50 > $OUT/cfg/config3.json 2> $OUT/cfg/config3.err || { echo "config3 failed"; tail -5 $OUT/cfg/config3.err; exit 1; }
for m in GPP NNGP Full; do
  timeout -k 10 600 python -u bench.py --full --workload spatial --method $m --steps 200 --warmup 50 > $OUT/cfg/config5_$m.json 2> $OUT/cfg/config5_$m.err || { echo "config5 $m failed"; tail -5 $OUT/cfg/config5_$m.err; exit 1; }
done
echo configs done
