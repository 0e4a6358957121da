#!/bin/bash
# One GPU round: parity tests, PMC passes of the dominant kernels, bench (reading that PMC
# summary for roofline.traffic), rocprofv3 kernel-trace stats of the same bench command.
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
TAG=${1:-run}
STEPS=${STEPS:-1000}
export OUT=${OUT:-$R/results}   # where the logs, profiles and bench lines go (scripts/pmc_z.sh too)
mkdir -p $OUT
cd $R
timeout -k 10 600 python -u -m pytest tests -x -q -m gpu --timeout 300 --timeout-method thread > $OUT/${TAG}_pytest.log 2>&1 || { echo "pytest failed"; tail -40 $OUT/${TAG}_pytest.log; exit 1; }
tail -2 $OUT/${TAG}_pytest.log
bash scripts/pmc_z.sh ${TAG}_pmc "z_wave|eta_fused|beta_lambda|gammav_wave" || exit 1
python scripts/pmc_summary.py $OUT/${TAG}_pmc > $OUT/${TAG}_pmc.json || exit 1
timeout -k 10 600 python bench.py --full --steps $STEPS --warmup 100 --pmc-json $OUT/${TAG}_pmc.json > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { echo "bench failed"; tail -20 $OUT/${TAG}_bench.err; exit 1; }
cat $OUT/${TAG}_bench.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o run -- python $R/bench.py --full --steps $STEPS --warmup 100 --no-cpu --pmc-json $OUT/${TAG}_pmc.json > $OUT/${TAG}_prof_bench.json 2> $OUT/${TAG}_prof.err || { echo "rocprof failed"; tail -20 $OUT/${TAG}_prof.err; exit 1; }
cat $OUT/${TAG}_prof_bench.json
echo done
