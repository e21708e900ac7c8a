#!/bin/bash
# Round profiling on the GPU box: the GPU tests, rocprofv3 kernel-trace stats of a bench run, the
# PMC passes (tools/pmc_bench.sh), a full bench line, and the other BASELINE configs with their
# kernel stats.  Each step has its own time limit; the chain stops at the first failure.  Outputs
# under $OUT/ (copy the ones to keep into profiles/).
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
if [ -z "$SKIP_TESTS" ]; then
  timeout -k 10 600 python3 -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/gputests.log 2>&1
fi
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/ktrace -o run -- python3 bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-parity --no-latency > $OUT/ktrace_bench.json 2> $OUT/ktrace.err
python3 tools/rocpd_stats.py $OUT/ktrace/run_results.db > $OUT/kernel_stats.csv
rm -rf $OUT/ktrace
timeout -k 10 900 bash tools/pmc_bench.sh
# the full bench line below reads this round's PMC results (copied back from $OUT/ locally)
cp $OUT/exec_k_chain.json profiles/${ROUND:-r3}_exec_k_chain.json
cp $OUT/traffic.json profiles/${ROUND:-r3}_traffic.json
timeout -k 10 400 python3 bench.py --full --steps 20 --warmup 5 > $OUT/bench.json 2> $OUT/bench.err
if [ -z "$SKIP_CONFIGS" ]; then
  timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/kcfg -o run -- python3 tools/configs_bench.py --configs 2,4,5 > $OUT/configs.json 2> $OUT/configs.err
  python3 tools/rocpd_stats.py $OUT/kcfg/run_results.db > $OUT/configs_kernel_stats.csv
  rm -rf $OUT/kcfg
fi
