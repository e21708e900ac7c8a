#!/bin/bash
# Jacobi threshold experiment: degenerate-spectrum probe, SVD / MPS GPU tests, bench, config 5.
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 200 python3 tools/probe_degenerate.py > $OUT/deg.txt 2>&1
timeout -k 10 400 python3 -u -m pytest tests/test_gpu_svd.py tests/test_gpu_mps.py tests/test_gpu_bigchi.py tests/test_gpu_headline.py -x -q --timeout 120 --timeout-method thread > $OUT/jtests.log 2>&1
timeout -k 10 300 python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-latency > $OUT/e_bench.json 2> $OUT/e_bench.err
timeout -k 10 300 python3 tools/configs_bench.py --configs 5 > $OUT/cfg5.json 2> $OUT/cfg5.err
