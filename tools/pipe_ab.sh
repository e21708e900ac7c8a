set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 300 python3 -u -m pytest tests/test_gpu_headline.py tests/test_gpu_mps.py -x -q --timeout 120 --timeout-method thread > $OUT/pipe_tests.log 2>&1
timeout -k 10 300 python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-latency > $OUT/bench_pipe.json 2> $OUT/bench_pipe.err
timeout -k 10 300 python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-latency --no-pipeline > $OUT/bench_nopipe.json 2> $OUT/bench_nopipe.err
