# GPU tests + one bench line (+ config 2/4/5 when CONFIGS is set).  Outputs under $OUT/.
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 600 python3 -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/gputests.log 2>&1
timeout -k 10 400 python3 bench.py --full --steps 20 --warmup 5 > $OUT/bench.json 2> $OUT/bench.err
if [ -n "$CONFIGS" ]; then
timeout -k 10 400 python3 tools/configs_bench.py --configs $CONFIGS > $OUT/configs.json 2> $OUT/configs.err
fi
