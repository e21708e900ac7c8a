#!/bin/bash
# PMC passes over a short bench run (one rocprofv3 --pmc pass per counter group; gfx950 slot
# limits: 8 SQ, 4 TCC (FETCH_SIZE uses 3, WRITE_SIZE 2), 2 GRBM).  Summaries land in $OUT/
# (pmc_summary.txt, traffic.json); the databases (tens of MB each) are deleted.
# Usage (GPU box): bash tools/pmc_bench.sh [bench args...]
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
ARGS=${@:-"--steps 1 --warmup 0 --no-cpu-baseline --no-parity --no-latency"}
pass() {
  local k=$1; shift
  timeout -s KILL 180 rocprofv3 --pmc "$@" -d $OUT/pmc_$k -o run -- python3 bench.py $ARGS > $OUT/pmc_$k.log 2>&1
}
pass sq1 SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS
pass sq2 SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_WAIT_INST_LDS SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_LDS_BANK_CONFLICT GRBM_GUI_ACTIVE
pass mfma SQ_INSTS_VALU_MFMA_MOPS_F64 SQ_INSTS_VALU_MFMA_F64 SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE
pass fetch FETCH_SIZE
pass write WRITE_SIZE
python3 tools/pmc_summary.py $OUT/pmc_sq1 $OUT/pmc_sq2 $OUT/pmc_mfma $OUT/pmc_fetch $OUT/pmc_write > $OUT/pmc_summary.txt
python3 tools/pmc_traffic.py $OUT/pmc_fetch $OUT/pmc_write ${PMC_KERNEL:-k_chain} > $OUT/traffic.json
rm -rf $OUT/pmc_sq1 $OUT/pmc_sq2 $OUT/pmc_mfma $OUT/pmc_fetch $OUT/pmc_write
python3 tools/pmc_exec.py $OUT/pmc_summary.txt ${PMC_KERNEL:-k_chain} --units-per-dispatch ${PMC_UNITS:-15872} > $OUT/exec_k_chain.json
