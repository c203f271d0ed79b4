#!/bin/bash
N=$1; shift; OUT=${OUT:-build/runs}; mkdir -p "$OUT/$(dirname "$N")"
export TMPDIR=/tmp
rocprofv3 --pmc SQ_IFETCH SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS SQ_INSTS_VALU_TRANS_F32 SQ_INST_CYCLES_SALU SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVE_CYCLES --kernel-trace --output-format csv -d $OUT/$N/c -- python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline "$@" > $OUT/$N.c.log 2>&1 &&
rocprofv3 --pmc SQ_INSTS_VALU_FMA_F32 SQ_INSTS_VALU_ADD_F32 SQ_INSTS_VALU_MUL_F32 SQ_INSTS_VALU_INT32 SQ_INSTS_VALU_CVT SQ_INSTS_VALU SQ_BUSY_CU_CYCLES SQ_INSTS_VSKIPPED --kernel-trace --output-format csv -d $OUT/$N/d -- python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline "$@" > $OUT/$N.d.log 2>&1
python tools/pmc_summary.py $OUT/$N/c $OUT/$N/d > $OUT/$N.summary2.txt; cat $OUT/$N.summary2.txt
