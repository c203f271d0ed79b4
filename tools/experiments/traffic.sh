#!/bin/bash
# HBM-side traffic of one bench step (separate PMC passes: FETCH_SIZE uses 3 of 4 TCC slots, WRITE_SIZE 2)
N=$1; shift; OUT=${OUT:-build/runs}; mkdir -p "$OUT/$(dirname "$N")"
export TMPDIR=/tmp
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/$N/f -- python bench.py --full --steps 1 --warmup 2 --no-cpu-baseline "$@" > $OUT/$N.f.log 2>&1 &&
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/$N/w -- python bench.py --full --steps 1 --warmup 2 --no-cpu-baseline "$@" > $OUT/$N.w.log 2>&1 &&
rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --kernel-trace --output-format csv -d $OUT/$N/h -- python bench.py --full --steps 1 --warmup 2 --no-cpu-baseline "$@" > $OUT/$N.h.log 2>&1
python tools/pmc_summary.py $OUT/$N/f $OUT/$N/w $OUT/$N/h > $OUT/$N.summary.txt; cat $OUT/$N.summary.txt
