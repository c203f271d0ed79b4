#!/bin/bash
# usage: tools/profile_round.sh <tag>   (on the GPU box) -> $OUT/<tag>/{stats,pmc,traffic}
TAG=$1; OUT=${OUT:-build/runs}; export TMPDIR=/tmp
mkdir -p $OUT/$TAG
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$TAG/stats -- python bench.py --full --steps 20 --warmup 1 --no-cpu-baseline > $OUT/$TAG/bench_stats.log 2>&1
tools/experiments/pmc.sh $TAG/pmc > /dev/null 2>&1
tools/traffic.sh $TAG/traffic > /dev/null 2>&1
tools/traffic.sh $TAG/traffic_c3 --config 3 > /dev/null 2>&1
tools/traffic.sh $TAG/traffic_c5 --config 5 > /dev/null 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$TAG/stats_c3 -- python bench.py --full --steps 8 --warmup 1 --no-cpu-baseline --config 3 > $OUT/$TAG/bench_stats_c3.log 2>&1
python bench.py --full --steps 10 --warmup 2 > $OUT/$TAG/bench.json 2> $OUT/$TAG/bench.err
python bench.py --full --steps 5 --warmup 2 --config 3 --no-cpu-baseline > $OUT/$TAG/bench_c3.json 2>> $OUT/$TAG/bench.err
python bench.py --full --steps 5 --warmup 2 --config 5 --no-cpu-baseline > $OUT/$TAG/bench_c5.json 2>> $OUT/$TAG/bench.err
python bench.py --full --steps 2 --warmup 1 --config 5 --passes 16 > $OUT/$TAG/bench_c5_progressive.json 2>> $OUT/$TAG/bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$TAG/stats_c5 -- python bench.py --full --steps 8 --warmup 1 --no-cpu-baseline --config 5 > $OUT/$TAG/bench_stats_c5.log 2>&1
ls $OUT/$TAG
