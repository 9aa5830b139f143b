#!/bin/bash
# rocprofv3 kernel-trace summary of the bench chain (run from the repo root on the GPU box): $1 = path (1 census, 2 streaming), $2 = tag
R=$PWD
O=${OUT:-$R/prof_out}  # where the logs and counter files go
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/prof_$2
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_$2 -- python3 $R/bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --path $1 ${@:3} > $O/prof_$2.log 2>&1
f=$(find /tmp/prof_$2 -name "*kernel_stats.csv" | head -1)
cp "$f" $O/prof_$2_kernel_stats.csv
tail -1 $O/prof_$2.log
