#!/bin/bash
# rocprofv3 --kernel-trace --stats of the full bench command (--full: every block); keeps our kernels' rows and the JSON line
# (in $OUT_DIR, default prof_out/).
#   usage: scripts/prof_r04.sh <tag> [bench args]
set -e
OUT_DIR=${OUT_DIR:-prof_out}
export TMPDIR=/tmp
T=${1:-r04_x}; shift || true
rm -rf /tmp/prof_r04; mkdir -p /tmp/prof_r04 $OUT_DIR
rocprofv3 --kernel-trace --stats -d /tmp/prof_r04 -o p --output-format csv -- python3 bench.py --full --no-cpu --no-dropin "$@" > $OUT_DIR/${T}_bench_line.json 2> /tmp/prof_r04/err.txt || { tail -5 /tmp/prof_r04/err.txt; exit 1; }
f=$(find /tmp/prof_r04 -name "*kernel_stats.csv" | head -1)
head -1 $f > $OUT_DIR/${T}_kernel_stats.csv; grep "ppm::" $f >> $OUT_DIR/${T}_kernel_stats.csv
cut -c1-130 $OUT_DIR/${T}_kernel_stats.csv | head -8
tail -1 $OUT_DIR/${T}_bench_line.json | cut -c1-3000
