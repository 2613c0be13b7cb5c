set -e
OUT_DIR=${OUT_DIR:-prof_out}
export TMPDIR=/tmp
rm -rf /tmp/prof_rc /tmp/prof_rf; mkdir -p /tmp/prof_rc /tmp/prof_rf $OUT_DIR
T=${1:-r01_x}
rocprofv3 --kernel-trace --stats -d /tmp/prof_rc -o rc --output-format csv -- python3 bench.py --full --workload reconstruct --particles 100000 --steps 2 --warmup 1 > $OUT_DIR/${T}_reconstruct_line.json 2> /tmp/prof_rc/err.txt
f=$(find /tmp/prof_rc -name "*kernel_stats.csv" | head -1)
head -1 $f > $OUT_DIR/${T}_reconstruct_kernel_stats.csv; grep "ppm::" $f >> $OUT_DIR/${T}_reconstruct_kernel_stats.csv
cut -c1-110 $OUT_DIR/${T}_reconstruct_kernel_stats.csv | head -5
tail -1 $OUT_DIR/${T}_reconstruct_line.json | cut -c1-200
rocprofv3 --kernel-trace --stats -d /tmp/prof_rf -o rf --output-format csv -- python3 bench.py --full > $OUT_DIR/${T}_bench_line.json 2> /tmp/prof_rf/err.txt
f=$(find /tmp/prof_rf -name "*kernel_stats.csv" | head -1)
head -1 $f > $OUT_DIR/${T}_kernel_stats.csv; grep "ppm::" $f >> $OUT_DIR/${T}_kernel_stats.csv
cut -c1-110 $OUT_DIR/${T}_kernel_stats.csv | head -6
tail -1 $OUT_DIR/${T}_bench_line.json | cut -c1-1500
