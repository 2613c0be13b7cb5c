set -e
OUT_DIR=${OUT_DIR:-prof_out}
export TMPDIR=/tmp
rm -rf /tmp/prof_rc; mkdir -p /tmp/prof_rc $OUT_DIR
rocprofv3 --kernel-trace --stats -d /tmp/prof_rc -o rc --output-format csv -- python3 bench.py --full --workload reconstruct --particles 100000 --steps 2 --warmup 1 > $OUT_DIR/r01_bricks_reconstruct_line.json 2> /tmp/prof_rc/err.txt
f=$(find /tmp/prof_rc -name "*kernel_stats.csv" | head -1)
head -1 $f > $OUT_DIR/r01_bricks_reconstruct_kernel_stats.csv; grep "ppm::" $f >> $OUT_DIR/r01_bricks_reconstruct_kernel_stats.csv
cat $OUT_DIR/r01_bricks_reconstruct_kernel_stats.csv | cut -c1-150
tail -1 $OUT_DIR/r01_bricks_reconstruct_line.json | cut -c1-300
