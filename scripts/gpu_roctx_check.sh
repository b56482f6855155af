export TMPDIR=/tmp
OUT=${OUT:-bench_out}  # where the logs and result lines go
cd "$(dirname "$0")/.." && mkdir -p $OUT && \
timeout -k 10 600 python -u -m pytest tests/test_gpu.py -m gpu -x -q --timeout 300 --timeout-method thread -k "coset_lde or proof_bytes_match or commit_root or mfma" > $OUT/pytest_ws_default.log 2>&1 && \
timeout -k 10 300 rocprofv3 --marker-trace --kernel-trace --stats -d /tmp/rtx -o run --output-format csv -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-extra --sustain-s 0 --solo-world 0 > $OUT/rtx_bench.json 2> $OUT/rtx_bench.err && \
find /tmp/rtx -name "*marker*" -o -name "*kernel_stats*" | tee $OUT/rtx_files.txt && \
cp $(find /tmp/rtx -name "*marker_api_trace.csv" | head -1) $OUT/rtx_marker_api_trace.csv && \
cp $(find /tmp/rtx -name "*kernel_stats.csv" | head -1) $OUT/rtx_kernel_stats.csv
rc=$?
tail -3 $OUT/pytest_ws_default.log
echo rc=$rc
exit $rc
