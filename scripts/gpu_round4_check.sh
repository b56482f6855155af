# Round-4 check on the GPU box (repo root): selected parity tests, the NTT counter passes, a
# short bench and a kernel trace of back-to-back proofs (idle time per proof).
export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}  # where the logs and result lines go
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -k "${PYTEST_K:-divergence or proof_bytes_match or coset_lde or record_from or open}" > $OUT/pytest_check.log 2>&1 && \
bash scripts/gpu_ntt_counters.sh > $OUT/ntt_counters.out 2>&1 && \
timeout -k 10 300 python -u bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-extra --sustain-s 2 --solo-world 0 > $OUT/bench_check.json 2> $OUT/bench_check.err && \
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/kt -o run \
  -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-extra --sustain-s 0 --solo-world 0 > $OUT/kt.log 2>&1 && \
python3 scripts/timeline.py $OUT/kt/run_kernel_trace.csv > $OUT/timeline.txt
rc=$?
echo "exit $rc"
tail -3 $OUT/pytest_check.log
exit $rc
