# bench + rocprofv3 kernel-trace summary (run on the GPU box from the repo root)
export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}  # where the logs and result lines go
mkdir -p $OUT
timeout -k 10 900 python bench.py --full ${BENCH_ARGS} > $OUT/bench.json 2> $OUT/bench.err && \
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extra --sustain-s 0 > $OUT/prof.log 2>&1
echo "exit $?"
