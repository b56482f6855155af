#!/bin/bash
# Constraint-checker timing on the GPU box: wall times against a proof (debug_constraints_time.py),
# then the same program under rocprofv3 --kernel-trace --stats for the k_check / k_lookup_balance
# kernel times (a run of its own: tracing slows the host).  Results under $OUT (bench_out/).
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 240 python3 scripts/debug_constraints_time.py --reps 5 > $OUT/debug_constraints_time.json 2> $OUT/debug_constraints_time.err && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/debug_constraints_kt -o run -- \
  python3 scripts/debug_constraints_time.py --reps 2 > $OUT/debug_constraints_kt.json 2> $OUT/debug_constraints_kt.err && \
grep -h -E 'k_check|k_lookup_balance|k_balance_reduce|k_quotient|k_perm_rows' $OUT/debug_constraints_kt/*/*kernel_stats.csv $OUT/debug_constraints_kt/*kernel_stats.csv 2>/dev/null > $OUT/debug_constraints_kernels.csv
cat $OUT/debug_constraints_time.json
