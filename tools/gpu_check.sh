#!/bin/bash
# GPU parity tests, then one default bench line (run via gpurun).
set -o pipefail
mkdir -p gpurun_out
export SHREWD_FI_JIT_CACHE=$PWD/gpurun_out/jitcache
timeout -k 10 500 python -u -m pytest tests -m gpu -x -v --timeout 200 --timeout-method thread > gpurun_out/pytest_gpu.log 2>&1; rc=$?
tail -5 gpurun_out/pytest_gpu.log
[ $rc -eq 0 ] || exit $rc
# the bench line goes to $BENCH_OUT (default build/bench, which git ignores)
B=${BENCH_OUT:-build/bench}
mkdir -p $B
timeout -k 10 400 python -u bench.py --full > $B/bench.json 2> $B/bench.err; rc=$?
cat $B/bench.json; tail -3 $B/bench.err
exit $rc
