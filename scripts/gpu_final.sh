#!/bin/bash
# Round-end rehearsal: whole GPU suite, smoke(), the headline bench (N = 1, driver
# defaults) and its kernel trace.
set -u
R=${GRAFT_REPO_ROOT:-$PWD}
OUT=${OMLDM_OUT:-$R/out}  # where this script leaves its records
mkdir -p $OUT
cd $R
export HSA_ENABLE_IPC_MODE_LEGACY=0
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/pytest_gpu.log 2>&1; rc=$?; tail -3 $OUT/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -20 $OUT/smoke.log; exit 3; }
tail -2 $OUT/smoke.log
timeout -k 10 300 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { tail -20 $OUT/bench.err; exit 4; }
cat $OUT/bench.json
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_bench
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_bench -o run -- python3 $R/bench.py --full --steps 100 --warmup 10 --latency-samples 100 > $OUT/prof_bench.log 2>&1 || { tail -20 $OUT/prof_bench.log; exit 5; }
cd $R && python scripts/trace_summary.py $OUT/prof_bench > $OUT/prof_bench_summary.txt && head -14 $OUT/prof_bench_summary.txt
