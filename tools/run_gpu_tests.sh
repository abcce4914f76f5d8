#!/bin/bash
# GPU box: every GPU test file in its own process, each under its own time limit. A file whose tests merely fail does not stop the
# run; a GPU fault, an abort, a segmentation fault or a time limit does: nothing more is started on a card after that.
# usage: tools/run_gpu_tests.sh <outdir> [pytest args]
OUT=${1:-gpurun_out/tests}; shift || true
mkdir -p $OUT
rc=0
for f in tests/test_gpu_*.py; do
  n=$(basename $f .py)
  timeout -k 10 900 python -m pytest $f -m gpu -q -x "$@" > $OUT/$n.log 2>&1
  c=$?
  echo "$n exit $c: $(grep -E 'passed|failed|error' $OUT/$n.log | tail -1)"
  [ $c -ne 0 ] && rc=1
  if [ $c -eq 124 ] || [ $c -eq 137 ] || [ $c -eq 134 ] || [ $c -eq 139 ] || grep -q -E 'illegal memory access|Memory access fault|HSA_STATUS_ERROR' $OUT/$n.log; then
    echo "STOPPED at $n (exit $c): fault, abort or time limit - see $OUT/$n.log"
    exit 2
  fi
done
exit $rc
