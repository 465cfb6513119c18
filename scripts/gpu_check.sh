#!/bin/bash
# GPU check: the whole -m gpu suite, then the bench line with everything in it (--full).
# Usage: bash scripts/gpu_check.sh <tag>
tag=${1:-check}
out=${OUT:-out}/$tag  # results folder: OUT (default ./out) / tag
mkdir -p $out
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -s > $out/tests.log 2>&1
rc=$?
echo "TESTS EXIT $rc" >> $out/tests.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python -u bench.py --full > $out/bench.log 2>&1
