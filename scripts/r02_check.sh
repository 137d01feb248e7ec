#!/bin/bash
# GPU check: gpu tests (one process), then the driver's exact bench command (with the
# secondary measurements: --full).  Logs go to $O (default bench_out/).
set -u
cd "$(dirname "$0")/.."
O=${O:-bench_out}
mkdir -p "$O"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread -p no:cacheprovider \
    > "$O/gpu_tests.log" 2>&1
rc=$?; echo "tests rc=$rc"; tail -n 5 "$O/gpu_tests.log"
[ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 --full > "$O/bench_driver.log" 2>&1
rc=$?; echo "bench rc=$rc"; tail -n 2 "$O/bench_driver.log"
exit $rc
