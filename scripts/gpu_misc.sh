#!/bin/bash
# Tracking parity tests + a short tracking bench, then the N=2 bench path rehearsed on one GPU (gloo).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
mkdir -p gpurun_out
timeout -k 10 400 python -u -m pytest tests/test_gpu_matching.py tests/test_gpu_tracking.py tests/test_gpu_configs.py -m gpu -q -p no:cacheprovider --timeout 200 --timeout-method thread > gpurun_out/track_tests.log 2>&1
rc=$?; echo "TRACK_TESTS_RC=$rc"; tail -3 gpurun_out/track_tests.log; [ $rc -eq 0 ] || exit $rc
# Both benches go through gpu_bench.sh, which runs `bench.py --full` with the selectors given here (kernels_us and
# the ba legs need --full), prints each run's whole JSON line and stderr tail, and keeps the last run's as
# bench.json / bench.err beside the test log.
STEPS=200 bash scripts/gpu_bench.sh --warmup 20 --no-cpu --no-ba --no-peaks --no-retrieval || exit $?
# N = 2 on one GPU: bench.py's own launcher starts the two ranks (both on device 0, gloo); the ba legs shard over them
M3S_BENCH_DEVICE=0 M3S_DIST_BACKEND=gloo STEPS=50 bash scripts/gpu_bench.sh --gpus 2 --warmup 5 --no-cpu
