#!/bin/bash
# Round-end evidence in one call: smoke + every GPU test, the default bench line, then the profiles
# (gpu_prof_round.sh: kernel-trace stats + PMC passes of the tracking bench and of the C5 BA loop).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
mkdir -p gpurun_out
bash scripts/gpu_check.sh || exit $?
# every leg of the benchmark at its default 100 steps: gpu_bench.sh runs `bench.py --full`, keeps the line and
# its stderr as bench.json / bench.err beside this script's other records, and prints both
STEPS=100 bash scripts/gpu_bench.sh || exit $?
TAG=${TAG:-r03} bash scripts/gpu_prof_round.sh
