#!/bin/bash
# One gpurun call: GPU parity tests, smoke, a short bench and a rocprofv3 kernel-trace summary.
# Every GPU step has its own time limit; steps are chained so the first failure ends the call.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p ${OUT:-bench_out}
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > ${OUT:-bench_out}/pytest_gpu.log 2>&1 &&
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > ${OUT:-bench_out}/smoke.log 2>&1 &&
timeout -k 10 600 python bench.py --full --steps 10 --warmup 2 > $TMPDIR/bench_full.log 2>&1 &&
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d ${OUT:-bench_out}/prof -o run --output-format csv -- python3 bench.py --full --steps 5 --warmup 1 --no-cpu-baseline > ${OUT:-bench_out}/prof.log 2>&1
rc=$?
echo "exit $rc"
exit $rc
