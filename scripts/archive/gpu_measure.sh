#!/bin/bash
# Round measurement: GPU tests, smoke, the default bench (matrix + reference CPU baseline), a kernel-trace profile of
# the headline configuration, and the PMC traffic passes (scripts/pmc_traffic.sh).  Logs under ${OUT:-bench_out}/.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p ${OUT:-bench_out}
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > ${OUT:-bench_out}/pytest_gpu.log 2>&1 || { tail -5 ${OUT:-bench_out}/pytest_gpu.log; exit 1; }
tail -1 ${OUT:-bench_out}/pytest_gpu.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > ${OUT:-bench_out}/smoke.log 2>&1 || exit $?
timeout -k 10 600 python bench.py --full > $TMPDIR/bench_full.log 2>&1 || { tail -5 $TMPDIR/bench_full.log; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d ${OUT:-bench_out}/prof -o run --output-format csv -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-matrix > ${OUT:-bench_out}/prof.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d ${OUT:-bench_out}/prof1 -o run --output-format csv -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-matrix --frames-in-flight 1 > ${OUT:-bench_out}/prof1.log 2>&1 || exit $?
bash scripts/pmc_traffic.sh
