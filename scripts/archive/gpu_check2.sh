#!/bin/bash
# Diagnostic + all GPU tests without -x, smoke, bench, kernel-trace profile.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p ${OUT:-bench_out}
export TMPDIR=/tmp
timeout -k 10 120 python -u scripts/diag_stats.py > ${OUT:-bench_out}/diag_stats.log 2>&1 &&
timeout -k 10 900 python -u -m pytest tests -m gpu -v --timeout 120 --timeout-method thread > ${OUT:-bench_out}/pytest_gpu.log 2>&1
rc=$?
case $rc in 0|1) ;; *) echo "exit $rc"; exit $rc;; esac
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > ${OUT:-bench_out}/smoke.log 2>&1 &&
timeout -k 10 600 python bench.py --full --steps 10 --warmup 2 > $TMPDIR/bench_full.log 2>&1 &&
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d ${OUT:-bench_out}/prof -o run --output-format csv -- python3 bench.py --full --steps 5 --warmup 1 --no-cpu-baseline > ${OUT:-bench_out}/prof.log 2>&1
rc2=$?
echo "pytest $rc rest $rc2"
exit $rc2
