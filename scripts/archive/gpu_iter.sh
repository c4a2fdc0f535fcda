#!/bin/bash
# Iteration call: all GPU parity tests, a short bench, a 2-rank gloo rehearsal of the N > 1 path on the one GPU,
# and a rocprofv3 kernel-trace summary.  Every GPU step has its own time limit; the first failure ends the call.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p ${OUT:-bench_out}
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > ${OUT:-bench_out}/pytest_gpu.log 2>&1 &&
timeout -k 10 300 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline > ${OUT:-bench_out}/bench.log 2>&1 &&
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29511 bench.py --gpus 2 --steps 5 --warmup 1 --dist-backend gloo > ${OUT:-bench_out}/bench_gloo2.log 2>&1 &&
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d ${OUT:-bench_out}/prof -o run --output-format csv -- python3 bench.py --full --steps 5 --warmup 1 --no-cpu-baseline > ${OUT:-bench_out}/prof.log 2>&1
rc=$?
echo "exit $rc"
exit $rc
