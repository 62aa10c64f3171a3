# full GPU suite, then the workload bench lines (outputs under $OUT, default bench_out/)
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || exit 1
timeout -k 10 700 python -u bench.py --full > $OUT/bench.json 2> $OUT/bench.err || exit 2
for wl in ${WORKLOADS:-fern acaq scannet}; do
  timeout -k 10 200 python -u bench.py --full --workload $wl --no-cpu-baseline > $OUT/bench_${wl}.json 2> $OUT/bench_${wl}.err || exit 3
done
