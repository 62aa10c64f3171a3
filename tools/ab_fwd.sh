# A/B of library builds (build/variants/<name>) on the lego bench: per-kernel times per build,
# then the hash parity tests against each build named in PARITY. Usage: bash tools/ab_fwd.sh NAME v1 v2 ...
# (outputs under $OUT/NAME, OUT: default bench_out)
set -o pipefail
out=${OUT:-bench_out}/$1; shift
mkdir -p $out
for v in "$@"; do
  L=build/variants/$v/libnerfhip.so
  NERF_HIP_LIB=$L timeout -k 10 200 python bench.py --full --steps 30 --warmup 10 --no-cpu-baseline > $out/bench_$v.json 2> $out/bench_$v.err || exit 1
done
for v in $PARITY; do
  NERF_HIP_LIB=build/variants/$v/libnerfhip.so timeout -k 10 400 python -u -m pytest tests/test_gpu_parity.py -x -v --timeout 200 --timeout-method thread -k "hash or train_step or render" > $out/parity_$v.log 2>&1 || exit 2
done
