# A/B of library builds (build/variants/<name>, "default" = the in-tree library) on the lego bench,
# alternating over two rounds; outputs $OUT/<NAME>/bench_<name>_<round>.json (OUT: default bench_out).
# usage: bash tools/ab_libs.sh NAME default v1 ...
set -o pipefail
out=${OUT:-bench_out}/$1; shift
mkdir -p $out
for r in 1 2; do
  for v in "$@"; do
    if [ $v = default ]; then L=indoor-nerf_amd/libnerfhip.so; else L=build/variants/$v/libnerfhip.so; fi
    NERF_HIP_LIB=$L timeout -k 10 200 python bench.py --full --steps 40 --warmup 10 --no-cpu-baseline > $out/bench_${v}_$r.json 2> $out/bench_${v}_$r.err || exit 1
  done
done
