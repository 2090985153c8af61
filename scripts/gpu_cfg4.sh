cd $GRAFT_REPO_ROOT
# logs and tables go under $OUT (default bench_out/, git-ignored)
export OUT=${OUT:-bench_out}; mkdir -p "$OUT"
export TMPDIR=/tmp
for K in 8 1; do
  timeout -k 10 400 python bench.py --full --workload cfg4 --virtual-shards $K --no-cpu --steps 2 --warmup 1 > $OUT/cfg4_k$K.log 2>&1 || { tail -20 $OUT/cfg4_k$K.log; exit 1; }
  tail -1 $OUT/cfg4_k$K.log | cut -c1-700
done
