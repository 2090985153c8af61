# Parity of several library builds on chosen GPU tests, then a bench A/B of
# the ones that pass.  Usage: gpu_bisect.sh TAG "TESTS" lib1 lib2 ...
cd $GRAFT_REPO_ROOT
# logs and tables go under $OUT (default bench_out/, git-ignored)
export OUT=${OUT:-bench_out}; mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=$1; TESTS=$2; shift 2
ok=""
for lib in "$@"; do
  GK_LIB_PATH=sketches-py_amd/gkarray_amd/$lib timeout -k 10 300 python -u -m pytest $TESTS -q --timeout 120 --timeout-method thread > $OUT/${TAG}_${lib}.log 2>&1
  rc=$?
  echo "$lib tests rc=$rc: $(tail -1 $OUT/${TAG}_${lib}.log)" | tee -a $OUT/${TAG}_ab.txt
  if [ $rc -eq 0 ]; then ok="$ok $lib"; fi
  if [ $rc -gt 1 ]; then echo "abort (rc $rc)"; exit 1; fi
done
for rep in 1 2; do
  for lib in libgkarray_hip_r03.so $ok; do
    GK_LIB_PATH=sketches-py_amd/gkarray_amd/$lib timeout -k 10 200 python bench.py --full --no-cpu --steps 10 --warmup 3 > $OUT/${TAG}_ab.tmp 2>&1 || { echo "FAILED: $lib"; tail -20 $OUT/${TAG}_ab.tmp; exit 1; }
    python3 -c "import json,sys; d=json.loads(open('$OUT/${TAG}_ab.tmp').read().strip().splitlines()[-1]); print('%-32s %7.2f Gv/s  ms/step %.3f  launch_ms %.3f  frac %.3f' % (sys.argv[1], d['value']/1e9, d['ms_per_step'], d['roofline']['launch_ms'], d['roofline']['frac']))" "$lib" | tee -a $OUT/${TAG}_ab.txt
  done
done
