set -o pipefail
O=${OUT_DIR:-bench_out}
mkdir -p $O
python -m pytest tests -m gpu -x -q > $O/r03_t1_pytest.log 2>&1; echo "pytest rc=$?" | tee $O/r03_t1_rc.txt
tail -5 $O/r03_t1_pytest.log
for v in "" "CSTARK_LDE_BATCH_MB=0"; do
  echo "== $v" ; env $v python tools/bench_ntt.py 20
done 2>&1 | tee $O/r03_t1_ntt.txt
python bench.py --steps 5 --warmup 2 --full --no-cpu-baseline > $O/r03_t1_bench.json 2> $O/r03_t1_bench.err; tail -c 1500 $O/r03_t1_bench.json
CSTARK_LDE_BATCH_MB=0 python bench.py --steps 5 --warmup 2 --full --no-cpu-baseline > $O/r03_t1_bench_old.json 2>> $O/r03_t1_bench.err; tail -c 600 $O/r03_t1_bench_old.json
