O=${OUT_DIR:-bench_out}
mkdir -p $O
python bench.py --full --steps 5 --warmup 2 ${BENCH_ARGS:-} > $O/${1:-r03_bench}.json 2> $O/${1:-r03_bench}.err; echo rc=$?
tail -c 3000 $O/${1:-r03_bench}.json; tail -3 $O/${1:-r03_bench}.err
