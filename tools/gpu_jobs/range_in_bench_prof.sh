O=${OUT_DIR:-bench_out}
mkdir -p $O
CSTARK_RB_PROF=1 python bench.py --steps 2 --warmup 1 --full --no-cpu-baseline > $O/rb_in_bench.json 2> $O/rb_in_bench.err; echo rc=$?
grep "cstark range batch" $O/rb_in_bench.err | sed -n 80,104p
