# The benchmark's full run (every leg) and its two-rank rehearsal over gloo; lines and logs under $OUT.
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 python3 bench.py --full > $OUT/bench_full.json 2> $OUT/bench_full.err
r=$?; echo "bench full rc=$r"; tail -c 600 $OUT/bench_full.err; [ $r -eq 0 ] || exit $r
BCOSGPU_BENCH_BACKEND=gloo timeout -k 10 300 python3 bench.py --full --gpus 2 --steps 300 --no-merkle --no-cpu-baseline > $OUT/bench_gloo2.json 2> $OUT/bench_gloo2.err
r=$?; echo "bench gloo2 rc=$r"; tail -c 600 $OUT/bench_gloo2.err; exit $r
