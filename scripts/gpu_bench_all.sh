# Full bench line (bench.py --full) + rocprofv3 kernel stats over every bench
# leg (GPU box); written to $OUT, default bench_out/.
set -o pipefail
cd "$GRAFT_REPO_ROOT"
mkdir -p gpurun_out
export TMPDIR=/tmp PYTHONUNBUFFERED=1
TAG=${TAG:-v9}
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 600 python3 bench.py --full > "$OUT"/bench_$TAG.json 2> "$OUT"/bench_$TAG.err || { tail -20 "$OUT"/bench_$TAG.err; exit 1; }
echo "bench done"
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/prof_all_$TAG -o kt -- python3 bench.py --full --no-cpu-baseline > "$OUT"/prof_all_$TAG.json 2> "$OUT"/prof_all_$TAG.err || { tail -20 "$OUT"/prof_all_$TAG.err; exit 1; }
echo "rocprof done"
find "$OUT"/prof_all_$TAG -name "*stats.csv"
