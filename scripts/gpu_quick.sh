# Focused GPU check: named tests first, then the whole GPU suite, then the
# lean-relay timing and a 1-GPU bench line with every leg but the CPU baseline
# (bench.py --full; written to $OUT, default bench_out/).
set -o pipefail
cd "$GRAFT_REPO_ROOT"
mkdir -p gpurun_out
export TMPDIR=/tmp PYTHONUNBUFFERED=1
TAG=${TAG:-q}
if [ -n "$FIRST_TESTS" ]; then
timeout -k 10 300 python -u -m pytest $FIRST_TESTS -m gpu -x -v -p no:cacheprovider --timeout 120 --timeout-method thread > gpurun_out/pytest_first_$TAG.log 2>&1 || { tail -60 gpurun_out/pytest_first_$TAG.log; exit 1; }
tail -3 gpurun_out/pytest_first_$TAG.log
fi
if [ -z "$SKIP_SUITE" ]; then
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 300 --timeout-method thread > gpurun_out/pytest_gpu_$TAG.log 2>&1 || { tail -40 gpurun_out/pytest_gpu_$TAG.log; exit 1; }
tail -2 gpurun_out/pytest_gpu_$TAG.log
fi
if [ -n "$EXTRA" ]; then
timeout -k 10 600 bash -c "$EXTRA" > gpurun_out/extra_$TAG.txt 2>&1 || { tail -30 gpurun_out/extra_$TAG.txt; exit 1; }
tail -40 gpurun_out/extra_$TAG.txt
fi
if [ -z "$SKIP_BENCH" ]; then
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 400 python -u bench.py ${BENCH_ARGS:---full --steps 20 --warmup 5 --no-cpu-baseline} > "$OUT"/bench_$TAG.json 2> "$OUT"/bench_$TAG.err || { tail -30 "$OUT"/bench_$TAG.err; exit 1; }
cat "$OUT"/bench_$TAG.json
fi
