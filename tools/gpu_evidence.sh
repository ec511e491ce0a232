# Round evidence at the current sources: every -m gpu test, smoke, the default
# bench line (C2 + CPU baseline + the reference's own workloads) and C1.
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:-build/evidence}  # where the lines and logs go
mkdir -p $OUT
tag=${1:-r03}
bash tools/gpu_tests.sh all_$tag tests || exit $?
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$tag.log 2>&1 || exit $?
cat $OUT/smoke_$tag.log
timeout -k 10 600 python -u bench.py --full > $OUT/bench_c2_$tag.json 2> $OUT/bench_c2_$tag.log || exit $?
cat $OUT/bench_c2_$tag.json
timeout -k 10 300 python -u bench.py --config c1 --ref-workloads 0 --no-cpu-baseline > $OUT/bench_c1_$tag.json 2> $OUT/bench_c1_$tag.log || exit $?
cat $OUT/bench_c1_$tag.json
