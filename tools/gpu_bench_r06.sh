# Round-6 evidence: the default bench line (C2 + CPU baseline + the
# reference's own workloads), C1 with its CPU baseline (VERDICT r05 Next 7),
# C0 (Voronoi), and smoke.
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:-build/evidence}  # where the lines and logs go
mkdir -p $OUT
tag=${1:-r06}
timeout -k 10 600 python -u bench.py --full > $OUT/bench_c2_$tag.json 2> $OUT/bench_c2_$tag.log || exit $?
cat $OUT/bench_c2_$tag.json
timeout -k 10 400 python -u bench.py --full --config c1 --ref-workloads 0 > $OUT/bench_c1_$tag.json 2> $OUT/bench_c1_$tag.log || exit $?
cat $OUT/bench_c1_$tag.json
timeout -k 10 300 python -u bench.py --full --config c0 --ref-workloads 0 > $OUT/bench_c0_$tag.json 2> $OUT/bench_c0_$tag.log || exit $?
cat $OUT/bench_c0_$tag.json
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$tag.log 2>&1 || exit $?
cat $OUT/smoke_$tag.log
