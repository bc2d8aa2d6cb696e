# Round check: GPU parity tests, smoke, full bench line, kernel-trace profile.
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${VAEB_OUT:-out}   # logs and result lines go here
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests -x -v --timeout 120 --timeout-method thread -m gpu > $OUT/pytest.log 2>&1; rc=$?; echo "pytest rc=$rc" >> $OUT/pytest.log
tail -8 $OUT/pytest.log
if [ $rc -ne 0 ]; then exit 1; fi
timeout -k 10 120 python3 -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || exit 1
cat $OUT/smoke.log
timeout -k 10 240 python3 bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err || exit 1
cut -c1-1500 $OUT/bench_default.json
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run -- python3 bench.py --steps 1000 --warmup 100 --no-cpu-baseline > $OUT/bench_prof.json 2> $OUT/bench_prof.err || exit 1
cut -c1-160 $OUT/prof/run_kernel_stats.csv
