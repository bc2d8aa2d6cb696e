# Quick GPU iteration: parity tests, plain bench, in-kernel timeline.
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${VAEB_OUT:-out}   # logs and result lines go here
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 400 python -m pytest tests/test_gpu_step.py tests/test_gpu_api.py -q -m gpu -x > $OUT/pytest.log 2>&1; rc=$?; echo "pytest rc=$rc" >> $OUT/pytest.log
tail -6 $OUT/pytest.log
if grep -q -E "illegal memory|core dumped|Aborted|HSA_STATUS|Memory access fault" $OUT/pytest.log; then echo "GPU fault: stopping"; exit 1; fi
timeout -k 10 120 python3 bench.py --full --steps 2000 --warmup 200 --no-cpu-baseline > $OUT/bench_plain.json 2> $OUT/bench_plain.err || exit 1
cut -c1-200 $OUT/bench_plain.json; python3 -c "import json;d=json.load(open('$OUT/bench_plain.json'));print(d['kernels_ms'])"
timeout -k 10 120 python3 scripts/gpu_timeline.py > $OUT/timeline.txt 2>&1
tail -16 $OUT/timeline.txt
