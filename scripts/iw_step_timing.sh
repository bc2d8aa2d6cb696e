# DESIGN 4.3.2 measurements: the ELBO step of an earlier build (vaeb_amd/libvaeb_hip_<variant>.so,
# VAEB_LIB_VARIANT) against this build's, binary and cont, and this build's importance-weighted
# step at K = 5 and K = 50; one process per build and line, alternating, AB_ROUNDS rounds.
#   usage: scripts/iw_step_timing.sh <variant>      (lines go to $VAEB_OUT/iw_step_timing.txt)
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${VAEB_OUT:-out}
mkdir -p $OUT
V=${1:?variant name of the earlier build}
run() { timeout -k 10 120 python3 scripts/iw_step_timing.py "$@" | tee -a $OUT/iw_step_timing.txt; }
: > $OUT/iw_step_timing.txt
for r in $(seq ${AB_ROUNDS:-2}); do
  for ot in binary cont; do
    VAEB_LIB_VARIANT=$V run --otype $ot || exit 1
    run --otype $ot || exit 1
  done
  run --iw 5 || exit 1
  run --iw 50 || exit 1
done
