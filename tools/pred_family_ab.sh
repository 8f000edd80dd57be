#!/bin/bash
# A/B of the prediction kernels (profiles/pred_family_ab.log): every probe once per library, parent /
# new / parent / new, each run under its own time limit; the first failure ends the call.
# usage: tools/pred_family_ab.sh mc8 mc merge skip surface pi8 pi
#   PARENT: the parent commit's libfme_amd.so (default: variants/parent, as `make variant NAME=parent` builds it)
set -o pipefail
OUT=${OUT:-bench_out/pred_family_ab}
mkdir -p $OUT
export TMPDIR=/tmp CPU=0
PARENT=${PARENT:-$PWD/hm16.9-nn_fme_amd/variants/parent/libfme_amd.so}
NEW=$PWD/hm16.9-nn_fme_amd/libfme_amd.so
LOG=$OUT/ab.log
: > $LOG
run() {  # label, lib, command...
  local label=$1 lib=$2; shift 2
  echo "== $label: $*" | tee -a $LOG
  FME_LIB_PATH=$lib timeout -k 10 170 "$@" > $OUT/step.log 2>&1
  local rc=$?
  grep -v "amdgpu.ids" $OUT/step.log | sed "s/^/[$label] /" | tee -a $LOG | cut -c1-400
  if [ $rc -ne 0 ]; then echo "== $label FAILED rc=$rc" | tee -a $LOG; exit $rc; fi
}
for probe in "$@"; do
  case $probe in
    mc8) cmd="python tools/mc_probe.py" ;;
    surface) cmd="python tools/surface_probe.py" ;;
    pi8) cmd="python tools/pred_inter_probe.py" ;;
    *) cmd="python tools/pred_family_probe.py $probe" ;;
  esac
  for pass in 1 2; do
    run "parent $probe #$pass" $PARENT $cmd
    run "new    $probe #$pass" $NEW $cmd
  done
done
echo "== all done" | tee -a $LOG
