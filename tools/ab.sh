#!/bin/bash
# A/B runs of prebuilt library variants (tools/ab/lib*.so) in one box: tools/ab.sh "A B C" [rounds]
OUT=${OUT:-out}   # output folder, relative to the repository root
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd $ROOT; mkdir -p $OUT
cp sinddm_amd/libsinddm_hip.so /tmp/lib_keep.so
for r in $(seq 1 ${2:-2}); do for v in $1; do
  cp tools/ab/lib$v.so sinddm_amd/libsinddm_hip.so
  python bench.py --full --steps 10 --warmup 2 --no-cpu --no-full 2>&1 | tail -1 | python -c "
import sys, json
d = json.loads(sys.stdin.readline()); r = d['roofline']
print('$v', 'ms/step', d['ms_per_step'], 'conv TF/s', r['achieved'])"
done; done | tee $OUT/ab.log
cp /tmp/lib_keep.so sinddm_amd/libsinddm_hip.so
