#!/bin/bash
# A/B of ablation builds (results are wrong: finiteness check off): tools/ab_abl.sh "BASE X Y" [rounds]
OUT=${OUT:-out}   # output folder, relative to the repository root
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd $ROOT; mkdir -p $OUT
cp sinddm_amd/libsinddm_hip.so /tmp/lib_keep.so
for r in $(seq 1 ${2:-1}); do for v in $1; do
  cp tools/ab/lib$v.so sinddm_amd/libsinddm_hip.so
  SINDDM_BENCH_NOFINITE=1 python bench.py --full --steps 10 --warmup 2 --no-cpu --no-full --no-train --no-strong 2>&1 | tail -1 | python -c "
import sys, json
d = json.loads(sys.stdin.readline()); r = d['roofline']
print('$v', 'C3 ms/step', d['ms_per_step'], 'conv launch ms', r['avg_launch_ms'], 'W', r['power']['socket_w'], 'MHz', r['power']['sclk_mhz'], '| C2 ms/step', d['c2']['ms_per_step'])"
done; done | tee $OUT/ab_abl.log
cp /tmp/lib_keep.so sinddm_amd/libsinddm_hip.so
