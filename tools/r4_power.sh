#!/bin/bash
# socket power / clocks sampled while the C3 bench loop runs: is the dominant kernel power-limited?
OUT=${OUT:-out}   # output folder, relative to the repository root
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd $ROOT; mkdir -p $OUT
(python bench.py --full --steps 150 --warmup 2 --no-cpu --no-full > $OUT/power_bench.log 2>&1 &)
for i in $(seq 1 70); do rocm-smi --showpower --showclocks 2>&1 | grep -i "power (W)\|sclk" | sed 's/.*: //' | tr '\n' ' '; echo; sleep 0.3; done | uniq -c
wait
tail -n 1 $OUT/power_bench.log | cut -c1-200
