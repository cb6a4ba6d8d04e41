#!/bin/bash
# round-2 GPU box script: parity-band tests first (new), then the rest, then baseline benches.
TAG=${1:-r02a}
OUT=${OUT:-out}   # output folder, relative to the repository root
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
mkdir -p $ROOT/$OUT
cd $ROOT
python -m pytest tests/test_gpu_parity_band.py -q -m gpu -p no:cacheprovider -s 2>&1 | tail -40 > $OUT/band_$TAG.log
python -m pytest tests -q -m gpu -p no:cacheprovider --deselect tests/test_gpu_parity_band.py 2>&1 | tail -15 > $OUT/tests_$TAG.log
python bench.py --full --no-cpu > $OUT/bench_c2_$TAG.log 2>&1
python bench.py --full --config C3 --steps 5 --warmup 1 --no-cpu --no-full > $OUT/bench_c3_$TAG.log 2>&1
tail -30 $OUT/band_$TAG.log; tail -4 $OUT/tests_$TAG.log; tail -1 $OUT/bench_c2_$TAG.log; tail -1 $OUT/bench_c3_$TAG.log
