#!/bin/bash
# One GPU-box round: parity tests, smoke, benchmark, rocprofv3 kernel stats.  Run as
#   bash tools/gpu_round.sh <tag>
# Outputs land in $OUT/; copy what should be judged into profiles/.
TAG=${1:-r}
OUT=${OUT:-out}   # output folder, relative to the repository root
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
mkdir -p $ROOT/$OUT
cd $ROOT
python -m pytest tests -q -m gpu -p no:cacheprovider 2>&1 | tail -15 > $OUT/tests_$TAG.log
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1
python bench.py --full > $OUT/bench_$TAG.log 2>&1
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $ROOT/$OUT/prof_$TAG -o bench -- python $ROOT/bench.py --full --steps 10 --warmup 2 --no-full --no-cpu --no-strong > $ROOT/$OUT/prof_$TAG.log 2>&1
cd $ROOT
tail -4 $OUT/tests_$TAG.log; tail -2 $OUT/smoke_$TAG.log; tail -1 $OUT/bench_$TAG.log; tail -2 $OUT/prof_$TAG.log
find $OUT/prof_$TAG -type f | head
