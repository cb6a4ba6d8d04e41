#!/bin/bash
# round 5: full GPU suite, smoke, default bench, kernel-trace stats of a short bench
OUT=${OUT:-out}   # output folder, relative to the repository root
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd $ROOT; mkdir -p $OUT
TAG=${1:-r5}
timeout 3000 python -m pytest tests -q -m gpu -p no:cacheprovider 2>&1 | grep -v amdgpu.ids | tail -15 > $OUT/tests_$TAG.log
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1
timeout 900 python bench.py --full > $OUT/bench_$TAG.log 2>&1
tail -1 $OUT/bench_$TAG.log > $OUT/bench_$TAG.json
cd /tmp && export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof_$TAG -o bench -- python $ROOT/bench.py --full --steps 10 --warmup 2 --no-full --no-cpu --no-strong --no-train --no-ab > $ROOT/$OUT/prof_$TAG.log 2>&1
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof_${TAG}_c3 -o bench -- python $ROOT/bench.py --full --config C3 --steps 10 --warmup 2 --no-full --no-cpu --no-strong --no-train --no-ab --no-c2 > $ROOT/$OUT/prof_${TAG}_c3.log 2>&1
cd $ROOT
tail -6 $OUT/tests_$TAG.log; tail -2 $OUT/smoke_$TAG.log; tail -c 600 $OUT/bench_$TAG.json; echo; find $OUT/prof_$TAG -name "*stats*" | head
