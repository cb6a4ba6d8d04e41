#!/bin/bash
OUT=${OUT:-out}   # output folder, relative to the repository root
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}; TAG=${1:-x}
mkdir -p $ROOT/$OUT; cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $ROOT/$OUT/prof_$TAG -o bench -- python $ROOT/bench.py --full --steps 10 --warmup 2 --no-full --no-cpu > $ROOT/$OUT/prof_$TAG.log 2>&1
tail -1 $ROOT/$OUT/prof_$TAG.log | cut -c1-300
