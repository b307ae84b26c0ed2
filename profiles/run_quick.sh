#!/bin/bash
# Quick check of a kernel change in one gpurun call: the GPU test suite, the default bench line, a kernel trace of the
# short bench.   bash profiles/run_quick.sh <tag> [pytest args]
tag=${1:-q}
shift
R=$PWD
OUT=${EPA_PROF_OUT:-$PWD/prof_out}; export EPA_PROF_OUT=$OUT   # where raw profiles land (git-ignored)
mkdir -p $OUT
timeout 900 python -m pytest tests -m gpu -x -q "$@" > $OUT/${tag}_gputest.log 2>&1
tail -3 $OUT/${tag}_gputest.log
python bench.py --full --no-cpu-baseline --no-extras > $OUT/${tag}_bench_short.json 2> $OUT/${tag}_bench_short.err
tail -1 $OUT/${tag}_bench_short.json | cut -c1-300
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/${tag}_stats
timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/${tag}_stats -o st -- \
  python $R/bench.py --full --no-cpu-baseline --no-extras > $OUT/${tag}_stats.log 2>&1
cd $R
python profiles/db_to_txt.py $OUT/${tag}_stats/st_results.db > $OUT/${tag}_kernel_trace_stats.txt
head -22 $OUT/${tag}_kernel_trace_stats.txt
rm -rf $OUT/${tag}_stats
