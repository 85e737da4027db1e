#!/bin/bash
# The default bench command with one build of libhgx under the kernel tracer, for a before / after of the class dedup:
#   tools/dedup_profile.sh <path/to/libhgx.so> <out dir>
# -> <out dir>/stats/*_kernel_stats.csv (rocprofv3 --stats), kernel_per_step.txt (launches, average, sum per step), step_timeline.txt
#    (the last step's dispatches), bench_under_rocprof.json; then an untraced short run with --dump-outputs -> <out dir>/out/*.npy
# (tools/compare_dumps.py compares two such directories).  No counters in the traced run; the program itself follows `--`.
set -u -o pipefail
LIB=$1; D=$2
mkdir -p $D
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $D/stats -o p -- python3 tools/bench_with_lib.py $LIB > $D/bench_under_rocprof.json 2> $D/stats.err || exit $?
T=$(ls $D/stats/*kernel_trace.csv | head -1)
python3 tools/step_timeline.py $T > $D/step_timeline.txt
python3 tools/kernel_per_step.py $T > $D/kernel_per_step.txt
rm -f $D/stats/*kernel_trace.csv $D/stats/*agent_info.csv
timeout -k 10 300 python3 tools/bench_with_lib.py $LIB --dump-outputs $D/out --steps 3 --warmup 2 > $D/bench_dump.json 2> $D/dump.err || exit $?
