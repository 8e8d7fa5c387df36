#!/bin/bash
# End-of-round evidence set (runs on the MI355X box, from the repository root):  bash tools/round_profiles.sh r05
# Writes into $MDS_PROFILE_OUT (default profile_out/):
#   <tag>_bench_default.json                 the full `python bench.py --full` line (config 2 + other_configs)
#   <tag>_{bench,long004,predict_fbf}_kernel_stats.csv   rocprofv3 --kernel-trace --stats of each traced config (bench.py's own
#                                            child runs: MDS_KEEP_TRACE_STATS is a prefix, one file per config)
#   <tag>_pmc_hbm.{json,txt}, <tag>_pmc_mfma.{json,txt}   counter passes of the training step (tools/gpu_profile.sh)
#   <tag>_step_timeline.txt, <tag>_launch_table.txt, <tag>_predict_timeline.txt
TAG=${1:-rXX}
ROOT=$(pwd)
export MDS_PROFILE_OUT=$(realpath -m ${MDS_PROFILE_OUT:-profile_out})
OUT=$MDS_PROFILE_OUT
mkdir -p $OUT; export TMPDIR=/tmp
MDS_KEEP_TRACE_STATS=$OUT/${TAG} python bench.py --full > $OUT/${TAG}_bench_default.json 2> $OUT/${TAG}_bench_default.err
SKIP_TRACE=1 bash tools/gpu_profile.sh ${TAG}p --no-other-configs > $OUT/${TAG}_profile.log 2>&1
for k in hbm mfma; do for e in json txt; do [ -f $OUT/${TAG}p_pmc_$k.$e ] && cp $OUT/${TAG}p_pmc_$k.$e $OUT/${TAG}_pmc_$k.$e; done; done
rm -rf /tmp/prof_kt && mkdir -p /tmp/prof_kt
(cd /tmp && rocprofv3 --kernel-trace -d /tmp/prof_kt -o kt --output-format csv -- python $ROOT/bench.py --steps 8 --warmup 3 --profile-steps 0 --no-cpu-baseline --no-pmc --no-other-configs > /dev/null 2> $OUT/${TAG}_trace.err)
f=$(find /tmp/prof_kt -name '*kernel_trace.csv' | head -1)
python tools/step_timeline.py $f 3 > $OUT/${TAG}_step_timeline.txt 2>&1
python tools/launch_table.py 700 > $OUT/${TAG}_launch_table.txt 2>&1
python tools/predict_timeline.py 1 > $OUT/${TAG}_predict_timeline.txt 2>&1
python tools/bench_brief.py < $OUT/${TAG}_bench_default.json 2>/dev/null | head -12
ls -la $OUT/${TAG}_*
