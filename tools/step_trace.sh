#!/bin/bash
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
dir=${OUT_DIR:-traces}; out=$dir/step_trace
rm -rf $out; mkdir -p $dir
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out -- python3 bench.py --full --no-cpu --no-extras --steps 3 --engines ${1:-2} > $out.log 2>&1
grep '^{' $out.log | python3 tools/brief.py traced
python3 tools/trace_timeline.py $out
cp $(find $out -name "*kernel_stats.csv" | head -1) $dir/step_kernel_stats.csv
