#!/bin/bash
# usage: tools/poly_n_profile.sh [tag]  -- rocprofv3 --kernel-trace --stats of tools/poly_n_batch.py (64 x 1080p pairs per
# batch, poly_n 5 and 7); per-image k_polyexp times into profiles/<tag>_polyexp.csv, the --stats table beside it
tag=${1:-poly_n}
cd $(dirname $0)/..
out=${OUT_DIR:-traces}/poly_n_$tag
rm -rf $out; mkdir -p $out profiles
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $out -- python3 tools/poly_n_batch.py 3 5 7 > $out.log 2>&1 \
  || { echo "profiled run failed"; tail -5 $out.log; exit 1; }
cat $out.log
python3 tools/poly_n_summary.py $out profiles/${tag}_polyexp.csv && cat profiles/${tag}_polyexp.csv
cp $(find $out -name "*kernel_stats.csv" | head -1) profiles/${tag}_kernel_stats.csv
