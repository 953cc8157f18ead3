#!/bin/bash
# usage: tools/winsize_profile.sh [tag] [ws ...] -- one rocprofv3 --kernel-trace --stats run of tools/winsize_bench.py per
# window (64 x 1080p pairs per batch, 1 warm-up + 3 timed batches), then tools/winsize_summary.py: level-0 per-launch
# times into profiles/<tag>_level0.csv, each window's --stats table beside it
tag=${1:-winsize}
shift
ws_list=${*:-15 17 19 31 61 127 255}
cd $(dirname $0)/..
out=${OUT_DIR:-traces}/$tag
rm -rf $out; mkdir -p $out profiles
for ws in $ws_list; do
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/winsize_$ws -- \
      python3 tools/winsize_bench.py --reps 3 --warmup 1 $ws > $out/winsize_$ws.log 2>&1 \
    || { echo "profiled run winsize $ws failed"; tail -5 $out/winsize_$ws.log; exit 1; }
  cat $out/winsize_$ws.log
  cp $(find $out/winsize_$ws -name "*kernel_stats.csv" | head -1) profiles/${tag}_${ws}_kernel_stats.csv
done
python3 tools/winsize_summary.py $out profiles/${tag}_level0.csv && cat profiles/${tag}_level0.csv
