#!/bin/bash
# usage: tools/ab.sh : A/B of two builds of libofc.so kept as ab_nopref.so and ab_pref.so in the repository root
for i in 1 2 3; do
  cp ab_nopref.so opticalflowclustering_amd/libofc.so; python bench.py --full --no-cpu | python tools/brief.py nopref
  cp ab_pref.so opticalflowclustering_amd/libofc.so; python bench.py --full --no-cpu | python tools/brief.py pref
done
