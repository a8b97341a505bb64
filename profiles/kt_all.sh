#!/bin/bash
# per-kernel alone-times (LSX_SERIAL=1) of the all-atoms workload for one library variant:  bash profiles/kt_all.sh TAG LIB
# (outputs under $OUT, default profiles/out/kta_TAG)
TAG=$1; LIB=$2
cd "$(dirname "$0")/.." && D=${OUT:-profiles/out}/kta_$TAG && mkdir -p $D
LSX_SERIAL=1 LSX_HIP_LIBRARY=$LIB timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $D -o kt -- python3 bench.py --full --workload all --steps 10 --warmup 2 --no-cpu-baseline --no-single-column > $D/run.log 2>&1 || exit 1
cp $(find $D -name "*kernel_stats.csv") ${D}_stats.csv
find $D -name "*trace.csv" -delete
grep "fast_gamma\|fast_prepass\|gamma_finish" ${D}_stats.csv | cut -d, -f1-4 | sed 's/(anonymous namespace):://g' | cut -c1-120
tail -c 400 $D/run.log | grep -o '"summary": {[^}]*}'
