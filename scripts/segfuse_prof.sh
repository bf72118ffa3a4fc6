#!/bin/bash
# parity + timing + rocprofv3 kernel stats of the fused SegFormer embedding (one GPU-box visit)
export OUT=${OUT:-out}   # results directory, relative to the repository root
cd "$(dirname "$0")/.."; export TMPDIR=/tmp; mkdir -p $OUT/prof_sf
timeout 900 python -m pytest tests/test_segfuse.py -m gpu -q -x --no-header -p no:cacheprovider 2>&1 | tail -3
timeout 300 python scripts/segfuse_bench.py 2>/dev/null | tail -1 | tee $OUT/segfuse_bench.json
(cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_sf -o sf -- python $OLDPWD/scripts/segfuse_bench.py > $OLDPWD/$OUT/sf_rocprof.log 2>&1)
find /tmp/prof_sf -name "*kernel_stats.csv" -exec cp {} $OUT/prof_sf/ \;
grep "k_segfuse" $OUT/prof_sf/sf_kernel_stats.csv | cut -c1-120
