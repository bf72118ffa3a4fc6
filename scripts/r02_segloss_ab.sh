#!/bin/bash
# segloss backward: block form (default) against the round-1 gather form; tests, op time and per-kernel time
export OUT=${OUT:-out}   # results directory, relative to the repository root
cd "$(dirname "$0")/.."; export TMPDIR=/tmp; mkdir -p $OUT; R=$(pwd)
timeout 600 python -m pytest tests/test_segloss.py tests/test_segfuse.py -m gpu -x -q --no-header -p no:cacheprovider 2>&1 | tail -3
for f in block gather; do
  echo "== CFFM_UPCE_BWD=$f"; CFFM_UPCE_BWD=$f timeout 300 python scripts/segloss_bench.py 2>/dev/null | tail -1
done
for t in ${TYS:-4 5 8 10 12}; do
  echo "== block, CFFM_UPCE_TY=$t"; CFFM_UPCE_TY=$t timeout 300 python scripts/segloss_bench.py 2>/dev/null | tail -1 | cut -c1-70
done
cd /tmp
for f in block; do
  rm -rf /tmp/sl_$f; CFFM_UPCE_BWD=$f timeout 300 rocprofv3 --kernel-trace --stats -d /tmp/sl_$f -o t -- python $R/scripts/segloss_bench.py > /dev/null 2>&1
  echo "== kernel stats $f"; python - <<PY
import csv, glob
for p in glob.glob('/tmp/sl_$f/**/*kernel_stats.csv', recursive=True):
    for r in csv.DictReader(open(p)):
        if 'upce' in r['Name']: print(r['Name'][:40], r['Calls'], r['AverageNs'])
PY
done
