#!/bin/bash
# kernel durations (rocprofv3 --kernel-trace --stats) and SQ counters of the fused resize + cross entropy kernels
cd "$(dirname "$0")/.." && R=$PWD
export TMPDIR=/tmp SEGLOSS_HIP_ONLY=1
export OUT=${OUT:-out}   # results directory, relative to the repository root
mkdir -p $OUT/pmc
(cd /tmp && rm -rf /tmp/slk && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/slk -o sl -- python $R/scripts/segloss_bench.py > $R/$OUT/pmc/slk.log 2>&1)
find /tmp/slk -name "*kernel_stats.csv" -exec cp {} $OUT/r02_segloss_kernel_stats.csv \;
grep -E "upce|Name" $OUT/r02_segloss_kernel_stats.csv | cut -c1-150
i=0
for grp in "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY" "SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS" "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD" "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_VMEM SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE" "SQ_INST_CYCLES_VMEM SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_SCA SQ_INSTS_VMEM_WR" "GRBM_GUI_ACTIVE SQ_INSTS_VALU_TRANS SQ_THREAD_CYCLES_VALU SQ_WAVES_EQ_64"; do
  i=$((i+1))
  (cd /tmp && rm -rf /tmp/slq_$i && timeout 300 rocprofv3 --kernel-trace --pmc $grp --output-format csv -d /tmp/slq_$i -o p -- python $R/scripts/segloss_bench.py > $R/$OUT/pmc/slq_$i.log 2>&1)
done
python - <<'PY' | tee $OUT/r02_segloss_pmc_sq.txt
import csv, glob, collections
acc = collections.defaultdict(lambda: collections.defaultdict(lambda: [0, 0.0]))
for f in glob.glob('/tmp/slq_*/**/*counter_collection.csv', recursive=True):
    for r in csv.DictReader(open(f)):
        k = r['Kernel_Name'].split('(')[0][:48]
        if 'upce' not in k: continue
        a = acc[k][r['Counter_Name']]; a[0] += 1; a[1] += float(r['Counter_Value'])
for k, d in acc.items():
    print(k)
    print('   ' + '  '.join('%s=%.4g' % (c, v[1] / v[0]) for c, v in sorted(d.items())))
PY
