#!/bin/bash
# round-2 PMC evidence: FETCH_SIZE / WRITE_SIZE (separate passes) and the SQ counter groups of the attention kernels
export OUT=${OUT:-out}   # results directory, relative to the repository root
cd "$(dirname "$0")/.."; export TMPDIR=/tmp; mkdir -p $OUT/pmc
bash scripts/pmc_attn.sh > $OUT/r02_pmc_hbm.txt 2>&1
cp $OUT/pmc/FETCH_SIZE.summary.csv $OUT/r02_pmc_FETCH_SIZE.csv; cp $OUT/pmc/WRITE_SIZE.summary.csv $OUT/r02_pmc_WRITE_SIZE.csv
bash scripts/pmc_sq.sh "attn|dkv_gather|ln_pool|gemm" > /dev/null 2>&1; cp $OUT/pmc/sq_summary.txt $OUT/r02_pmc_sq.txt
bash scripts/kstats.sh "" "." > $OUT/r02_stage_kernel_stats.txt 2>&1
head -14 $OUT/r02_pmc_FETCH_SIZE.csv; head -14 $OUT/r02_pmc_WRITE_SIZE.csv; grep -A1 "attn" $OUT/r02_pmc_sq.txt | head -12
