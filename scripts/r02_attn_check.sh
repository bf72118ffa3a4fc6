#!/bin/bash
# round 2: parity tests, per-kernel averages (rocprofv3 kernel trace) and SQ counters of the attention kernels; run on the GPU box
cd "$(dirname "$0")/.." && R=$PWD; export TMPDIR=/tmp
export OUT=${OUT:-out}   # results directory, relative to the repository root
mkdir -p $OUT
timeout 900 python -m pytest tests/test_gpu_parity.py tests/test_emu_kernels.py -m gpu -q -x --no-header -p no:cacheprovider 2>&1 | tail -3
bash scripts/kstats.sh "" "${1:-attn|dkv|gemm|ln_pool|sum_splits|transpose}" | tee $OUT/r02_kstats.txt
if [ -n "$2" ]; then bash scripts/pmc_sq.sh "$2" > /dev/null 2>&1; cp $OUT/pmc/sq_summary.txt $OUT/r02_pmc_sq.txt; cat $OUT/r02_pmc_sq.txt; fi
