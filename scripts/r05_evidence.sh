#!/bin/bash
# Round-5 evidence in one GPU-box visit; everything lands in $OUT/ with r05_ names (copied into profiles/ afterwards):
#   r05_bench.json / .err          the default bench line
#   r05_bench_kernel_stats.csv     rocprofv3 --kernel-trace --stats of the bench command (no cpu baseline / head step legs)
#   r05_timeline_graph.txt         one replayed step: start / duration / hardware queue of every kernel (scripts/r05_trace.sh)
#   r05_pmc_FETCH_SIZE.csv, r05_pmc_WRITE_SIZE.csv, r05_pmc_attn_fwd.json   HBM traffic (separate --pmc passes)
#   r05_pmc_sq.txt                 SQ issue / stall counters of the hot kernels
#   r05_stage_kernel_stats.txt     per-kernel durations of one clip-block step launched eagerly (scripts/kstats.sh)
#   r05_head_step.txt              torch-profiler attribution of the whole-head step
#   r05_gtc_step.json, r05_gtc_kernel_stats.csv, r05_gtc_fused_vs_unfused.txt   the CFFM++ prototype layer (BASELINE config 5)
#   r05_dw_dma_bench.txt           the LDS-DMA weight-gradient kernel against the register-staged group
#   r05_dw_stream_bench.txt        the streaming weight-gradient kernel (T-frag operands) against the register-staged group
#   r05_gpu_suite.txt              tail of pytest -m gpu

export OUT=${OUT:-out}   # results directory, relative to the repository root
cd "$(dirname "$0")/.." && R=$PWD; export TMPDIR=/tmp; mkdir -p $OUT/pmc
python bench.py --full --steps 20 --warmup 5 > $OUT/r05_bench.json 2> $OUT/r05_bench.err; tail -2 $OUT/r05_bench.err
(cd /tmp && rm -rf /tmp/bp && rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/bp -o x -- python $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-head-step --no-gtc-step --spinup-steps 100 > $R/$OUT/r05_bench_prof.json 2>/dev/null)
cp $(find /tmp/bp -name '*kernel_stats.csv' | head -1) $OUT/r05_bench_kernel_stats.csv
python - <<'PY'
import csv, json, os
j = json.loads(open(os.path.join(os.environ['OUT'], 'r05_bench.json')).read().strip().splitlines()[-1])
print('bench:', j['value'], j['ms_per_step'], 'graph', j['config']['hip_graph'], j['config']['hip_graph_calibration'], 'roofline', j['roofline']['frac'], j['roofline']['avg_launch_us'], j['roofline'].get('back_to_back_us'), 'head', j['head_step'] and j['head_step'].get('ms_per_step'), 'cpu', j['cpu_baseline'] and j['cpu_baseline']['value'])
rows = list(csv.DictReader(open(os.path.join(os.environ['OUT'], 'r05_bench_kernel_stats.csv'))))
tot = sum(float(r['TotalDurationNs']) for r in rows)
for r in rows[:30]:
    print('%-64s %6s calls %8.1f us avg %5.1f %%' % (r['Name'][:64], r['Calls'], float(r['AverageNs']) / 1e3, 100 * float(r['TotalDurationNs']) / tot))
PY
bash scripts/r05_trace.sh graph --graph | head -3; cp $OUT/r05_timeline_graph.txt $OUT/r05_timeline_graph_evidence.txt
bash scripts/pmc_attn.sh > $OUT/r05_pmc_hbm.txt 2>&1
cp $OUT/pmc/FETCH_SIZE.summary.csv $OUT/r05_pmc_FETCH_SIZE.csv; cp $OUT/pmc/WRITE_SIZE.summary.csv $OUT/r05_pmc_WRITE_SIZE.csv
python - <<'PY'
import json, os
def load(p):      # kernel names contain commas: the two numeric columns are the last two fields
    out = {}
    for line in list(open(p))[1:]:
        name, n, avg = line.rstrip().rsplit(',', 2)
        out[name] = float(avg)
    return out
f, w = load(os.path.join(os.environ['OUT'], 'r05_pmc_FETCH_SIZE.csv')), load(os.path.join(os.environ['OUT'], 'r05_pmc_WRITE_SIZE.csv'))
k = [n for n in f if 'k_cfm_attn_fwd' in n][0]
cal = [n for n in f if 'k_mlp_fwd' in n]
calnote = ''
if cal:
    c = cal[0]
    calnote = ('same run: k_mlp_fwd (B = 2: reads 7.4 MB attention output + 7.4 MB residual rows + 2.25 MB of weights, writes x1, z2, hraw, act, x2 = 81 MB as '
               '16-byte stores) reports FETCH_SIZE %.2f MB / WRITE_SIZE %.2f MB; ' % (f.get(c, 0) / 1024, w.get(c, 0) / 1024))
out = {'kernel': 'k_cfm_attn_fwd', 'batch_clips': 2, 'FETCH_SIZE_KB_per_launch': f[k], 'WRITE_SIZE_KB_per_launch': w.get(k, 0.0),
       'hbm_bytes_per_launch_raw': int((f[k] + w.get(k, 0.0)) * 1024), 'hbm_bytes_per_launch_fetch_x2': int((2 * f[k] + w.get(k, 0.0)) * 1024),
       'calibration': (calnote + 'WRITE_SIZE is exact for the attention kernel (2 x 3600 tokens x 256 x 4 B + lse = 7.52 MB); it gathers 64-byte (token, head) slices '
                       'of the f16 q/k/v rows (unique data 15.9 MB), for which the raw FETCH counter already matches (MI355X_MICROARCH.md halves FETCH_SIZE only for wide '
                       'streaming reads), so the raw value is reported as traffic and the x2 value as an upper bound'),
       'source': 'rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (separate passes), scripts/pmc_attn.sh; profiles/r05_pmc_*.csv'}
json.dump(out, open(os.path.join(os.environ['OUT'], 'r05_pmc_attn_fwd.json'), 'w'), indent=1)
print(json.dumps(out)[:300])
PY
bash scripts/r05_pmc_table.sh > /dev/null 2>&1; head -8 $OUT/r05_pmc_sq.txt
bash scripts/kstats.sh "" "." > $OUT/r05_stage_kernel_stats.txt 2>&1
bash scripts/r02_head_profile.sh > $OUT/r05_head_step.txt 2>&1; head -12 $OUT/r05_head_step.txt
bash scripts/r05_gtc.sh > $OUT/r05_gtc_all.txt 2>&1; grep -A3 "K=100" $OUT/r05_gtc_step.json | head -5
python scripts/r05_dw_dma_bench.py > $OUT/r05_dw_dma_bench.txt 2>&1; tail -4 $OUT/r05_dw_dma_bench.txt
python scripts/r05_dw_stream_bench.py > $OUT/r05_dw_stream_bench.txt 2>&1; tail -8 $OUT/r05_dw_stream_bench.txt
timeout 1800 python -m pytest tests -q -m gpu 2>&1 | tail -4 > $OUT/r05_gpu_suite.txt; cat $OUT/r05_gpu_suite.txt
