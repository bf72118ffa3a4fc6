#!/bin/bash
# rocprofv3 kernel-trace summary of the default bench command (profiles/r02_bench_kernel_stats.csv) + the bench line itself
export OUT=${OUT:-out}   # results directory, relative to the repository root
cd "$(dirname "$0")/.." && R=$PWD; export TMPDIR=/tmp; mkdir -p $OUT
python bench.py --full --steps 20 --warmup 5 > $OUT/r02_bench.json 2> $OUT/r02_bench.err; tail -2 $OUT/r02_bench.err
(cd /tmp && rm -rf /tmp/bp && rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/bp -o x -- python $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-head-step --spinup-steps 100 > $R/$OUT/r02_bench_prof.json 2>/dev/null)
cp $(find /tmp/bp -name '*kernel_stats.csv' | head -1) $OUT/r02_bench_kernel_stats.csv
python - <<'PY'
import csv, json, os
j = json.load(open(os.path.join(os.environ['OUT'], 'r02_bench.json')))
print('bench:', j['value'], j['ms_per_step'], 'graph', j['config']['hip_graph'], j['config']['hip_graph_calibration'], 'roofline', j['roofline']['frac'], j['roofline']['avg_launch_us'], j['roofline'].get('back_to_back_us'), 'head', j['head_step'] and j['head_step'].get('ms_per_step'), 'cpu', j['cpu_baseline'] and j['cpu_baseline']['value'])
rows = list(csv.DictReader(open(os.path.join(os.environ['OUT'], 'r02_bench_kernel_stats.csv'))))
tot = sum(float(r['TotalDurationNs']) for r in rows)
for r in rows[:32]:
    print('%-64s %6s calls %8.1f us avg %5.1f %%' % (r['Name'][:64], r['Calls'], float(r['AverageNs']) / 1e3, 100 * float(r['TotalDurationNs']) / tot))
PY
