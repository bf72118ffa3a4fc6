#!/bin/bash
# Where the time between kernels goes: rocprofv3 kernel trace of the bench command, idle / overlapped time per replayed step
export OUT=${OUT:-out}   # results directory, relative to the repository root
cd "$(dirname "$0")/.." && R=$PWD; export TMPDIR=/tmp; mkdir -p $OUT
(cd /tmp && rm -rf /tmp/gt && rocprofv3 --kernel-trace --output-format csv -d /tmp/gt -o x -- python $R/bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-head-step --spinup-steps 50 ${BENCH_EXTRA} > /dev/null 2>&1)
python - <<'PY' | tee $OUT/r02_gap_trace.txt
import csv, glob
f = glob.glob('/tmp/gt/**/*kernel_trace.csv', recursive=True)[0]
rows = [(int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name'].split('(')[0][:40], r.get('Queue_Id', ''), r.get('Stream_Id', '')) for r in csv.DictReader(open(f))]
rows.sort()
# steps are delimited by k_adamw_rows launches
idx = [i for i, r in enumerate(rows) if r[2].startswith('k_adamw_rows')]
print('kernels', len(rows), 'adamw launches', len(idx))
import statistics
res = []
for a, b in zip(idx[-12:-1], idx[-11:]):
    seg = rows[a + 1:b + 1]
    t0, t1 = rows[a][1], rows[b][1]
    busy, cur_s, cur_e, ksum = 0, None, None, 0
    for s, e, n, q, st in seg:
        ksum += e - s
        if cur_e is None or s > cur_e:
            if cur_e is not None: busy += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    busy += cur_e - cur_s
    res.append((t1 - t0, busy, ksum, len(seg)))
for r in res[-3:]: print('step wall %.1f us, busy (union of kernels) %.1f, idle %.1f, kernel sum %.1f, kernels %d' % (r[0] / 1e3, r[1] / 1e3, (r[0] - r[1]) / 1e3, r[2] / 1e3, r[3]))
print('median wall %.1f busy %.1f idle %.1f kernel-sum %.1f' % tuple(statistics.median(x[i] for x in res) / 1e3 if i < 3 else 0 for i in (0, 1, 1, 2)))
seg = rows[idx[-2] + 1:idx[-1] + 1]
prev_end = rows[idx[-2]][1]
print('--- last step, kernel by kernel: start offset, duration, gap to the latest end so far')
latest = prev_end
for s, e, n, q, st in seg:
    print('%8.1f %7.1f %6.1f  %s  q%s' % ((s - prev_end) / 1e3, (e - s) / 1e3, (s - latest) / 1e3, n, q))
    latest = max(latest, e)
PY
