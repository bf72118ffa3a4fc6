"""Read a `rocprofv3 --kernel-trace --output-format csv` trace of a bench.py run: per-kernel figures over the last whole steps, the end
of the layer backward (from the end of k_ln_pool_bwd_ref to the start of k_adamw_rows_tick) and the timeline of one step.
usage: python scripts/trace_step.py <..._kernel_trace.csv> [steps, default 20]
A step starts at k_transpose_prep.  "#n" = the n-th launch of that kernel inside a step, for the kernels that run more than once."""
import collections
import csv
import sys


def short(name):
    name = name.replace('void ', '')
    for cut in ('(', '<'):
        if cut in name and not name.startswith('_Z'):
            name = name[:name.index(cut)]
    return name[:44]


def stats(v):
    return '%7.2f [%6.2f %6.2f]' % (sum(v) / len(v), min(v), max(v)) if v else '      -'


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    nsteps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    for r in rows:
        r['s'], r['e'] = int(r['Start_Timestamp']) / 1e3, int(r['End_Timestamp']) / 1e3
    rows.sort(key=lambda r: r['s'])
    idx = [i for i, r in enumerate(rows) if r['Kernel_Name'].startswith('k_transpose_prep')]
    idx = idx[-(nsteps + 1):]
    steps = [rows[a:b] for a, b in zip(idx[:-1], idx[1:])]
    print('%d whole steps, step period %s us' % (len(steps), stats([b[0]['s'] - a[0]['s'] for a, b in zip(steps[:-1], steps[1:])])))
    dur, count = collections.defaultdict(list), collections.Counter()
    tail, gap_tgt = collections.defaultdict(list), []
    for st in steps:
        seen = collections.Counter()
        ref_end = adamw = tgt_end = None
        for r in st:
            k = short(r['Kernel_Name'])
            seen[k] += 1
            dur[k].append(r['e'] - r['s'])
            dur['%s #%d' % (k, seen[k])].append(r['e'] - r['s'])
            if k.startswith('k_ln_pool_bwd_ref'):
                ref_end = r['e']
            elif k.startswith('k_adamw_rows_tick') and ref_end is not None and adamw is None:
                adamw = r['s']
            elif ref_end is not None and adamw is None:
                tail[k].append(r['e'] - r['s'])
            if k.startswith('k_ln_pool_bwd_tgt') and seen[k] == 1:
                tgt_end = r['e']
            if k.startswith('k_mlp_bwd') and seen[k] == 2 and tgt_end is not None:
                gap_tgt.append(r['s'] - tgt_end)
        for k, n in seen.items():
            count[k] = max(count[k], n)
        if ref_end is not None and adamw is not None:
            tail['end of k_ln_pool_bwd_ref -> start of k_adamw_rows_tick'].append(adamw - ref_end)
    print('kernel: launches per step, average us [min max]')
    for k in sorted(dur, key=lambda k: -sum(dur[k]) / len(dur[k])):
        base = k.split(' #')[0]
        if ' #' in k and count[base] < 2:
            continue
        print('  %-52s %3s  %s' % (k, count[k] if ' #' not in k else '', stats(dur[k])))
    print('behind k_ln_pool_bwd_ref, before k_adamw_rows_tick (any queue): average us [min max]')
    for k, v in tail.items():
        print('  %-60s %s' % (k, stats(v)))
    print('  start of the second k_mlp_bwd - end of the first k_ln_pool_bwd_tgt  %s' % stats(gap_tgt))
    st = steps[-3] if len(steps) > 3 else steps[-1]
    print('one step (start us, duration us, queue):')
    for r in st:
        print('%9.1f %8.1f  q%-3s %s' % (r['s'] - st[0]['s'], r['e'] - r['s'], r.get('Queue_Id', '?'), r['Kernel_Name'][:90]))


if __name__ == '__main__':
    main()
