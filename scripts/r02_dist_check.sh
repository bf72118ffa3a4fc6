#!/bin/bash
# the N > 1 paths of bench.py on a one-GPU box: self-launched 2 ranks sharing cuda:0 over gloo (graph pieces + eager), and
# RCCL itself with a single rank (CFFM_BENCH_FORCE_DIST) for the graph-pieces default, eager blockwise overlap and torch DDP
export OUT=${OUT:-out}   # results directory, relative to the repository root
cd "$(dirname "$0")/.."; export TMPDIR=/tmp; mkdir -p $OUT
show() { python - "$1" <<'PY'
import json,sys
try:
    j=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
    print(j['value'], j['ms_per_step'], 'n_gpus', j['n_gpus'], j['rccl'], 'graph', j['config']['hip_graph'], j['config']['hip_graph_calibration'], 'sync', j['config']['ranks_in_sync'], '|', j['config']['hip_graph_note'])
except Exception as e:
    print('no JSON line:', e)
PY
}
echo "== python bench.py --gpus 2 (self-launch; gloo, both ranks on cuda:0)"
CFFM_BENCH_BACKEND=gloo CFFM_BENCH_ONE_DEVICE=1 timeout 900 python bench.py --full --gpus 2 --steps 10 --warmup 3 --spinup-steps 20 --no-stage-timing > $OUT/d2.log 2> $OUT/d2.err; echo rc=$?; tail -c 500 $OUT/d2.err; show $OUT/d2.log
echo "== same, --eager"
CFFM_BENCH_BACKEND=gloo CFFM_BENCH_ONE_DEVICE=1 timeout 900 python bench.py --full --gpus 2 --steps 10 --warmup 3 --spinup-steps 20 --no-stage-timing --eager > $OUT/d2e.log 2> $OUT/d2e.err; echo rc=$?; tail -c 300 $OUT/d2e.err; show $OUT/d2e.log
for v in "" "--eager" "--ddp"; do
  echo "== RCCL, single rank, $v"
  CFFM_BENCH_FORCE_DIST=1 timeout 400 python bench.py --full --no-cpu-baseline --no-head-step $v > $OUT/dr.log 2> $OUT/dr.err; echo "rc=$?"; tail -c 300 $OUT/dr.err; show $OUT/dr.log
done
