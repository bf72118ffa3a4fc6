#!/bin/bash
cd "$(dirname "$0")/.."; export TMPDIR=/tmp
show() { python - "$1" <<'PY'
import json,sys
try:
    j=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
    print(j['value'], j['ms_per_step'], 'graph', j['config']['hip_graph'], 'sync', j['config']['ranks_in_sync'], 'finite', j['config']['params_finite'])
except Exception as e:
    print('no JSON line:', e)
PY
}
for v in "--graph" "--eager" ""; do
echo "== 2 ranks gloo one device $v"
CFFM_BENCH_BACKEND=gloo CFFM_BENCH_ONE_DEVICE=1 timeout 900 python bench.py --full --gpus 2 --steps 10 --warmup 3 --spinup-steps 20 --no-stage-timing $v > /tmp/d.log 2> /tmp/d.err; echo rc=$?; grep -v "Gloo\|socket\|amdgpu" /tmp/d.err | tail -3; show /tmp/d.log
done
