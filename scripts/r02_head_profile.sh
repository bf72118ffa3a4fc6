#!/bin/bash
# the whole-head training step: GPU tests of the fused row path + torch-profiler kernel attribution of the step
export OUT=${OUT:-out}   # results directory, relative to the repository root
cd "$(dirname "$0")/.."; export TMPDIR=/tmp; mkdir -p $OUT
timeout 900 python -m pytest tests/test_headfuse.py tests/test_boundary.py tests/test_data.py tests/test_segfuse.py tests/test_segloss.py -m gpu -x -q --no-header -p no:cacheprovider 2>&1 | tail -3
HEAD_STEP_ONLY=hip,hip python scripts/head_step_bench.py 2>/dev/null | tail -1
python - <<'PY'
import os, sys, torch
sys.path.insert(0, os.getcwd())
import vss_cffm_amd as V
from vss_cffm_amd.head import revert_sync_batchnorm
B1 = (64, 128, 320, 512)
dev = torch.device('cuda:0'); torch.manual_seed(0)
cfg = dict(type='CFFMHead_clips_resize1_8', in_channels=list(B1), in_index=[0, 1, 2, 3], feature_strides=[4, 8, 16, 32], channels=128, dropout_ratio=0.1, num_classes=124,
           norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False, decoder_params=dict(embed_dim=256, depths=2),
           loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0), num_clips=4)
head = revert_sync_batchnorm(V.build_head(cfg)).to(dev).train()
gen = torch.Generator().manual_seed(1)
feats = [torch.randn(8, c, 480 // s, 480 // s, generator=gen).to(dev).requires_grad_(True) for c, s in zip(B1, (4, 8, 16, 32))]
labels = torch.randint(0, 124, (2, 4, 1, 480, 480), generator=gen).to(dev)
def step():
    for p in head.parameters(): p.grad = None
    for f in feats: f.grad = None
    head.forward_train(feats, None, labels, None, 2, 4)['loss_seg'].backward()
for _ in range(3): step()
torch.cuda.synchronize()
from torch.profiler import profile, ProfilerActivity
with profile(activities=[ProfilerActivity.CUDA]) as prof:
    for _ in range(5): step()
    torch.cuda.synchronize()
rows = sorted(prof.key_averages(), key=lambda e: -e.device_time_total)[:28]
tot = sum(e.device_time_total for e in prof.key_averages())
print('GPU time per step: %.3f ms' % (tot / 5 / 1e3))
for e in rows: print('%-70s %4d calls/step %8.1f us/step' % (e.key[:70], e.count // 5, e.device_time_total / 5))
PY
