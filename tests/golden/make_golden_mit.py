#!/usr/bin/env python
"""Golden vectors of the MiT backbone, produced by the REFERENCE mit_b0 built through its own registry (mmseg.models imported from the
reference tree with stand-ins for the absent mmcv / timm: oracle/ref_import.py; its DropPath stand-in is the identity, so train mode is
deterministic).  Run in the build container only:  python tests/golden/make_golden_mit.py
Stores outputs and gradients only; parameters and inputs are regenerated from oracle/recipe.py (state seed 40, image seed 41, the
weights of the scalar loss seed 42).  The stored values are the reference run in fp64, rounded to fp32; every gradient comes with its
gate = 10 x max|fp32 run - fp64 run| of the reference itself, floored at 1e-6 of the tensor's largest element.

    mit_b0_64.npz             train mode, [2,3,64,64]: the four outputs, the input gradient and the parameter gradients of
                              sum_i (out_i * w_i).sum() -- in full for tensors of <= 16384 elements, the first 4096 elements otherwise
    mit_b0_64_grads34.npz     ... of which the gradients of stages 3 and 4 (block3, norm3, block4, norm4) live here: one file with all
                              of them would pass 1 MiB
    mit_b0_96x72.npz          eval mode, [1,3,96,72]: the four outputs (maps 24x18, 12x9, 6x5, 3x3; every sr convolution floors to 3x2)
    mit_state_dict_keys.json  keys, shapes and dtypes of mit_b0 .. mit_b5
    seg_mit_b0_64.npz         the reference EncoderDecoder_clips with mit_b0 and the B0 head (recipe seed 30) on one 4-frame 64x64 clip
                              (seed 43): the head's eval logits [1,124,16,16]
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import recipe as R, ref_import as RI  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
FULL, HEAD = 16384, 4096


def stored(t):
    """what the fixture keeps of a parameter gradient"""
    t = t.detach().reshape(-1)
    return t if t.numel() <= FULL else t[:HEAD]


def build(kind='mit_b0', dtype=torch.float32):
    M = RI.import_mmseg_models()
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.build_backbone(dict(type=kind, style='pytorch'))
    res = m.load_state_dict(R.synth_state(m, seed=40), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m.to(dtype)


def run_train(m, dtype):
    m.train()
    img = R.synth_input('img', (2, 3, 64, 64), seed=41, scale=1.0, dtype=dtype).requires_grad_(True)
    outs = m(img)
    sum((o * R.synth_input('w%d' % i, o.shape, seed=42, scale=1.0, dtype=dtype)).sum() for i, o in enumerate(outs)).backward()
    return [o.detach() for o in outs], img.grad, {k: p.grad for k, p in m.named_parameters()}


def main():
    torch.manual_seed(0)
    # ---- 64 x 64, train mode, outputs + gradients
    o32, di32, g32 = run_train(build(), torch.float32)
    o64, di64, g64 = run_train(build(dtype=torch.float64), torch.float64)
    d = {}
    for i, (a, b) in enumerate(zip(o32, o64)):
        d['out%d' % i] = b.float().numpy()
        print('out%d %s max %.3e, fp32 - fp64 %.2e of it' % (i, tuple(b.shape), float(b.abs().max()), float((a.double() - b).abs().max() / b.abs().max())))

    def gate(a, b):
        return np.float64(max(10 * float((a.double() - b).abs().max()), 1e-6 * float(b.abs().max())))

    d['dimg'], d['gate:dimg'] = di64.float().numpy(), gate(di32, di64)
    assert len(g64) == 176
    for k in g64:
        d['grad:' + k], d['gate:' + k] = stored(g64[k]).float().numpy(), gate(stored(g32[k]), stored(g64[k]))
    rel = [float(d['gate:' + k] / max(float(stored(g64[k]).abs().max()), 1e-30)) for k in g64]
    print('gradient gates: %.2e .. %.2e of the tensors\' largest elements; dimg %.2e' % (min(rel), max(rel), d['gate:dimg'] / float(di64.abs().max())))
    late = {k: v for k, v in d.items() if k.split(':')[-1].startswith(('block3.', 'norm3.', 'block4.', 'norm4.'))}
    np.savez_compressed(os.path.join(OUT, 'mit_b0_64_grads34.npz'), **late)
    np.savez_compressed(os.path.join(OUT, 'mit_b0_64.npz'), **{k: v for k, v in d.items() if k not in late})
    # ---- 96 x 72, eval mode, outputs only
    m = build(dtype=torch.float64).eval()
    with torch.no_grad():
        outs = m(R.synth_input('img', (1, 3, 96, 72), seed=41, scale=1.0, dtype=torch.float64))
    assert [tuple(o.shape[2:]) for o in outs] == [(24, 18), (12, 9), (6, 5), (3, 3)]
    np.savez_compressed(os.path.join(OUT, 'mit_b0_96x72.npz'), **{'out%d' % i: o.float().numpy() for i, o in enumerate(outs)})
    # ---- keys of the six variants
    M = RI.import_mmseg_models()
    keys = {}
    for kind in ('mit_b0', 'mit_b1', 'mit_b2', 'mit_b3', 'mit_b4', 'mit_b5'):
        with contextlib.redirect_stdout(io.StringIO()):
            v = M.build_backbone(dict(type=kind, style='pytorch'))
        keys[kind] = [[k, list(t.shape), str(t.dtype)] for k, t in v.state_dict().items()]
        print(kind, len(keys[kind]), 'keys')
    json.dump(keys, open(os.path.join(OUT, 'mit_state_dict_keys.json'), 'w'))
    # ---- the segmentor: mit_b0 + the B0 head, eval logits of the head on one clip
    from mmseg.models import builder
    with contextlib.redirect_stdout(io.StringIO()):
        seg = builder.build_segmentor(dict(type='EncoderDecoder_clips', backbone=dict(type='mit_b0', style='pytorch'),
                                           decode_head=RI.head_cfg(), test_cfg=dict(mode='whole')))
    seg.backbone.load_state_dict(R.synth_state(seg.backbone, seed=40), strict=True)
    assert not seg.decode_head.load_state_dict(R.synth_state(seg.decode_head, seed=30), strict=False).unexpected_keys
    seg.eval()
    clip = R.synth_input('clip', (1, 4, 3, 64, 64), seed=43, scale=1.0)
    with torch.no_grad():
        logits = seg.decode_head.forward_test(seg.extract_feat(clip.flatten(0, 1)), None, seg.test_cfg, 1, 4)
    assert tuple(logits.shape) == (1, 124, 16, 16)
    np.savez_compressed(os.path.join(OUT, 'seg_mit_b0_64.npz'), head_logits=logits.numpy())
    for f in ('mit_b0_64.npz', 'mit_b0_64_grads34.npz', 'mit_b0_96x72.npz', 'mit_state_dict_keys.json', 'seg_mit_b0_64.npz'):
        print(f, os.path.getsize(os.path.join(OUT, f)), 'bytes')


if __name__ == '__main__':
    main()
