"""Times streaming video inference (vss_cffm_amd.ClipStream) against the clip path on one MI355X.

    python scripts/bench_stream.py [--reps 25] [--out profiles/stream.txt]

Step `kernel`: cffm_segfuse_pool_fwd alone against cffm_segfuse_fwd + cffm_bn_relu_pool_fwd (what the eval rows path runs for the same
rows) at (N,H,W) = (1,120,216) and (4,120,120), maps at 1/2, 1/4 and 1/8 of the side; each time as a share of its byte count at 8 TB/s,
the counts computed here from the shapes (every tensor once per pass that touches it; the re-reads of the small maps by neighbouring
patches are L2 traffic and not counted).
Step `layer`: cffm_layer_infer_rows_ring on a 10-slot ring against index_select + transpose (the gather that builds the stack) +
cffm_layer_infer_rows, at (1,60,108), depth 2.
Steps `b1_864_*`, `b1_480_*`: the per-frame time of ClipStream.push (frames i >= 9 only: the regular clips) against simple_test on the
4-frame clip, mit_b1 + the B1 head at [1,3,480,864] and [1,3,480,480], with the backbone's stage_impl / embed_impl at 'torch' and at
'hip'; label maps to the device (to_numpy=False).

Method (as scripts/bench_mit.py): the parent never opens the GPU; each step is one child process under its own time limit and the next
starts only if the one before ended well.  Everything is warmed up first and the outputs are compared before anything is timed; one
repetition times every variant once, in turn (the variants ALTERNATE), between two device events; a figure is the median over the
repetitions, its spread the distance between the 10th and the 90th percentile.  Streaming counts as faster when median(clip) -
median(stream) exceeds the sum of the two spreads.  The script reads nothing outside the tree."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_mit import alternate, fmt  # noqa: E402

KERNEL_SHAPES = ((1, 120, 216), (4, 120, 120))
MODEL_INPUTS = {'864': (1, 3, 480, 864), '480': (1, 3, 480, 480)}
STEP_LIMIT = {'kernel': 180, 'layer': 180, 'b1_864_torch': 300, 'b1_864_hip': 300, 'b1_480_torch': 300, 'b1_480_hip': 300}
HBM = 8e12


def verdict(old, new, what):
    gain, spread = old['median'] - new['median'], (old['p90'] - old['p10']) + (new['p90'] - new['p10'])
    return '%s: ratio %.2f, difference %.1f us against a sum of spreads of %.1f us -> faster beyond the spreads: %s' % (
        what, old['median'] / new['median'], gain, spread, 'yes' if gain > spread else 'NO')


def child_kernel(reps):
    import torch
    from vss_cffm_amd import _lib, ops
    dev, lib = torch.device('cuda:0'), _lib.get()
    res = []
    for n, h, w in KERNEL_SHAPES:
        g = torch.Generator().manual_seed(0)
        maps = [(h // 2, w // 2), (h // 4, w // 4), (h // 8, w // 8)]
        y0 = torch.randn(n * h * w, 256, generator=g).to(dev)
        d = torch.randn(256, generator=g).to(dev)
        z = [torch.randn(n * a * b, 256, generator=g).to(dev) for a, b in maps]
        scale, shift = (0.5 + torch.rand(256, generator=g)).to(dev), (0.3 * torch.randn(256, generator=g)).to(dev)
        zp = (C.c_void_p * 3)(*[t.data_ptr() for t in z])
        hs, ws = (C.c_int * 3)(*[a for a, _ in maps]), (C.c_int * 3)(*[b for _, b in maps])
        rows = n * (h // 2) * (w // 2)
        y, fused, stack = y0.clone(), torch.empty_like(y0), torch.empty(rows, 256, device=dev)
        ring, slots = torch.empty(2, rows, 256, device=dev), torch.tensor([0, 0, 0, 1], dtype=torch.int32).to(dev)
        st = ops._stream(y)

        def pair():
            # (y is updated in place: from the second call on the values drift, the bytes and the work do not)
            _lib.check(lib.cffm_segfuse_fwd(ops._ptr(y), ops._ptr(d), zp, hs, ws, 3, n, h, w, st), lib)
            _lib.check(lib.cffm_bn_relu_pool_fwd(ops._ptr(y), ops._ptr(scale), ops._ptr(shift), None, ops._ptr(fused), ops._ptr(stack), n, h, w, st), lib)

        def fused_pool():
            _lib.check(lib.cffm_segfuse_pool_fwd(ops._ptr(y0), ops._ptr(d), zp, hs, ws, 3, ops._ptr(scale), ops._ptr(shift), ops._ptr(ring),
                                                 rows * 256, 2, ops._ptr(slots), 3, n, h, w, st), lib)

        pair()
        fused_pool()
        torch.cuda.synchronize()
        same = bool(torch.equal(ring[1], stack))
        us = alternate({'pair': pair, 'pool': fused_pool}, reps, 8)
        full, small, out = 4 * y0.numel(), 4 * sum(t.numel() for t in z), 4 * rows * 256
        res.append(dict(shape=[n, h, w], same=same, us=us, bytes_pair=(2 * full + small) + (full + full + out), bytes_pool=full + small + out,
                        bytes_maps=small))
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), shapes=res)), flush=True)


def child_layer(reps):
    import torch
    from scripts.bench_infer import layer_params
    from vss_cffm_amd import _lib, ops
    dev, lib = torch.device('cuda:0'), _lib.get()
    b, h, w, depth, r = 1, 60, 108, 2, 10
    params = layer_params(depth, dev)
    prepared = ops.layer_prepare(depth, params)
    ring = torch.randn(r, b, h * w, 256, device=dev)
    slots = torch.tensor([0, 3, 6, 9], dtype=torch.int32).to(dev)
    idx = slots.long()
    need = lib.cffm_layer_infer_ws_floats(C.byref(ops.make_geom(lib, b, h, w)))
    ws, out_a, out_b = torch.empty(need, device=dev), torch.empty(b, h * w, 256, device=dev), torch.empty(b, h * w, 256, device=dev)

    def gathered():
        stack = ring.index_select(0, idx).transpose(0, 1).contiguous()
        return ops.cffm_layer_rows_infer(stack, h, w, depth, params, prepared, ws=ws, out=out_a)

    def from_ring():
        return ops.cffm_layer_rows_ring(ring, slots, h, w, depth, params, prepared, ws=ws, out=out_b)

    gathered()
    from_ring()
    torch.cuda.synchronize()
    same = bool(torch.equal(out_a, out_b))
    us = alternate({'gather+layer': gathered, 'ring': from_ring}, reps, 8)
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), shape=[b, h, w, depth], same=same, us=us,
                                      gather_bytes=2 * 4 * 4 * b * h * w * 256, copy_bytes=2 * 4 * b * h * w * 256)), flush=True)


def child_model(which, kind, reps):
    import torch
    import vss_cffm_amd as V
    from oracle import recipe as R
    from vss_cffm_amd import backbone as B
    dev = torch.device('cuda:0')
    model = V.Config.fromfile(os.path.join(ROOT, 'configs', 'cffm_b1_480.py')).model.copy()
    model['backbone'] = dict(type='mit_b1', style='pytorch')
    seg = V.build_segmentor(model, test_cfg=dict(mode='whole'))
    seg.decode_head.load_state_dict(R.synth_state(seg.decode_head, seed=30), strict=False)
    seg.backbone.load_state_dict(R.synth_state(seg.backbone, seed=40), strict=True)
    seg.to(dev).eval()
    B.MixVisionTransformer.stage_impl = B.MixVisionTransformer.embed_impl = kind
    shape = MODEL_INPUTS[which]
    n_frames = 14
    video = [R.synth_input('frame%d' % i, shape, seed=100 + i, scale=1.0).to(dev) for i in range(n_frames)]
    meta = [dict(ori_shape=(shape[2], shape[3] - 11 if which == '864' else shape[3], 3), img_shape=shape[2:] + (3,), pad_shape=shape[2:] + (3,),
                 flip=False, flip_direction=None, filename='data/vid0/origin/0001.jpg')]
    stream = V.ClipStream(seg)
    with torch.no_grad():
        for i in range(n_frames):
            got = stream.push(video[i], meta, to_numpy=False)
        i = n_frames - 1
        clip = [video[f] for f in V.data.clip_indices_test(i, n_frames)]
        want = seg.simple_test(clip, meta, to_numpy=False)
        torch.cuda.synchronize()
        differ = float((got != want).float().mean())
        state = dict(i=i)

        def push():
            # (the same frame again and again, as frame i, i + 1, ...: the work of a push does not depend on the pixels)
            stream.push(video[state['i'] % n_frames], meta, to_numpy=False)
            state['i'] += 1

        def clip_path():
            seg.simple_test(clip, meta, to_numpy=False)

        us = alternate({'clip': clip_path, 'stream': push}, reps, 4)
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), shape=list(shape), kind=kind, differ=differ, us=us)), flush=True)


def run_child(step, reps):
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', step, '--reps', str(reps)], capture_output=True, text=True,
                           timeout=STEP_LIMIT[step])
    except subprocess.TimeoutExpired:
        raise SystemExit('step %s ran past its %d s limit' % (step, STEP_LIMIT[step]))
    got = [l for l in p.stdout.splitlines() if l.startswith('RESULT ')]
    if p.returncode != 0 or not got:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit('step %s failed (exit code %d)' % (step, p.returncode))
    return json.loads(got[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--child', choices=tuple(STEP_LIMIT), default=None, help='run this step in this process')
    ap.add_argument('--steps', default=','.join(STEP_LIMIT), help='comma-separated steps to run (default: all)')
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit('at least 20 repetitions')
    if a.child == 'kernel':
        return child_kernel(a.reps)
    if a.child == 'layer':
        return child_layer(a.reps)
    if a.child:
        _, which, kind = a.child.split('_')
        return child_model(which, kind, a.reps)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    steps = a.steps.split(',')
    if 'kernel' in steps:
        r = run_child('kernel', a.reps)
        say('The eval tail of a frame on %s, us per call; one repetition = every variant once, in turn' % r['device'])
        for s in r['shapes']:
            u = s['us']
            say('(N,H,W) = %s; rows equal bit for bit: %s; the three small maps: %.1f MB' % (tuple(s['shape']), s['same'], s['bytes_maps'] / 1e6))
            for k, nb in (('pair', s['bytes_pair']), ('pool', s['bytes_pool'])):
                bound = nb / HBM * 1e6
                say('  %-5s %s   %.1f MB from shapes, %.2f us at 8 TB/s, byte bound / median = %.2f' % (k, fmt(u[k]), nb / 1e6, bound, bound / u[k]['median']))
            say('  ' + verdict(u['pair'], u['pool'], 'segfuse_fwd + bn_relu_pool_fwd against segfuse_pool_fwd'))
    if 'layer' in steps:
        r = run_child('layer', a.reps)
        u = r['us']
        say()
        say('The layer at (B,H,W,depth) = %s from a 10-slot ring against gather + layer; outputs equal bit for bit: %s' % (tuple(r['shape']), r['same']))
        say('  (the gather moves %.1f MB; the ring form copies the target frame once for the residual: %.1f MB)' % (r['gather_bytes'] / 1e6, r['copy_bytes'] / 1e6))
        for k in ('gather+layer', 'ring'):
            say('  %-13s %s' % (k, fmt(u[k])))
        say('  ' + verdict(u['gather+layer'], u['ring'], 'gather + cffm_layer_infer_rows against cffm_layer_infer_rows_ring'))
    for step in steps:
        if not step.startswith('b1_'):
            continue
        r = run_child(step, a.reps)
        u = r['us']
        say()
        say('mit_b1 + B1 head on %s, stage_impl = embed_impl = %r: one frame, us (frames i >= 9); pixels where the maps differ: %.4f %%'
            % (r['shape'], r['kind'], 100 * r['differ']))
        say('  simple_test, 4-frame clip %s' % fmt(u['clip']))
        say('  ClipStream.push           %s' % fmt(u['stream']))
        say('  ' + verdict(u['clip'], u['stream'], 'clip path against streaming'))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
