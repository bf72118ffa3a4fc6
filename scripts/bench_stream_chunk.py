"""Times segmenting a video in chunks (vss_cffm_amd.ClipStream.push_many) against frame-by-frame streaming on one MI355X.

    python scripts/bench_stream_chunk.py [--reps 25] [--out profiles/stream_chunk.txt]

Step `kernel`: cffm_segfuse_pool_fwd_frames on M frames (a slot each) against M calls of cffm_segfuse_pool_fwd at N = 1 on the frames'
slices, at (H,W) = (120,216) and (120,120), maps at 1/2, 1/4 and 1/8 of the side.
Step `layer`: cffm_layer_infer_rows_ring_tables at B = M (a clip table per sample) against M calls of cffm_layer_infer_rows_ring at B = 1,
at (60,108), depth 2, a 25-slot ring of single frames.
Steps `b1_864_*`, `b1_480_*`: ClipStream.push_many of M frames (max_chunk = 16: one chunk) against M successive ClipStream.push calls of
the same frames on a stream of its own -- the path without chunks --, M = 1, 2, 4, 8, 16, mit_b1 + the B1 head at [M,3,480,864] and
[M,3,480,480], with the backbone's stage_impl / embed_impl at 'torch' and at 'hip'; label maps to the device (to_numpy=False); regular
clips only (both streams have been pushed 16 frames before anything is timed).  Figures are per FRAME: the time of the call(s) / M.

Method (as scripts/bench_stream.py): the parent never opens the GPU; each step is one child process under its own time limit and the next
starts only if the one before ended well.  Everything is warmed up first and the outputs are compared before anything is timed; one
repetition times every variant once, in turn (the variants ALTERNATE), between two device events; a figure is the median over the
repetitions, its spread the distance between the 10th and the 90th percentile.  Chunks count as faster when median(push) -
median(push_many) exceeds the sum of the two spreads.  The script reads nothing outside the tree."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_mit import alternate, fmt  # noqa: E402
from scripts.bench_stream import verdict  # noqa: E402

CHUNKS = (1, 2, 4, 8, 16)
KERNEL_SHAPES = ((120, 216), (120, 120))
MODEL_INPUTS = {'864': (3, 480, 864), '480': (3, 480, 480)}
STEP_LIMIT = {'kernel': 240, 'layer': 240, 'b1_864_torch': 420, 'b1_864_hip': 420, 'b1_480_torch': 420, 'b1_480_hip': 420}


def per_frame(us, m):
    return {k: (v / m if k != 'reps' else v) for k, v in us.items()}


def child_kernel(reps):
    import torch
    from vss_cffm_amd import _lib, ops
    dev, lib = torch.device('cuda:0'), _lib.get()
    res = []
    for h, w in KERNEL_SHAPES:
        for n in CHUNKS:
            g = torch.Generator().manual_seed(0)
            maps = [(h // 2, w // 2), (h // 4, w // 4), (h // 8, w // 8)]
            y = torch.randn(n * h * w, 256, generator=g).to(dev)
            d = torch.randn(256, generator=g).to(dev)
            z = [torch.randn(n * a * b, 256, generator=g).to(dev) for a, b in maps]
            scale, shift = (0.5 + torch.rand(256, generator=g)).to(dev), (0.3 * torch.randn(256, generator=g)).to(dev)
            ptrs = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
            zp = ptrs(z)
            zn = [ptrs([t[f * a * b:(f + 1) * a * b] for t, (a, b) in zip(z, maps)]) for f in range(n)]
            hs, ws = (C.c_int * 3)(*[a for a, _ in maps]), (C.c_int * 3)(*[b for _, b in maps])
            rows = (h // 2) * (w // 2)
            ring_a, ring_b = torch.zeros(n + 2, rows, 256, device=dev), torch.zeros(n + 2, rows, 256, device=dev)
            slots = torch.arange(1, n + 1, dtype=torch.int32).to(dev)
            one = [torch.tensor([0, 0, 0, f + 1], dtype=torch.int32).to(dev) for f in range(n)]
            st = ops._stream(y)
            yn = [y[f * h * w:(f + 1) * h * w] for f in range(n)]

            def singles():
                for f in range(n):
                    _lib.check(lib.cffm_segfuse_pool_fwd(ops._ptr(yn[f]), ops._ptr(d), zn[f], hs, ws, 3, ops._ptr(scale),
                                                         ops._ptr(shift), ops._ptr(ring_a), rows * 256, n + 2, ops._ptr(one[f]), 3, 1, h, w, st), lib)

            def frames():
                _lib.check(lib.cffm_segfuse_pool_fwd_frames(ops._ptr(y), ops._ptr(d), zp, hs, ws, 3, ops._ptr(scale), ops._ptr(shift),
                                                            ops._ptr(ring_b), rows * 256, n + 2, ops._ptr(slots), n, h, w, st), lib)

            singles()
            frames()
            torch.cuda.synchronize()
            same = bool(torch.equal(ring_a, ring_b)) and bool(ring_a[1:n + 1].abs().sum() > 0)
            us = alternate({'singles': singles, 'frames': frames}, reps, 8)
            res.append(dict(shape=[n, h, w], same=same, us={k: per_frame(v, n) for k, v in us.items()}))
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), shapes=res)), flush=True)


def child_layer(reps):
    import torch
    from scripts.bench_infer import layer_params
    from vss_cffm_amd import _lib, ops
    dev, lib = torch.device('cuda:0'), _lib.get()
    h, w, depth, r = 60, 108, 2, 25
    params = layer_params(depth, dev)
    prepared = ops.layer_prepare(depth, params)
    ring = torch.randn(r, h * w, 256, device=dev)
    res = []
    for b in CHUNKS:
        host = [[f, f + 3, f + 6, f + 9] for f in range(b)]
        tables = torch.tensor(host, dtype=torch.int32).to(dev)
        one = [torch.tensor(t, dtype=torch.int32).to(dev) for t in host]
        ws_b = torch.empty(lib.cffm_layer_infer_ws_floats(C.byref(ops.make_geom(lib, b, h, w))), device=dev)
        ws_1 = torch.empty(lib.cffm_layer_infer_ws_floats(C.byref(ops.make_geom(lib, 1, h, w))), device=dev)
        out_a, out_b = torch.empty(b, h * w, 256, device=dev), torch.empty(b, h * w, 256, device=dev)
        ring4 = ring.unsqueeze(1)

        def singles():
            for s in range(b):
                ops.cffm_layer_rows_ring(ring4, one[s], h, w, depth, params, prepared, ws=ws_1, out=out_a[s:s + 1])

        def with_tables():
            ops.cffm_layer_rows_ring_tables(ring, tables, h, w, depth, params, prepared, ws=ws_b, out=out_b)

        singles()
        with_tables()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_a, out_b))
        us = alternate({'singles': singles, 'tables': with_tables}, reps, 8)
        res.append(dict(shape=[b, h, w, depth], same=same, us={k: per_frame(v, b) for k, v in us.items()}))
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), shapes=res)), flush=True)


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
    n_frames = max(CHUNKS)
    video = torch.cat([R.synth_input('frame%d' % i, (1,) + shape, seed=100 + i, scale=1.0) for i in range(n_frames)]).to(dev)
    meta = [dict(ori_shape=(shape[1], shape[2] - 11 if which == '864' else shape[2], 3), img_shape=shape[1:] + (3,), pad_shape=shape[1:] + (3,),
                 flip=False, flip_direction=None, filename='data/vid0/origin/0001.jpg')]
    res = []
    with torch.no_grad():
        one, many = V.ClipStream(seg), V.ClipStream(seg, max_chunk=n_frames)
        for m in CHUNKS:
            # (the same frames again and again, as the next m frames of the video: the work does not depend on the pixels)
            def pushes():
                return [one.push(video[i:i + 1], meta, to_numpy=False) for i in range(m)]

            def chunk():
                return many.push_many(video[:m], meta, to_numpy=False)

            one.reset()
            many.reset()
            for i in range(n_frames):
                one.push(video[i:i + 1], meta, to_numpy=False)
            many.push_many(video, meta, to_numpy=False)
            want, got = torch.cat(pushes()), chunk()                # the same m frames behind the same 16 on both streams
            torch.cuda.synchronize()
            differ = float((got != want).float().mean())
            us = alternate({'push': pushes, 'push_many': chunk}, reps, 2)
            res.append(dict(m=m, differ=differ, us={k: per_frame(v, m) for k, v in us.items()}))
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), shape=list(shape), kind=kind, chunks=res)), flush=True)


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
        say('The eval tail of M frames on %s, us per FRAME; one repetition = every variant once, in turn' % r['device'])
        for s in r['shapes']:
            u = s['us']
            say('(M,H,W) = %s; rings equal bit for bit: %s' % (tuple(s['shape']), s['same']))
            say('  M x segfuse_pool_fwd (N = 1)   %s' % fmt(u['singles']))
            say('  segfuse_pool_fwd_frames        %s' % fmt(u['frames']))
            say('  ' + verdict(u['singles'], u['frames'], 'M single-frame calls against one call with a slot per frame'))
    if 'layer' in steps:
        r = run_child('layer', a.reps)
        say()
        say('The layer on a 25-slot ring of single frames, us per FRAME (sample)')
        for s in r['shapes']:
            u = s['us']
            say('(B,H,W,depth) = %s; outputs equal bit for bit: %s' % (tuple(s['shape']), s['same']))
            say('  B x layer_infer_rows_ring (B = 1)   %s' % fmt(u['singles']))
            say('  layer_infer_rows_ring_tables        %s' % fmt(u['tables']))
            say('  ' + verdict(u['singles'], u['tables'], 'B single-sample calls against one call with a table per sample'))
    for step in steps:
        if not step.startswith('b1_'):
            continue
        r = run_child(step, a.reps)
        say()
        say('mit_b1 + B1 head on [M,%s], stage_impl = embed_impl = %r: us per FRAME (regular clips)' % (', '.join(map(str, r['shape'])), r['kind']))
        for c in r['chunks']:
            u = c['us']
            say('M = %d; pixels where the maps differ: %.4f %%' % (c['m'], 100 * c['differ']))
            say('  M x ClipStream.push       %s' % fmt(u['push']))
            say('  ClipStream.push_many      %s' % fmt(u['push_many']))
            say('  ' + verdict(u['push'], u['push_many'], 'frame by frame against one chunk'))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
