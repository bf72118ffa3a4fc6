"""Times the three differentiable LayerNorms (vss_cffm_amd.layer_norm_rows / nchw_layer_norm_rows / layer_norm_rows_nchw), forward +
backward, against the stock PyTorch sequences they replace, and a mit_b1 training pass with MixVisionTransformer.norm_impl 'hip' against
'torch', on one MI355X.

    python scripts/bench_ln_train.py [--reps 25] [--out profiles/ln_train.txt]

Step 1, the kernels: each form at the four stage shapes of mit_b1 on [8,3,480,480] -- (8,64,120,120), (8,128,60,60), (8,320,30,30),
(8,512,15,15) -- forward alone (under no_grad) and forward + backward with x, weight and bias requiring grad, next to the bytes the
library's kernels move at 8 TB/s: 8 per element forward (one read, one write), 12 more backward (x and dout read, dx written; the
dweight / dbias records are small beside them).
Step 2, the model: mit_b1 in train mode (drop path 0) on [8,3,480,480], forward + backward, `norm_impl` 'torch' against 'hip' with
`dwconv_impl`, `attn_impl` and `sr_impl` at their defaults; peak allocated memory of one pass beyond what was allocated before it; the
largest |hip - torch| / max|torch| of the four outputs.

Method (as scripts/bench_mit.py): the parent process never opens the GPU; each step is one child process under its own time limit, and
the next starts only if the one before ended well.  Everything is warmed up first; one repetition times every variant once, in turn (the
variants ALTERNATE), between two device events; the figure of a variant is the median over the repetitions, its spread the distance
between the 10th and the 90th percentile.  'hip' counts as faster when median(torch) - median(hip) exceeds the sum of the two spreads.
The script reads nothing outside the tree."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_mit import alternate, fmt, peak_extra, verdict  # noqa: E402

SHAPES = ((8, 64, 120, 120), (8, 128, 60, 60), (8, 320, 30, 30), (8, 512, 15, 15))     # (B, C, H, W): the stages of mit_b1 on [8,3,480,480]
MODEL_INPUT = (8, 3, 480, 480)
STEP_LIMIT = {'kernels': 300, 'model': 360}            # seconds per child process
HBM = 8e12                                             # bytes per second
FORMS = ('layer_norm_rows', 'nchw_layer_norm_rows', 'layer_norm_rows_nchw')
EPS = 1e-6


def child_kernels(reps):
    import torch
    import torch.nn.functional as F
    import vss_cffm_amd as V
    dev = torch.device('cuda:0')
    res = []
    for b, c, h, w in SHAPES:
        g = torch.Generator().manual_seed(0)
        img = (1.5 * torch.randn(b, c, h, w, generator=g) + 2.0).to(dev).requires_grad_(True)
        rows = img.detach().flatten(2).transpose(1, 2).contiguous().requires_grad_(True)
        gam = (1 + 0.3 * torch.randn(c, generator=g)).to(dev).requires_grad_(True)
        bet = (0.3 * torch.randn(c, generator=g)).to(dev).requires_grad_(True)
        d_rows, d_img = torch.randn(b, h * w, c, generator=g).to(dev), torch.randn(b, c, h, w, generator=g).to(dev)
        # form -> (input, dout, the library's function, the stock sequence)
        forms = {
            'layer_norm_rows': (rows, d_rows, lambda: V.layer_norm_rows(rows, gam, bet, EPS), lambda: F.layer_norm(rows, (c,), gam, bet, EPS)),
            'nchw_layer_norm_rows': (img, d_rows, lambda: V.nchw_layer_norm_rows(img, gam, bet, EPS),
                                     lambda: F.layer_norm(img.flatten(2).transpose(1, 2), (c,), gam, bet, EPS)),
            'layer_norm_rows_nchw': (rows, d_img, lambda: V.layer_norm_rows_nchw(rows, gam, bet, h, w, EPS),
                                     lambda: F.layer_norm(rows, (c,), gam, bet, EPS).reshape(b, h, w, c).permute(0, 3, 1, 2).contiguous()),
        }

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        def both(fn, x, dout):
            def run():
                x.grad = gam.grad = bet.grad = None
                fn().backward(dout)
            return run

        fns, err = {}, {}
        for name, (x, dout, hip, seq) in forms.items():
            both(seq, x, dout)()
            want = (seq().detach(), x.grad.clone(), gam.grad.clone(), bet.grad.clone())
            both(hip, x, dout)()
            got = (hip().detach(), x.grad.clone(), gam.grad.clone(), bet.grad.clone())
            err[name] = [float((p - q).abs().max() / q.abs().max()) for p, q in zip(got, want)]
            fns.update({'torch_fwd ' + name: no_grad(seq), 'hip_fwd ' + name: no_grad(hip),
                        'torch_fwd_bwd ' + name: both(seq, x, dout), 'hip_fwd_bwd ' + name: both(hip, x, dout)})
        torch.cuda.synchronize()
        us = alternate(fns, reps, 8)
        res.append(dict(shape=[b, c, h, w], rel_err_vs_torch=err, us=us, fwd_bytes=8 * img.numel(), bwd_bytes=12 * img.numel()))
        del forms, fns, img, rows, d_rows, d_img
        torch.cuda.empty_cache()
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), shapes=res)), flush=True)


def child_model(reps):
    import torch
    import vss_cffm_amd as V
    from oracle import recipe as R
    dev = torch.device('cuda:0')
    m = V.build_backbone(dict(type='mit_b1', style='pytorch'))
    m.load_state_dict(R.synth_state(m, seed=40), strict=True)
    m.reset_drop_path(0.)                              # both variants the same deterministic network
    m.to(dev).train()
    img = R.synth_input('img', MODEL_INPUT, seed=41, scale=1.0).to(dev)

    def with_impl(kind, fn):
        def run():
            m.set_norm_impl(kind)
            return fn()
        return run

    def fwd():
        with torch.no_grad():
            return m(img)

    def fwd_bwd():
        for p in m.parameters():
            p.grad = None
        sum(o.square().mean() for o in m(img)).backward()

    outs = {k: [o.clone() for o in with_impl(k, fwd)()] for k in ('torch', 'hip')}
    err = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(outs['hip'], outs['torch'])]
    del outs
    fns = {'%s_%s' % (k, name): with_impl(k, fn) for name, fn in (('fwd', fwd), ('fwd_bwd', fwd_bwd)) for k in ('torch', 'hip')}
    mem = {k: peak_extra(fn) for k, fn in fns.items()}
    us = alternate(fns, reps, 1)
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), rel_err_hip_vs_torch=err, mem=mem, us=us)), flush=True)


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
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit('at least 20 repetitions')
    if a.child:
        return {'kernels': child_kernels, 'model': child_model}[a.child](a.reps)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    r = run_child('kernels', a.reps)
    say('The differentiable LayerNorms against the stock sequences on %s, us per call; one repetition = every variant once, in turn' % r['device'])
    for s in r['shapes']:
        u, fb, bb = s['us'], s['fwd_bytes'] / HBM * 1e6, (s['fwd_bytes'] + s['bwd_bytes']) / HBM * 1e6
        say('map (B,C,H,W) = %s: forward %.1f MB = %.2f us at 8 TB/s, forward + backward %.1f MB = %.2f us' % (
            tuple(s['shape']), s['fwd_bytes'] / 1e6, fb, (s['fwd_bytes'] + s['bwd_bytes']) / 1e6, bb))
        for k in FORMS:
            say('  %s   max|hip - torch| / max|torch| of out, dx, dweight, dbias: %s' % (k, ', '.join('%.1e' % e for e in s['rel_err_vs_torch'][k])))
            for kind, bound in (('fwd', fb), ('fwd_bwd', bb)):
                say('    %-14s %s   byte bound / median = %.2f' % ('hip_' + kind, fmt(u['hip_%s %s' % (kind, k)]), bound / u['hip_%s %s' % (kind, k)]['median']))
                say('    %-14s %s' % ('torch_' + kind, fmt(u['torch_%s %s' % (kind, k)])))
            say('    fwd + bwd: %s' % verdict(u['torch_fwd_bwd ' + k], u['hip_fwd_bwd ' + k]))
    r = run_child('model', a.reps)
    u, mem = r['us'], r['mem']
    say()
    say('mit_b1 on %s, train mode, norm_impl hip against torch (dwconv_impl, attn_impl, sr_impl at their defaults), us per pass' % (list(MODEL_INPUT),))
    say('  largest |hip - torch| / max|torch| of the four outputs: %s' % ', '.join('%.1e' % e for e in r['rel_err_hip_vs_torch']))
    for k in ('torch_fwd', 'hip_fwd', 'torch_fwd_bwd', 'hip_fwd_bwd'):
        say('  %-14s %s   peak memory %8.1f MB' % (k, fmt(u[k]), mem[k] / 1e6))
    say('  forward (no_grad): %s' % verdict(u['torch_fwd'], u['hip_fwd']))
    say('  forward + backward: %s' % verdict(u['torch_fwd_bwd'], u['hip_fwd_bwd']))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
