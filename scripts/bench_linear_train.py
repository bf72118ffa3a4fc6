"""Times vss_cffm_amd.linear_rows, forward + backward, against the stock PyTorch lines it replaces, and a mit_b1 training pass with
MixVisionTransformer.linear_impl 'hip' against 'torch', on one MI355X.

    python scripts/bench_linear_train.py [--reps 25] [--out profiles/linear_train.txt]

Step 1, the layers: the five Linear layers of a mit_b1 block on [8,3,480,480], each at the stage named -- q (64 -> 64), proj (64 -> 64,
residual + DropPath) and fc2 (256 -> 64, residual + DropPath) at stage 1 (M = 8 x 14400 rows), fc1 (128 -> 512) at stage 2 (M = 8 x 3600),
kv (320 -> 640) at stage 3 on the reduced map (M = 8 x 225) -- forward + backward with x, weight, bias (and the residual) requiring grad.
'torch' is ``F.linear`` and, for proj / fc2, the reference's line ``r + drop_path(F.linear(x, w, b))`` with DropPath(0.1) in train mode;
'hip' is ``linear_rows`` with the factor drawn as the backbone draws it (``backbone._drop_scale``), so both sides pay for their torch.rand.
Next to each: the bytes one pass must move at 8 TB/s (forward: x, y and the residual once; backward: dy, x and dx once) and the three
products' MFMA time at 833 TF (2 M N K flops per product: the three-pass split at 2.5 PF / 3).
Step 2, the model: mit_b1 in train mode on [8,3,480,480], forward + backward, `linear_impl` 'torch' against 'hip' with `norm_impl` 'hip' on
both sides and `dwconv_impl`, `attn_impl`, `sr_impl`, `conv_impl` at their defaults; at drop path 0.1 (what every reference config trains
with) and at 0; peak allocated memory of one pass beyond what was allocated before it; the largest |hip - torch| / max|torch| of the four
outputs at drop path 0.
Step 3, repeatability: 25 iterations of two training passes each (drop path 0, `norm_impl`, `conv_impl` and `sr_impl` 'hip' so that no stock
kernel with atomics feeds the Linear backwards, `linear_impl` 'hip'); the Linear weight and bias gradients of the two passes are compared bit
for bit.

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

# name -> (samples, rows per sample, in features, out features, residual + DropPath)
LAYERS = {'q (stage 1)': (8, 14400, 64, 64, False), 'proj (stage 1)': (8, 14400, 64, 64, True), 'fc2 (stage 1)': (8, 14400, 256, 64, True),
          'fc1 (stage 2)': (8, 3600, 128, 512, False), 'kv (stage 3)': (8, 225, 320, 640, False)}
MODEL_INPUT = (8, 3, 480, 480)
STEP_LIMIT = {'layers': 300, 'model': 360, 'repeat': 360}            # seconds per child process
HBM, MFMA = 8e12, 833e12                                              # bytes per second, flops per second of the three-pass product
DROP = 0.1


def child_layers(reps):
    import torch
    import torch.nn.functional as F
    import vss_cffm_amd as V
    from vss_cffm_amd import backbone as B
    dev = torch.device('cuda:0')
    res = {}
    for name, (nb, rps, k, n, tail) in LAYERS.items():
        g = torch.Generator().manual_seed(0)
        x = torch.randn(nb, rps, k, generator=g).to(dev).requires_grad_(True)
        w = (0.05 * torch.randn(n, k, generator=g)).to(dev).requires_grad_(True)
        b = (0.3 * torch.randn(n, generator=g)).to(dev).requires_grad_(True)
        r = torch.randn(nb, rps, n, generator=g).to(dev).requires_grad_(True) if tail else None
        dy = torch.randn(nb, rps, n, generator=g).to(dev)
        dp = B.DropPath(DROP).train()

        def stock():
            y = F.linear(x, w, b)
            return r + dp(y) if tail else y

        def hip():
            return V.linear_rows(x, w, b, r, B._drop_scale(dp, x) if tail else None)

        def both(fn):
            def run():
                for t in (x, w, b, r):
                    if t is not None:
                        t.grad = None
                fn().backward(dy)
            return run

        fns = {'torch': both(stock), 'hip': both(hip)}
        torch.cuda.synchronize()
        us = alternate(fns, reps, 8)
        m = nb * rps
        res[name] = dict(M=m, K=k, N=n, us=us, bytes=4 * (m * k + m * n * (2 if tail else 1)) + 4 * (m * n + 2 * m * k), flops=3 * 2 * m * n * k)
        del x, w, b, r, dy, fns
        torch.cuda.empty_cache()
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), layers=res)), flush=True)


def _model(norm='hip', conv='torch'):
    import torch
    import vss_cffm_amd as V
    from oracle import recipe as R
    dev = torch.device('cuda:0')
    m = V.build_backbone(dict(type='mit_b1', style='pytorch'))
    m.load_state_dict(R.synth_state(m, seed=40), strict=True)
    m.to(dev).train()
    m.set_norm_impl(norm)
    m.set_conv_impl(conv)
    return m, R.synth_input('img', MODEL_INPUT, seed=41, scale=1.0).to(dev)


def child_model(reps):
    import torch
    m, img = _model()

    def with_impl(kind, rate, fn):
        def run():
            m.set_linear_impl(kind)
            m.reset_drop_path(rate)
            return fn()
        return run

    def fwd():
        with torch.no_grad():
            return m(img)

    def fwd_bwd():
        for p in m.parameters():
            p.grad = None
        sum(o.square().mean() for o in m(img)).backward()

    outs = {k: [o.clone() for o in with_impl(k, 0., fwd)()] for k in ('torch', 'hip')}
    err = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(outs['hip'], outs['torch'])]
    del outs
    fns = {'%s_fwd_bwd drop path %g' % (k, rate): with_impl(k, rate, fwd_bwd) for rate in (DROP, 0.) for k in ('torch', 'hip')}
    mem = {k: peak_extra(fn) for k, fn in fns.items()}
    us = alternate(fns, reps, 1)
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), rel_err_hip_vs_torch=err, mem=mem, us=us)), flush=True)


def child_repeat(reps):
    import torch
    import torch.nn as nn
    m, img = _model(conv='hip')
    m.set_linear_impl('hip')
    m.reset_drop_path(0.)
    for mod in m.modules():                 # (no MIOpen convolution left in the pass: DESIGN 3w)
        if hasattr(type(mod), 'sr_impl'):
            mod.sr_impl = 'hip'
    names = [n + '.' + p for n, mod in m.named_modules() if isinstance(mod, nn.Linear) for p, t in mod.named_parameters(recurse=False)]
    params = dict(m.named_parameters())

    def grads():
        for p in m.parameters():
            p.grad = None
        sum(o.square().mean() for o in m(img)).backward()
        return {n: params[n].grad.clone() for n in names}

    differing = set()
    for _ in range(reps):
        a, b = grads(), grads()
        differing |= {n for n in names if not torch.equal(a[n], b[n])}
    print('RESULT ' + json.dumps(dict(iterations=reps, tensors=len(names), differing=sorted(differing))), flush=True)


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
        return {'layers': child_layers, 'model': child_model, 'repeat': child_repeat}[a.child](a.reps)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    r = run_child('layers', a.reps)
    say('linear_rows against the stock lines on %s, forward + backward, us per call; one repetition = every variant once, in turn' % r['device'])
    for name, s in r['layers'].items():
        u, bb, fb = s['us'], s['bytes'] / HBM * 1e6, s['flops'] / MFMA * 1e6
        say('%s: M = %d, %d -> %d: %.1f MB = %.2f us at 8 TB/s, three products = %.2f us at 833 TF' % (name, s['M'], s['K'], s['N'], s['bytes'] / 1e6, bb, fb))
        say('    %-6s %s   max(byte, MFMA floor) / median = %.2f' % ('hip', fmt(u['hip']), max(bb, fb) / u['hip']['median']))
        say('    %-6s %s' % ('torch', fmt(u['torch'])))
        say('    %s' % verdict(u['torch'], u['hip']))
    r = run_child('model', a.reps)
    u, mem = r['us'], r['mem']
    say()
    say('mit_b1 on %s, train mode, forward + backward, linear_impl hip against torch (norm_impl hip on both sides; dwconv_impl, attn_impl, sr_impl, '
        'conv_impl at their defaults), us per pass' % (list(MODEL_INPUT),))
    say('  largest |hip - torch| / max|torch| of the four outputs (drop path 0): %s' % ', '.join('%.1e' % e for e in r['rel_err_hip_vs_torch']))
    for rate in (DROP, 0.):
        t, h = 'torch_fwd_bwd drop path %g' % rate, 'hip_fwd_bwd drop path %g' % rate
        for k in (t, h):
            say('  %-28s %s   peak memory %8.1f MB' % (k, fmt(u[k]), mem[k] / 1e6))
        say('  drop path %g: %s' % (rate, verdict(u[t], u[h])))
    r = run_child('repeat', a.reps)
    say()
    say('repeatability: %d iterations of two mit_b1 training passes (norm_impl, conv_impl, sr_impl, linear_impl hip, drop path 0): of the %d Linear weight and '
        'bias gradients, %d differ between the two passes in some iteration%s' % (r['iterations'], r['tensors'], len(r['differing']),
                                                                               ': ' + ', '.join(r['differing']) if r['differing'] else ''))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
