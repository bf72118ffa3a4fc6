"""Times the fused spatial-reduction convolution + LayerNorm (vss_cffm_amd.sr_reduce) and the whole mit_b1 backbone on one MI355X against
the reference's op sequence in stock PyTorch on the same device.

    python scripts/bench_sr.py [--reps 25] [--out profiles/sr_reduce.txt]

Step 1, the kernel: forward and forward + backward at the three reducing stages of mit_b1 at the training shape (8 frames of 480 x 480),
(B, H, W, C, s) = (8,120,120,64,8), (8,60,60,128,4), (8,30,30,320,2).  'torch' is permute / reshape, Conv2d(C, C, s, s), reshape /
permute, LayerNorm with autograd, as Attention.sr_impl = 'torch' runs it; both variants are eager calls through autograd.  The backward's
time is (forward + backward) - forward of the same variant.  Floors: bytes = x once (plus dx once in the backward) at the nominal 8 TB/s
(this project has seen about 5.6 TB/s); compute = 2 M K N FLOP per product (M = B Ho Wo, K = s s C, N = C) at the 155 TF measured for the
f32-input MFMA, one product forward and two backward.  Also: the peak memory of one call beyond what was allocated before it, every variant
starting with no gradient held (a forward + backward figure includes the gradients it leaves).
Step 2, the model: mit_b1 on [8,3,480,480], forward under no_grad and forward + backward, Attention.sr_impl 'hip' against 'torch' with
Mlp.dwconv_impl = Attention.attn_impl = 'hip' in both, with the peak allocated memory of one call.

Method (as scripts/bench_sra.py): the parent process never opens the GPU; each step is one child process under its own time limit,
and the second starts only if the first ended well.  Everything is warmed up first; one repetition times every variant once, in turn
(the variants ALTERNATE), between two device events; the figure of a variant is the median over the repetitions, its spread the
distance between the 10th and the 90th percentile.  'hip' counts as faster when median(torch) - median(hip) exceeds the sum of the two
spreads."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((8, 120, 120, 64, 8), (8, 60, 60, 128, 4), (8, 30, 30, 320, 2))
MODEL_INPUT = (8, 3, 480, 480)
STEP_LIMIT = {'kernel': 300, 'model': 420}          # seconds per child process
MFMA_F32 = 155e12                                    # FLOP per second, f32-input MFMA as measured
HBM_NOMINAL, HBM_SEEN = 8e12, 5.6e12                # bytes per second


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, max(0, int(round(q * (len(v) - 1)))))]


def summary(v):
    return dict(median=pct(v, 0.5), p10=pct(v, 0.1), p90=pct(v, 0.9), min=min(v), max=max(v), reps=len(v))


def timed(fn, inner):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner          # us per call


def peak_extra(fn, clear):
    """peak allocation of one call beyond what was allocated before it; `clear` drops the gradients an earlier call left, so that every
    variant starts from the same state (a forward + backward figure includes the gradients it leaves behind)"""
    import torch
    clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def alternate(fns, reps, inner):
    for _ in range(3):
        for fn in fns.values():
            fn()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, inner))
    return {k: summary(v) for k, v in t.items()}


def child_kernel(reps):
    import torch
    import torch.nn.functional as F
    import vss_cffm_amd as V
    dev = torch.device('cuda:0')
    res = []
    for b, h, w, c, s in SHAPES:
        g = torch.Generator().manual_seed(0)
        x = torch.randn(b, h * w, c, generator=g).to(dev).requires_grad_(True)
        wt = (torch.randn(c, c, s, s, generator=g) / (s * s * c) ** 0.5).to(dev).requires_grad_(True)
        bias = torch.randn(c, generator=g).to(dev).requires_grad_(True)
        gamma = (1 + 0.1 * torch.randn(c, generator=g)).to(dev).requires_grad_(True)
        beta = (0.1 * torch.randn(c, generator=g)).to(dev).requires_grad_(True)
        m = b * (h // s) * (w // s)
        dout = torch.randn(b, m // b, c, generator=g).to(dev)
        leaves = (x, wt, bias, gamma, beta)

        def seq():
            y = F.conv2d(x.permute(0, 2, 1).reshape(b, c, h, w), wt, bias, stride=s).reshape(b, c, -1).permute(0, 2, 1)
            return F.layer_norm(y, (c,), gamma, beta, 1e-5)

        def hip():
            return V.sr_reduce(x, wt, bias, gamma, beta, h, w, s, 1e-5)

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        def both(fn):
            def run():
                for t in leaves:
                    t.grad = None
                fn().backward(dout)
            return run

        both(seq)()
        want = (seq().detach(),) + tuple(t.grad.clone() for t in leaves)
        both(hip)()
        got = (hip().detach(),) + tuple(t.grad.clone() for t in leaves)
        torch.cuda.synchronize()
        err = [float((a - y).abs().max() / y.abs().max()) for a, y in zip(got, want)]
        del want, got
        fns = {'torch_fwd': no_grad(seq), 'hip_fwd': no_grad(hip), 'torch_fwd_bwd': both(seq), 'hip_fwd_bwd': both(hip)}
        def clear():
            for t in leaves:
                t.grad = None

        mem = {k: peak_extra(fn, clear) for k, fn in fns.items()}
        clear()
        us = alternate(fns, reps, 4)
        res.append(dict(shape=[b, h, w, c, s], rel_err_vs_torch=err, us=us, mem=mem, flop=2.0 * m * s * s * c * c, x_bytes=4.0 * b * h * w * c))
        del x, wt, bias, gamma, beta, dout, leaves
        torch.cuda.empty_cache()
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), shapes=res)), flush=True)


def child_model(reps):
    import torch
    import vss_cffm_amd as V
    from oracle import recipe as R
    from vss_cffm_amd import backbone as B
    dev = torch.device('cuda:0')
    B.Mlp.dwconv_impl = B.Attention.attn_impl = 'hip'
    m = V.build_backbone(dict(type='mit_b1', style='pytorch'))
    m.load_state_dict(R.synth_state(m, seed=40), strict=True)
    m.reset_drop_path(0.)                              # both variants the same deterministic network
    m.to(dev).train()
    img = R.synth_input('img', MODEL_INPUT, seed=41, scale=1.0).to(dev)

    def with_impl(kind, fn):
        def run():
            B.Attention.sr_impl = kind
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
    def clear():
        for p in m.parameters():
            p.grad = None

    mem = {k: peak_extra(fn, clear) for k, fn in fns.items()}
    clear()
    us = alternate(fns, reps, 1)
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), rel_err_hip_vs_torch=err, mem=mem, us=us)), flush=True)


def fmt(s):
    return 'median %9.1f  p10 %9.1f  p90 %9.1f  (%d reps)' % (s['median'], s['p10'], s['p90'], s['reps'])


def verdict(t, h):
    gain, spread = t['median'] - h['median'], (t['p90'] - t['p10']) + (h['p90'] - h['p10'])
    return 'torch / hip = %.2f, torch - hip = %.1f us against a sum of spreads of %.1f us -> hip faster beyond the spreads: %s' % (
        t['median'] / h['median'], gain, spread, 'yes' if gain > spread else 'NO')


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
    ap.add_argument('--child', choices=('kernel', 'model'), default=None, help='run this step in this process')
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit('at least 20 repetitions')
    if a.child:
        return {'kernel': child_kernel, 'model': child_model}[a.child](a.reps)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    r = run_child('kernel', a.reps)
    say('Spatial-reduction Conv2d(C, C, s, s) + LayerNorm on token rows on %s, us per call (eager, through autograd); one repetition = every '
        'variant once, in turn' % r['device'])
    for s in r['shapes']:
        u, mem = s['us'], s['mem']
        say('shape (B,H,W,C,s) = %s; largest |hip - torch| / max|torch| of out, dx, dw, db, dgamma, dbeta: %s' % (
            tuple(s['shape']), ', '.join('%.1e' % e for e in s['rel_err_vs_torch'])))
        for k in ('torch_fwd', 'hip_fwd', 'torch_fwd_bwd', 'hip_fwd_bwd'):
            say('  %-14s %s   peak extra memory %8.1f MB' % (k, fmt(u[k]), mem[k] / 1e6))
        cf, bf, bs = s['flop'] / MFMA_F32 * 1e6, s['x_bytes'] / HBM_NOMINAL * 1e6, s['x_bytes'] / HBM_SEEN * 1e6
        say('  forward: %s' % verdict(u['torch_fwd'], u['hip_fwd']))
        say('    floors: bytes %.1f us (x once at 8 TB/s; %.1f us at the 5.6 TB/s seen), compute %.1f us (%.2f GFLOP at 155 TF) -> hip runs '
            'at %.2f of the larger' % (bf, bs, cf, s['flop'] / 1e9, max(bf, cf) / u['hip_fwd']['median']))
        bwd = {k: u[k + '_fwd_bwd']['median'] - u[k + '_fwd']['median'] for k in ('torch', 'hip')}
        say('  forward + backward: %s' % verdict(u['torch_fwd_bwd'], u['hip_fwd_bwd']))
        say('  backward alone (difference of the medians): torch %.1f us, hip %.1f us' % (bwd['torch'], bwd['hip']))
        say('    floors: bytes %.1f us (x and dx once at 8 TB/s; %.1f us at 5.6 TB/s), compute %.1f us (two products) -> hip runs at %.2f of '
            'the larger' % (2 * bf, 2 * bs, 2 * cf, max(2 * bf, 2 * cf) / max(bwd['hip'], 1e-9)))
    r = run_child('model', a.reps)
    u, mem = r['us'], r['mem']
    say()
    say('mit_b1 on %s (train mode, drop path 0, Mlp.dwconv_impl and Attention.attn_impl hip), Attention.sr_impl hip against torch, us per '
        'call; largest |hip - torch| / max|torch| of the four outputs: %s' % (list(MODEL_INPUT), ', '.join('%.1e' % e for e in r['rel_err_hip_vs_torch'])))
    for k in ('torch_fwd', 'hip_fwd', 'torch_fwd_bwd', 'hip_fwd_bwd'):
        say('  %-14s %s   peak memory %8.1f MB' % (k, fmt(u[k]), mem[k] / 1e6))
    say('  forward (no_grad): %s' % verdict(u['torch_fwd'], u['hip_fwd']))
    say('  forward + backward: %s' % verdict(u['torch_fwd_bwd'], u['hip_fwd_bwd']))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
