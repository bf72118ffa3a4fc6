"""Times the fused spatial-reduction attention core (vss_cffm_amd.sra_attention) and the whole mit_b1 backbone on one MI355X against the
reference's op sequence in stock PyTorch on the same device.

    python scripts/bench_sra.py [--reps 25] [--out profiles/sra_attention.txt]

Step 1, the core: forward and forward + backward at the four attention shapes of mit_b1 at the training shape (8 frames of 480 x 480),
(B, heads, N, Nk, hd) = (8,1,14400,225,64), (8,2,3600,225,64), (8,5,900,225,64), (8,8,225,225,64).  'torch' is reshape / permute,
q @ k^T, * scale, softmax, attn @ v, transpose / reshape with autograd, as Attention.attn_impl = 'torch' runs it.  The backward's time is
(forward + backward) - forward of the same variant.  Compute floor: 4 B N Nk C FLOP (the two products of the forward) at the 155 TF
measured for the f32-input MFMA; the backward as built has seven products (k_sra_bwd_dq three, k_sra_bwd_dkv four), five at the least.
Also: the peak memory of one call beyond what was allocated before it.
Step 2, the model: mit_b1 on [8,3,480,480], forward under no_grad and forward + backward, Attention.attn_impl 'hip' against 'torch' with
Mlp.dwconv_impl = 'hip' in both, with the peak allocated memory of one call.

Method (as scripts/bench_mit.py): the parent process never opens the GPU; each step is one child process under its own time limit,
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

SHAPES = ((8, 1, 14400, 225, 64), (8, 2, 3600, 225, 64), (8, 5, 900, 225, 64), (8, 8, 225, 225, 64))
MODEL_INPUT = (8, 3, 480, 480)
STEP_LIMIT = {'kernel': 300, 'model': 420}          # seconds per child process
MFMA_F32 = 155e12                                    # FLOP per second, f32-input MFMA as measured


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


def peak_extra(fn):
    import torch
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
    import vss_cffm_amd as V
    dev = torch.device('cuda:0')
    res = []
    for b, heads, n, nk, hd in SHAPES:
        c, scale = heads * hd, hd ** -0.5
        g = torch.Generator().manual_seed(0)
        q = torch.randn(b, n, c, generator=g).to(dev).requires_grad_(True)
        kv = torch.randn(b, nk, 2 * c, generator=g).to(dev).requires_grad_(True)
        dout = torch.randn(b, n, c, generator=g).to(dev)

        def seq():
            qh = q.reshape(b, n, heads, hd).permute(0, 2, 1, 3)
            k, v = kv.reshape(b, -1, 2, heads, hd).permute(2, 0, 3, 1, 4)
            attn = ((qh @ k.transpose(-2, -1)) * scale).softmax(dim=-1)
            return (attn @ v).transpose(1, 2).reshape(b, n, c)

        def hip():
            return V.sra_attention(q, kv, heads, scale)

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        def both(fn):
            def run():
                q.grad = kv.grad = None
                fn().backward(dout)
            return run

        both(seq)()
        want = (seq().detach(), q.grad.clone(), kv.grad.clone())
        both(hip)()
        got = (hip().detach(), q.grad.clone(), kv.grad.clone())
        torch.cuda.synchronize()
        err = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(got, want)]
        del want, got
        fns = {'torch_fwd': no_grad(seq), 'hip_fwd': no_grad(hip), 'torch_fwd_bwd': both(seq), 'hip_fwd_bwd': both(hip)}
        q.grad = kv.grad = None
        mem = {k: peak_extra(fn) for k, fn in fns.items()}
        us = alternate(fns, reps, 4)
        res.append(dict(shape=[b, heads, n, nk, hd], rel_err_vs_torch=err, us=us, mem=mem, fwd_flop=4.0 * b * n * nk * c))
        del q, kv, dout
        torch.cuda.empty_cache()
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), shapes=res)), flush=True)


def child_model(reps):
    import torch
    import vss_cffm_amd as V
    from oracle import recipe as R
    from vss_cffm_amd import backbone as B
    dev = torch.device('cuda:0')
    B.Mlp.dwconv_impl = 'hip'
    m = V.build_backbone(dict(type='mit_b1', style='pytorch'))
    m.load_state_dict(R.synth_state(m, seed=40), strict=True)
    m.reset_drop_path(0.)                              # both variants the same deterministic network
    m.to(dev).train()
    img = R.synth_input('img', MODEL_INPUT, seed=41, scale=1.0).to(dev)

    def with_impl(kind, fn):
        def run():
            B.Attention.attn_impl = kind
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
    say('Spatial-reduction attention core (q k^T, scale, softmax, attn v on the Linear layers\' layouts) on %s, us per call; one repetition = '
        'every variant once, in turn' % r['device'])
    for s in r['shapes']:
        u, mem = s['us'], s['mem']
        say('shape (B,heads,N,Nk,hd) = %s; largest |hip - torch| / max|torch| of out, dq, dkv: %s' % (
            tuple(s['shape']), ', '.join('%.1e' % e for e in s['rel_err_vs_torch'])))
        for k in ('torch_fwd', 'hip_fwd', 'torch_fwd_bwd', 'hip_fwd_bwd'):
            say('  %-14s %s   peak extra memory %8.1f MB' % (k, fmt(u[k]), mem[k] / 1e6))
        floor = s['fwd_flop'] / MFMA_F32 * 1e6
        say('  forward: %s; compute floor %.1f us (%.2f GFLOP at 155 TF) -> hip runs at %.2f of it' % (
            verdict(u['torch_fwd'], u['hip_fwd']), floor, s['fwd_flop'] / 1e9, floor / u['hip_fwd']['median']))
        bwd = {k: u[k + '_fwd_bwd']['median'] - u[k + '_fwd']['median'] for k in ('torch', 'hip')}
        say('  forward + backward: %s' % verdict(u['torch_fwd_bwd'], u['hip_fwd_bwd']))
        say('  backward alone (difference of the medians): torch %.1f us, hip %.1f us; compute floor of the seven products as built %.1f us '
            '-> hip runs at %.2f of it' % (bwd['torch'], bwd['hip'], 3.5 * floor, 3.5 * floor / max(bwd['hip'], 1e-9)))
    r = run_child('model', a.reps)
    u, mem = r['us'], r['mem']
    say()
    say('mit_b1 on %s (train mode, drop path 0, Mlp.dwconv_impl hip), Attention.attn_impl hip against torch, us per call; largest '
        '|hip - torch| / max|torch| of the four outputs: %s' % (list(MODEL_INPUT), ', '.join('%.1e' % e for e in r['rel_err_hip_vs_torch'])))
    for k in ('torch_fwd', 'hip_fwd', 'torch_fwd_bwd', 'hip_fwd_bwd'):
        say('  %-14s %s   peak memory %8.1f MB' % (k, fmt(u[k]), mem[k] / 1e6))
    say('  forward (no_grad): %s' % verdict(u['torch_fwd'], u['hip_fwd']))
    say('  forward + backward: %s' % verdict(u['torch_fwd_bwd'], u['hip_fwd_bwd']))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
