"""Times the differentiable patch embedding (vss_cffm_amd.overlap_patch_embed), forward + backward, against the stock PyTorch sequence it
replaces (Conv2d, flatten / transpose, LayerNorm), and a mit_b1 training pass with MixVisionTransformer.conv_impl 'hip' against 'torch', on
one MI355X.

    python scripts/bench_patch_embed_train.py [--reps 25] [--out profiles/patch_embed_train.txt]

Step 1, the embeddings: the four of mit_b1 on [8,3,480,480], each alone, forward + backward with every parameter requiring grad and -- stages
2 to 4 -- the input as well (stage 1's input is the image).  Next to them the three passes of the library's call timed by themselves through
the C ABI: the training forward, the backward without dx (LayerNorm backward, dw slabs, db, finalize) and, as the difference to the backward
with dx, the input gradient (weight transpose + gather).  Each pass has two floors: the bytes it must move at 8 TB/s (forward: x, w, out,
z; backward: z, dout, x, dw; dx: dz, w, dx) and its 3 x 2 M K N flops at 833 TF (three bf16 MFMA passes at a third of 2.5 PF); the table
gives the larger one over the median.
Step 2, the model: mit_b1 in train mode (drop path 0) on [8,3,480,480], forward + backward, `norm_impl` 'hip' on both sides, `conv_impl`
'torch' against 'hip'; peak allocated memory of one pass beyond what was allocated before it; whether two passes give the same bits in the
gradients of the four proj.weight, per variant -- and the same with `sr_impl` 'hip' as well, since a gradient can only repeat its bits
when the gradient that reaches the embedding does.

Method (as scripts/bench_ln_train.py): the parent process never opens the GPU; each step is one child process under its own time limit, and
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

# (k, stride), input (B, Cin, H, W), Cout: the embeddings of mit_b1 on [8,3,480,480]
EMBEDS = (((7, 4), (8, 3, 480, 480), 64), ((3, 2), (8, 64, 120, 120), 128), ((3, 2), (8, 128, 60, 60), 320), ((3, 2), (8, 320, 30, 30), 512))
MODEL_INPUT = (8, 3, 480, 480)
STEP_LIMIT = {'embeds': 300, 'model': 360}             # seconds per child process
HBM, MFMA3 = 8e12, 833e12                              # bytes per second; flops per second of a three-pass bf16 product
PROJ = tuple('patch_embed%d.proj.weight' % i for i in range(1, 5))


def child_embeds(reps):
    import torch
    import vss_cffm_amd as V
    from vss_cffm_amd import _lib, backbone, ops
    dev = torch.device('cuda:0')
    lib = _lib.get()
    res = []
    for (k, s), shape, cout in EMBEDS:
        g = torch.Generator().manual_seed(0)
        b, cin, h, w = shape
        m = backbone.OverlapPatchEmbed(img_size=h, patch_size=k, stride=s, in_chans=cin, embed_dim=cout).to(dev)
        with torch.no_grad():
            m.norm.weight.add_(0.2 * torch.randn(cout, generator=g).to(dev))
        with_dx = k == 3
        x = torch.randn(shape, generator=g).to(dev).requires_grad_(with_dx)
        ho, wo = ops.patch_embed_out_hw(m.proj, h, w)
        dout = torch.randn(b, ho * wo, cout, generator=g).to(dev)
        params = list(m.parameters())

        def both(fn):
            def run():
                x.grad = None
                for p in params:
                    p.grad = None
                fn()[0].backward(dout)
            return run

        def grads():
            return [x.grad.clone() if with_dx else None] + [p.grad.clone() for p in params]

        both(lambda: m(x))()
        want = grads()
        both(lambda: V.overlap_patch_embed(x, m.proj, m.norm))()
        got = grads()
        err = [float((p - q).abs().max() / q.abs().max()) for p, q in zip(got, want) if p is not None]
        # the passes of the library's call by themselves
        P, st = ops._ptr, ops._stream(x)
        xd, wt, bias, gam, bet = x.detach(), m.proj.weight.detach(), m.proj.bias.detach(), m.norm.weight.detach(), m.norm.bias.detach()
        out, z = torch.empty_like(dout), torch.empty_like(dout)
        dx, dw, db, dg, dbt = torch.empty_like(xd), torch.empty_like(wt), torch.empty_like(bias), torch.empty_like(gam), torch.empty_like(bet)
        dims = (b, cin, h, w, cout, k, s)
        nbytes = {d: lib.cffm_patch_embed_bwd_workspace_bytes(*dims, d) for d in ((0, 1) if with_dx else (0,))}
        ws = torch.empty(max(nbytes.values()) // 4, device=dev)

        def fwd():
            _lib.check(lib.cffm_patch_embed_fwd_train(P(xd), P(wt), P(bias), P(gam), P(bet), P(out), P(z), *dims, m.norm.eps, st), lib)

        def bwd(d):
            def run():
                _lib.check(lib.cffm_patch_embed_bwd(P(xd), P(wt), P(gam), P(z), P(dout), P(dx if d else None), P(dw), P(db), P(dg), P(dbt), P(ws),
                                                    *dims, m.norm.eps, st), lib)
            return run

        fns = {'torch_fwd_bwd': both(lambda: m(x)), 'hip_fwd_bwd': both(lambda: V.overlap_patch_embed(x, m.proj, m.norm)), 'pass_fwd': fwd,
               'pass_bwd_no_dx': bwd(0)}
        if with_dx:
            fns['pass_bwd_dx'] = bwd(1)
        torch.cuda.synchronize()
        us = alternate(fns, reps, 8)
        mrows, kk = b * ho * wo, cin * k * k
        f4 = lambda *ts: 4 * sum(t.numel() for t in ts)
        res.append(dict(k=k, stride=s, shape=list(shape), cout=cout, rows=mrows, K=kk, rel_err_vs_torch=err, us=us, ws_bytes=nbytes,
                        flops=3 * 2 * mrows * kk * cout,
                        bytes=dict(pass_fwd=f4(xd, wt, out, z), pass_bwd_no_dx=f4(z, dout, xd, dw), dx=f4(z, wt, dx))))
        del m, x, dout, fns, ws
        torch.cuda.empty_cache()
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), embeds=res)), flush=True)


def child_model(reps):
    import torch
    import vss_cffm_amd as V
    from oracle import recipe as R
    from vss_cffm_amd import backbone
    dev = torch.device('cuda:0')
    m = V.build_backbone(dict(type='mit_b1', style='pytorch'))
    m.load_state_dict(R.synth_state(m, seed=40), strict=True)
    m.reset_drop_path(0.)                              # both variants the same deterministic network
    m.to(dev).train()
    m.set_norm_impl('hip')
    img = R.synth_input('img', MODEL_INPUT, seed=41, scale=1.0).to(dev)
    named = dict(m.named_parameters())

    def with_impl(kind, fn):
        def run():
            m.set_conv_impl(kind)
            return fn()
        return run

    def fwd_bwd():
        for p in m.parameters():
            p.grad = None
        outs = m(img)
        sum(o.square().mean() for o in outs).backward()
        return outs

    def twice(kind):
        outs = [o.detach().clone() for o in with_impl(kind, fwd_bwd)()]
        a = [named[n].grad.clone() for n in PROJ]
        with_impl(kind, fwd_bwd)()
        return outs, [bool(torch.equal(p, named[n].grad)) for p, n in zip(a, PROJ)]

    same, first = {}, {}
    for kind in ('torch', 'hip'):
        first[kind], same[kind] = twice(kind)
    # the embeddings' gradients depend on the gradient that reaches them: the same question with the `sr` convolutions on the library too
    backbone.Attention.sr_impl = 'hip'
    for kind in ('torch', 'hip'):
        outs, same[kind + ', sr_impl hip'] = twice(kind)
    backbone.Attention.sr_impl = 'torch'
    err = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(first['hip'], first['torch'])]
    del first, outs
    fns = {'%s_fwd_bwd' % k: with_impl(k, fwd_bwd) for k in ('torch', 'hip')}
    mem = {k: peak_extra(fn) for k, fn in fns.items()}
    us = alternate(fns, reps, 1)
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), rel_err_hip_vs_torch=err, mem=mem, us=us, same_bits=same)), flush=True)


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
        return {'embeds': child_embeds, 'model': child_model}[a.child](a.reps)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    r = run_child('embeds', a.reps)
    say('The differentiable patch embedding against Conv2d + flatten / transpose + LayerNorm on %s, forward + backward, us per call; one '
        'repetition = every variant once, in turn' % r['device'])
    for e in r['embeds']:
        u = e['us']
        say('(k, stride) = (%d, %d), x %s -> %d rows of %d, K = %d; backward workspace %s MB; dx: %s' % (
            e['k'], e['stride'], tuple(e['shape']), e['rows'], e['cout'], e['K'],
            ' / '.join('%.1f' % (v / 1e6) for v in e['ws_bytes'].values()), 'yes' if e['k'] == 3 else 'no (the image)'))
        say('  max|hip - torch| / max|torch| of %sdw, db, dgamma, dbeta: %s' % ('dx, ' if e['k'] == 3 else '', ', '.join('%.1e' % v for v in e['rel_err_vs_torch'])))
        say('  %-16s %s' % ('hip_fwd_bwd', fmt(u['hip_fwd_bwd'])))
        say('  %-16s %s' % ('torch_fwd_bwd', fmt(u['torch_fwd_bwd'])))
        say('  forward + backward: %s' % verdict(u['torch_fwd_bwd'], u['hip_fwd_bwd']))
        fl = e['flops'] / MFMA3 * 1e6
        for name in ('pass_fwd', 'pass_bwd_no_dx'):
            by = e['bytes'][name] / HBM * 1e6
            say('  %-16s %s   floors: %.2f us of bytes, %.2f us of flops -> larger floor / median = %.3f' % (
                name, fmt(u[name]), by, fl, max(by, fl) / u[name]['median']))
        if 'pass_bwd_dx' in u:
            d, by = u['pass_bwd_dx']['median'] - u['pass_bwd_no_dx']['median'], e['bytes']['dx'] / HBM * 1e6
            say('  %-16s %s' % ('pass_bwd_dx', fmt(u['pass_bwd_dx'])))
            say('  dx = pass_bwd_dx - pass_bwd_no_dx = %.1f us (medians)   floors: %.2f us of bytes, %.2f us of flops -> larger floor / dx = %.3f' % (
                d, by, fl, max(by, fl) / d))
    r = run_child('model', a.reps)
    u, mem = r['us'], r['mem']
    say()
    say('mit_b1 on %s, train mode, forward + backward, norm_impl hip on both sides, conv_impl hip against torch, us per pass' % (list(MODEL_INPUT),))
    say('  largest |hip - torch| / max|torch| of the four outputs: %s' % ', '.join('%.1e' % e for e in r['rel_err_hip_vs_torch']))
    for k in ('torch_fwd_bwd', 'hip_fwd_bwd'):
        say('  %-14s %s   peak memory %8.1f MB' % (k, fmt(u[k]), mem[k] / 1e6))
    say('  forward + backward: %s' % verdict(u['torch_fwd_bwd'], u['hip_fwd_bwd']))
    for k, v in r['same_bits'].items():
        say('  two conv_impl %s passes, the gradients of the four proj.weight bit-equal: %s' % (k, ', '.join('yes' if e else 'NO' for e in v)))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
