"""Times the patch-embedding kernel (vss_cffm_amd.patch_embed) and the mit_b1 evaluation forward with the embeddings inside the library
call (MixVisionTransformer.embed_impl = 'hip') on one MI355X against stock PyTorch on the same device.

    python scripts/bench_patch_embed.py [--reps 25] [--out profiles/patch_embed.txt]

Step 1, the kernel: each of mit_b1's four embeddings at [8,3,480,480] -- (7,4) on [8,3,480,480] -> 64, (3,2) on [8,64,120,120] -> 128,
(3,2) on [8,128,60,60] -> 320, (3,2) on [8,320,30,30] -> 512 -- against the torch sequence Conv2d, flatten(2).transpose(1, 2), LayerNorm
under no_grad.  Two floors per shape: the bytes that have to move (input + weight + output rows, fp32) at 8 TB/s, and 3 x 2 M K N flops at
the 833 TF a three-pass bf16 product can reach (2.5 PF / 3).
Step 2, the model: mit_b1 in eval mode under no_grad with stage_impl = 'hip', embed_impl 'torch' against 'hip', eager and as one replay
of a captured graph, at [8,3,480,480] and [4,3,480,864]; the workspace bytes the module keeps and the peak allocated memory of one eager
call beyond what was allocated before it.

Method (as scripts/bench_mit.py): the parent process never opens the GPU; each step is one child process under its own time limit, and
the second starts only if the first ended well.  Everything is warmed up first; one repetition times every variant once, in turn (the
variants ALTERNATE), between two device events; the figure of a variant is the median over the repetitions, its spread the distance
between the 10th and the 90th percentile.  'hip' counts as faster when median(torch) - median(hip) exceeds the sum of the two spreads."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_mit import alternate, fmt, peak_extra, verdict  # noqa: E402

# (k, stride), input, Cout
EMBEDS = (((7, 4), (8, 3, 480, 480), 64), ((3, 2), (8, 64, 120, 120), 128), ((3, 2), (8, 128, 60, 60), 320), ((3, 2), (8, 320, 30, 30), 512))
MODEL_INPUTS = ((8, 3, 480, 480), (4, 3, 480, 864))
STEP_LIMIT = {'kernel': 300, 'model': 420}          # seconds per child process
HBM = 8e12                                           # bytes per second
PEAK3 = 2.5e15 / 3                                   # flops per second of a three-pass bf16 product


def child_kernel(reps):
    import torch
    import vss_cffm_amd as V
    from oracle import recipe as R
    from vss_cffm_amd import backbone as B
    dev = torch.device('cuda:0')
    res = []
    for (k, s), shape, cout in EMBEDS:
        pe = B.OverlapPatchEmbed(img_size=480, patch_size=k, stride=s, in_chans=shape[1], embed_dim=cout)
        pe.load_state_dict(R.synth_state(pe, seed=60), strict=True)
        pe.to(dev).eval()
        x = R.synth_input('pembed_x', shape, seed=61, scale=1.0).to(dev)

        def seq():
            with torch.no_grad():
                return pe(x)[0]

        def hip():
            with torch.no_grad():
                return V.patch_embed(x, pe.proj, pe.norm)[0]

        want, got = seq(), hip()
        again = hip()
        torch.cuda.synchronize()
        err = float((got - want).abs().max() / want.abs().max())
        same = bool(torch.equal(got, again))
        m, n, kk = got.shape[0] * got.shape[1], cout, shape[1] * k * k
        del want, got, again
        us = alternate({'torch': seq, 'hip': hip}, reps, 4)
        res.append(dict(k=k, stride=s, shape=list(shape), cout=cout, M=m, K=kk, rel_err_vs_torch=err, same_bits=same, us=us,
                        bytes=4 * (x.numel() + n * kk + m * n), flops=6 * m * kk * n))
        del x, pe
        torch.cuda.empty_cache()
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), shapes=res)), flush=True)


def child_model(reps):
    import torch
    import vss_cffm_amd as V
    from oracle import recipe as R
    from vss_cffm_amd import backbone as B
    dev = torch.device('cuda:0')
    B.MixVisionTransformer.stage_impl = 'hip'
    res = []
    for shape in MODEL_INPUTS:
        m = V.build_backbone(dict(type='mit_b1', style='pytorch'))
        m.load_state_dict(R.synth_state(m, seed=40), strict=True)
        m.to(dev).eval()
        img = R.synth_input('img', shape, seed=41, scale=1.0).to(dev)

        def eager(kind):
            def run():
                B.MixVisionTransformer.embed_impl = kind
                with torch.no_grad():
                    return m(img)
            return run

        outs = {k: [o.clone() for o in eager(k)()] for k in ('torch', 'hip')}
        err = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(outs['hip'], outs['torch'])]
        same = all(bool(torch.equal(a, b)) for a, b in zip(outs['hip'], eager('hip')()))
        del outs
        kept = {'torch': 4 * sum(w.numel() for w in m._stage_workspaces.values()), 'hip': 4 * sum(w.numel() for w in m._run_workspaces.values())}
        mem = {k: peak_extra(eager(k)) for k in ('torch', 'hip')}
        graphs = {}
        for k in ('torch', 'hip'):
            eager(k)()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                keep = eager(k)()
            graphs[k] = (g, keep)
        fns = {'torch_eager': eager('torch'), 'hip_eager': eager('hip'), 'torch_graph': graphs['torch'][0].replay, 'hip_graph': graphs['hip'][0].replay}
        us = alternate(fns, reps, 1)
        res.append(dict(shape=list(shape), rel_err_hip_vs_torch=err, same_bits=same, kept=kept, mem=mem, us=us))
        del graphs, fns, m, img
        torch.cuda.empty_cache()
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), inputs=res)), flush=True)


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
    say('Overlapping patch embedding (Conv2d + flatten / transpose + LayerNorm -> token rows) on %s, us per call under no_grad; one repetition = '
        'every variant once, in turn' % r['device'])
    for s in r['shapes']:
        u = s['us']
        say('k %d stride %d, input %s -> %d channels (GEMM M %d, K %d, N %d); largest |hip - torch| / max|torch| %.1e; two hip calls the same '
            'bits: %s' % (s['k'], s['stride'], s['shape'], s['cout'], s['M'], s['K'], s['cout'], s['rel_err_vs_torch'], 'yes' if s['same_bits'] else 'NO'))
        for k in ('torch', 'hip'):
            say('  %-6s %s' % (k, fmt(u[k])))
        fb, ff = s['bytes'] / HBM * 1e6, s['flops'] / PEAK3 * 1e6
        say('  %s' % verdict(u['torch'], u['hip']))
        say('  floors: bytes %.1f us (%.1f MB at 8 TB/s), three-pass flops %.1f us (%.2f GFLOP x 3 at 833 TF) -> hip runs at %.3f of the '
            'larger one' % (fb, s['bytes'] / 1e6, ff, s['flops'] / 3e9, max(fb, ff) / u['hip']['median']))
    r = run_child('model', a.reps)
    for s in r['inputs']:
        u = s['us']
        say()
        say('mit_b1 on %s (eval, no_grad, stage_impl hip), embed_impl hip against torch, us per forward; largest |hip - torch| / max|torch| of '
            'the four outputs: %s; two hip forwards the same bits: %s' % (s['shape'], ', '.join('%.1e' % e for e in s['rel_err_hip_vs_torch']),
                                                                          'yes' if s['same_bits'] else 'NO'))
        for k in ('torch_eager', 'hip_eager', 'torch_graph', 'hip_graph'):
            say('  %-12s %s' % (k, fmt(u[k])))
        say('  eager: %s' % verdict(u['torch_eager'], u['hip_eager']))
        say('  one graph replay: %s' % verdict(u['torch_graph'], u['hip_graph']))
        say('  workspace kept on the module: torch %.1f MB (four stages), hip %.1f MB (one run); peak memory of one eager forward: torch '
            '%.1f MB, hip %.1f MB' % (s['kept']['torch'] / 1e6, s['kept']['hip'] / 1e6, s['mem']['torch'] / 1e6, s['mem']['hip'] / 1e6))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
