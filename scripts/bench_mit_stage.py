"""Times the mit_b1 backbone's eval forward with one library call per stage (MixVisionTransformer.stage_impl = 'hip') against today's path
('torch': the modules' own forward with the three fused ops at their defaults) on one MI355X, and the three LayerNorm kernels behind the
stage call alone.

    python scripts/bench_mit_stage.py [--reps 25] [--out profiles/mit_stage_infer.txt]

Step 1, the kernels: cffm_ln_rows, cffm_nchw_ln_rows and cffm_ln_rows_nchw at the stage-1 and stage-4 shapes of mit_b1 on [8,3,480,480]
((8,64,120,120) and (8,512,15,15)), each against its byte count (every element read once and written once: 8 bytes) at 8 TB/s, next to
the stock PyTorch ops they replace.
Step 2 and 3, the model: mit_b1 in eval mode under no_grad on [8,3,480,480] (the shape of the other tables) and on [4,3,480,864] (one
VSPW evaluation clip), `stage_impl` 'torch' against 'hip' with `dwconv_impl`, `attn_impl` and `sr_impl` at their defaults, eager and
replayed from one torch.cuda.graph capture of the whole forward; peak allocated memory of one eager call beyond what was allocated
before it; the largest |hip - torch| / max|torch| of the four outputs.

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

LN_SHAPES = ((8, 64, 120, 120), (8, 512, 15, 15))     # (B, C, H, W): stage 1 and stage 4 of mit_b1 on [8,3,480,480]
MODEL_INPUTS = {'b1_480': (8, 3, 480, 480), 'b1_clip': (4, 3, 480, 864)}
STEP_LIMIT = {'kernels': 240, 'b1_480': 360, 'b1_clip': 360}      # seconds per child process
HBM = 8e12                                             # bytes per second


def child_kernels(reps):
    import torch
    import torch.nn.functional as F
    import vss_cffm_amd as V
    dev = torch.device('cuda:0')
    res = []
    for b, c, h, w in LN_SHAPES:
        g = torch.Generator().manual_seed(0)
        x = torch.randn(b, c, h, w, generator=g).to(dev)
        rows = x.flatten(2).transpose(1, 2).contiguous()
        gam, bet = (1 + 0.2 * torch.randn(c, generator=g)).to(dev), (0.1 * torch.randn(c, generator=g)).to(dev)
        o_rows, o_map = torch.empty_like(rows), torch.empty_like(x)
        with torch.no_grad():
            fns = {
                'ln_rows': lambda: V.ln_rows(rows, gam, bet, 1e-6, out=o_rows),
                'torch_ln_rows': lambda: F.layer_norm(rows, (c,), gam, bet, 1e-6),
                'nchw_ln_rows': lambda: V.nchw_ln_rows(x, gam, bet, 1e-6, out=o_rows),
                'torch_nchw_ln_rows': lambda: F.layer_norm(x.flatten(2).transpose(1, 2), (c,), gam, bet, 1e-6),
                'ln_rows_nchw': lambda: V.ln_rows_nchw(rows, gam, bet, h, w, 1e-6, out=o_map),
                'torch_ln_rows_nchw': lambda: F.layer_norm(rows, (c,), gam, bet, 1e-6).reshape(b, h, w, c).permute(0, 3, 1, 2).contiguous(),
            }
            err = {k: float((fns[k]() - fns['torch_' + k]()).abs().max()) for k in ('ln_rows', 'nchw_ln_rows', 'ln_rows_nchw')}
            us = alternate(fns, reps, 8)
        res.append(dict(shape=[b, c, h, w], abs_err_vs_torch=err, us=us, bytes=8 * x.numel()))
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), shapes=res)), flush=True)


def child_model(which, reps):
    import torch
    import vss_cffm_amd as V
    from oracle import recipe as R
    from vss_cffm_amd import backbone as B
    dev = torch.device('cuda:0')
    m = V.build_backbone(dict(type='mit_b1', style='pytorch'))
    m.load_state_dict(R.synth_state(m, seed=40), strict=True)
    m.to(dev).eval()
    img = R.synth_input('img', MODEL_INPUTS[which], seed=41, scale=1.0).to(dev)

    def eager(kind):
        def run():
            B.MixVisionTransformer.stage_impl = kind
            with torch.no_grad():
                return m(img)
        return run

    outs = {k: [o.clone() for o in eager(k)()] for k in ('torch', 'hip')}
    err = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(outs['hip'], outs['torch'])]
    del outs
    fns = {'torch_eager': eager('torch'), 'hip_eager': eager('hip')}
    mem = {k: peak_extra(fn) for k, fn in fns.items()}
    graphs, kept = {}, {}
    for kind in ('torch', 'hip'):
        for _ in range(2):
            eager(kind)()
        torch.cuda.synchronize()
        graphs[kind] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[kind]):
            kept[kind] = eager(kind)()
        fns[kind + '_graph'] = graphs[kind].replay
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    gerr = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(kept['hip'], kept['torch'])]
    us = alternate(fns, reps, 1)
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), rel_err_hip_vs_torch=err, rel_err_graph=gerr, mem=mem, us=us)), flush=True)


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
        return child_kernels(a.reps) if a.child == 'kernels' else child_model(a.child, a.reps)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    r = run_child('kernels', a.reps)
    say('LayerNorm kernels of the stage call on %s, us per call; one repetition = every variant once, in turn' % r['device'])
    for s in r['shapes']:
        u, bound = s['us'], s['bytes'] / HBM * 1e6
        say('map (B,C,H,W) = %s: %.1f MB read + written, %.2f us at 8 TB/s' % (tuple(s['shape']), s['bytes'] / 1e6, bound))
        for k in ('ln_rows', 'nchw_ln_rows', 'ln_rows_nchw'):
            say('  %-20s %s   byte bound / median = %.2f   max|hip - torch| %.1e' % (k, fmt(u[k]), bound / u[k]['median'], s['abs_err_vs_torch'][k]))
            say('  %-20s %s' % ('torch_' + k, fmt(u['torch_' + k])))
    for which in ('b1_480', 'b1_clip'):
        r = run_child(which, a.reps)
        u, mem = r['us'], r['mem']
        say()
        say('mit_b1 on %s, eval, no_grad, stage_impl hip against torch (dwconv_impl, attn_impl, sr_impl at their defaults), us per forward' % (list(MODEL_INPUTS[which]),))
        say('  largest |hip - torch| / max|torch| of the four outputs: eager %s; graph %s' % (
            ', '.join('%.1e' % e for e in r['rel_err_hip_vs_torch']), ', '.join('%.1e' % e for e in r['rel_err_graph'])))
        for k in ('torch_eager', 'hip_eager', 'torch_graph', 'hip_graph'):
            say('  %-12s %s%s' % (k, fmt(u[k]), '   peak memory %8.1f MB' % (mem[k] / 1e6) if k in mem else ''))
        say('  eager: %s' % verdict(u['torch_eager'], u['hip_eager']))
        say('  one graph replay: %s' % verdict(u['torch_graph'], u['hip_graph']))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
