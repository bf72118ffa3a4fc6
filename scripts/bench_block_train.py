"""Times a mit_b1 training pass with MixVisionTransformer.block_impl 'hip' (all blocks of a stage as one library call per direction,
``ops.mit_blocks_train``) against 'torch' (the loop over the blocks, one library call per op), on one MI355X.

    python scripts/bench_block_train.py [--reps 25] [--out profiles/block_train.txt]

Step 1, the model: mit_b1 in train mode on [8,3,480,480], forward + backward, `block_impl` 'torch' against 'hip' with `norm_impl`,
`conv_impl`, `linear_impl` and `sr_impl` 'hip' on both sides (`attn_impl`, `dwconv_impl` at their default, 'hip'); at drop path 0.1 (what
every reference config trains with) and at 0; peak allocated memory of one pass beyond what was allocated before it; whether the four
outputs of the two settings are equal bit for bit at drop path 0.
Step 2, the stages: forward + backward of each stage's blocks alone on the token rows that stage sees ([8, H*W, C] with H = W = 120, 60,
30, 15), both ways: the loop over the Block modules against one ``mit_blocks_train`` call, drop path 0.1, x and every parameter
requiring grad.

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

MODEL_INPUT = (8, 3, 480, 480)
STEP_LIMIT = {'model': 360, 'stages': 360}            # seconds per child process
DROP = 0.1


def _model():
    import torch
    import vss_cffm_amd as V
    from oracle import recipe as R
    dev = torch.device('cuda:0')
    m = V.build_backbone(dict(type='mit_b1', style='pytorch'))
    m.load_state_dict(R.synth_state(m, seed=40), strict=True)
    m.to(dev).train()
    m.set_norm_impl('hip')
    m.set_conv_impl('hip')
    m.set_linear_impl('hip')
    for mod in m.modules():
        if hasattr(type(mod), 'sr_impl'):
            mod.sr_impl = 'hip'
    return m, R.synth_input('img', MODEL_INPUT, seed=41, scale=1.0).to(dev)


def child_model(reps):
    import torch
    m, img = _model()

    def with_impl(kind, rate, fn):
        def run():
            m.set_block_impl(kind)
            m.reset_drop_path(rate)
            return fn()
        return run

    def fwd():
        # (grad mode on: under no_grad block_impl has no say)
        return [o.detach() for o in m(img)]

    def fwd_bwd():
        for p in m.parameters():
            p.grad = None
        sum(o.square().mean() for o in m(img)).backward()

    outs = {k: [o.clone() for o in with_impl(k, 0., fwd)()] for k in ('torch', 'hip')}
    equal = [bool(torch.equal(a, b)) for a, b in zip(outs['hip'], outs['torch'])]
    del outs
    fns = {'%s_fwd_bwd drop path %g' % (k, rate): with_impl(k, rate, fwd_bwd) for rate in (DROP, 0.) for k in ('torch', 'hip')}
    mem = {k: peak_extra(fn) for k, fn in fns.items()}
    us = alternate(fns, reps, 1)
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), outputs_equal=equal, mem=mem, us=us)), flush=True)


def child_stages(reps):
    import torch
    import vss_cffm_amd as V
    from vss_cffm_amd import backbone as B
    m, _ = _model()
    m.reset_drop_path(DROP)
    dev = torch.device('cuda:0')
    res = {}
    for i in range(1, 5):
        blocks = getattr(m, 'block%d' % i)
        c, hw = blocks[0].attn.dim, MODEL_INPUT[2] // 2 ** (i + 1)
        g = torch.Generator().manual_seed(i)
        x = torch.randn(MODEL_INPUT[0], hw * hw, c, generator=g).to(dev).requires_grad_(True)
        dy = torch.randn(MODEL_INPUT[0], hw * hw, c, generator=g).to(dev)
        params = list(blocks.parameters())

        def loop():
            y = x
            for blk in blocks:
                y = blk(y, hw, hw)
            return y

        def call():
            return V.mit_blocks_train(x, blocks, hw, hw, [(B._drop_scale(b.drop_path, x), B._drop_scale(b.drop_path, x)) for b in blocks])

        def both(fn):
            def run():
                for t in [x] + params:
                    t.grad = None
                fn().backward(dy)
            return run

        fns = {'torch': both(loop), 'hip': both(call)}
        mem = {k: peak_extra(fn) for k, fn in fns.items()}
        res['stage %d' % i] = dict(shape=[MODEL_INPUT[0], hw * hw, c], depth=len(blocks), us=alternate(fns, reps, 2), mem=mem)
        del x, dy, fns
        torch.cuda.empty_cache()
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), stages=res)), flush=True)


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
        return {'model': child_model, 'stages': child_stages}[a.child](a.reps)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    r = run_child('model', a.reps)
    u, mem = r['us'], r['mem']
    say('mit_b1 on %s on %s, train mode, forward + backward, block_impl hip against torch (norm_impl, conv_impl, linear_impl, sr_impl hip on both '
        'sides; attn_impl, dwconv_impl at their default), us per pass; one repetition = every variant once, in turn'
        % (list(MODEL_INPUT), r['device']))
    say('  the four outputs of hip equal those of torch bit for bit (drop path 0): %s' % ', '.join('yes' if e else 'NO' for e in r['outputs_equal']))
    for rate in (DROP, 0.):
        t, h = 'torch_fwd_bwd drop path %g' % rate, 'hip_fwd_bwd drop path %g' % rate
        for k in (t, h):
            say('  %-28s %s   peak memory %8.1f MB' % (k, fmt(u[k]), mem[k] / 1e6))
        say('  drop path %g: %s' % (rate, verdict(u[t], u[h])))
    r = run_child('stages', a.reps)
    say()
    say('the blocks of each stage alone, forward + backward on the token rows the stage sees, drop path %g, us per pass: the loop over the Block '
        'modules (torch) against one mit_blocks_train call (hip)' % DROP)
    for name, s in r['stages'].items():
        say('%s: rows %s, %d blocks' % (name, s['shape'], s['depth']))
        for k in ('torch', 'hip'):
            say('    %-6s %s   peak memory %8.1f MB' % (k, fmt(s['us'][k]), s['mem'][k] / 1e6))
        say('    %s' % verdict(s['us']['torch'], s['us']['hip']))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
