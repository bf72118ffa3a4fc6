"""Times evaluation's tail -- resize to the input size, resize to ori_shape, softmax, arg-max -- on one MI355X at VSPW's evaluation shape:
logits [1,124,120,216] as the head leaves them (token rows viewed as [B,K,h,w]) -> 480 x 864 -> 480 x 853.

    python scripts/bench_predict.py [--reps 25] [--out profiles/predict.txt]

Variants, all from the same logits:
  torch  the reference's op sequence in stock PyTorch on the device (F.interpolate twice, softmax, argmax), as predict_impl = 'torch' runs it;
  hip    vss_cffm_amd.predict (one library call), eager;
  graph  the same call replayed from a HIP graph;
  probs  the PROBS form (probabilities written, no label map) against the torch sequence without its argmax -- what inference() returns.

Before anything is timed the arg-max rule of tests/test_predict.py is checked at this shape against the op sequence in fp32 on the CPU.
Peak memory is torch.cuda.max_memory_allocated over one call minus what was allocated before it.

Method (as scripts/bench_kmeans.py): the parent process never opens the GPU; the measurement is one child process under its own time
limit.  Everything is warmed up first; one repetition times every variant once, in turn (the variants ALTERNATE), between two device
events around `inner` back-to-back calls; the figure of a variant is the median over the repetitions, its spread the distance between the
10th and the 90th percentile.  hip counts as faster than torch when median(torch) - median(hip) exceeds the sum of the two spreads."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (1, 124, (120, 216), (480, 864), (480, 853))
STEP_LIMIT = 420          # seconds for the child process
GAP, EXEMPT_CAP = 1e-4, 0.005


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
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def child(reps):
    import torch
    import torch.nn.functional as F
    import vss_cffm_amd as V
    dev = torch.device('cuda:0')
    m, k, (h, w), mid, out = SHAPE
    g = torch.Generator().manual_seed(0)
    x = 3.0 * torch.randn(m, k, h, w, generator=g)
    x = 3.0 * F.avg_pool2d(F.pad(x, (1, 1, 1, 1), mode='replicate'), 3, stride=1)        # neighbouring cells agree, as real logits do
    lg = x.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                  # token rows, as the heads leave them

    def seq(t, argmax=True):
        y = F.interpolate(t, size=mid, mode='bilinear', align_corners=False)
        y = F.interpolate(y, size=out, mode='bilinear', align_corners=False)
        p = F.softmax(y, dim=1)
        return p.argmax(dim=1) if argmax else p

    # ---- the arg-max rule at this shape, against the fp32 op sequence on the CPU
    y = F.interpolate(F.interpolate(x, size=mid, mode='bilinear', align_corners=False), size=out, mode='bilinear', align_corners=False)
    want = F.softmax(y, dim=1).argmax(dim=1)
    top = y.topk(2, dim=1).values
    exempt = (top[:, 0] - top[:, 1]) < GAP * float(x.abs().max())
    del y, top
    pred = V.predict(lg, mid, out)
    torch.cuda.synchronize()
    same = pred.cpu() == want
    rule = dict(exempt_share=float(exempt.float().mean()), differ=int((~same).sum()), differ_not_exempt=int((~same & ~exempt).sum()),
                torch_gpu_differs=int((seq(lg).cpu() != want).sum()), pixels=want.numel())
    if rule['exempt_share'] > EXEMPT_CAP or rule['differ_not_exempt']:
        print('RESULT ' + json.dumps(dict(rule=rule, failed=True)), flush=True)
        return

    probs = torch.empty((m, k) + tuple(out), device=dev)
    fns = {'torch': lambda: seq(lg), 'hip': lambda: V.predict(lg, mid, out), 'torch_probs': lambda: seq(lg, False),
           'probs': lambda: V.predict(lg, mid, out, probs=probs, want_pred=False)}
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    prob_err = float((probs - seq(lg, False)).abs().max())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gpred = V.predict(lg, mid, out)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    fns['graph'] = graph.replay
    mem = dict(torch=peak_extra(fns['torch']), hip=peak_extra(fns['hip']), label_map=pred.numel() * 8, logits=lg.numel() * 4)
    t = {key: [] for key in fns}
    inner = {'torch': 2, 'torch_probs': 2, 'hip': 8, 'probs': 4, 'graph': 8}
    for _ in range(reps):
        for key, fn in fns.items():
            t[key].append(timed(fn, inner[key]))
    print('RESULT ' + json.dumps(dict(rule=rule, device=torch.cuda.get_device_name(0), graph_equals_eager=bool(torch.equal(gpred, pred)),
                                      probs_max_err_vs_torch_gpu=prob_err, mem=mem, us={key: summary(v) for key, v in t.items()})), flush=True)


def fmt(s):
    return 'median %9.1f  p10 %9.1f  p90 %9.1f  min %9.1f  max %9.1f  (%d reps)' % (s['median'], s['p10'], s['p90'], s['min'], s['max'], s['reps'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--child', action='store_true', help='run the measurement in this process')
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit('at least 20 repetitions')
    if a.child:
        return child(a.reps)
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--reps', str(a.reps)], capture_output=True, text=True,
                           timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        raise SystemExit('the measurement ran past its %d s limit' % STEP_LIMIT)
    got = [l for l in p.stdout.splitlines() if l.startswith('RESULT ')]
    if p.returncode != 0 or not got:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit('the measurement failed (exit code %d)' % p.returncode)
    r = json.loads(got[-1][7:])
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    m, k, (h, w), mid, out = SHAPE
    rule = r['rule']
    say('prediction tail at VSPW\'s evaluation shape: logits [%d,%d,%d,%d] (token rows) -> %d x %d -> %d x %d, us per call' %
        (m, k, h, w, mid[0], mid[1], out[0], out[1]))
    say('arg-max rule against the fp32 op sequence on the CPU: %.3f %% of the %d pixels exempt (cap %.1f %%), %d differ, %d of them not exempt; '
        'the torch sequence on the GPU differs from the CPU one at %d pixels' %
        (100 * rule['exempt_share'], rule['pixels'], 100 * EXEMPT_CAP, rule['differ'], rule['differ_not_exempt'], rule['torch_gpu_differs']))
    if r.get('failed'):
        say('the arg-max rule does NOT hold at this shape: nothing was timed')
        raise SystemExit(1)
    u, mem = r['us'], r['mem']
    say('on %s; one repetition = every variant once, in turn; graph replay equals the eager call bit for bit: %s' % (r['device'], r['graph_equals_eager']))
    say('  torch        op sequence, arg-max          ' + fmt(u['torch']))
    say('  hip          vss_cffm_amd.predict, eager   ' + fmt(u['hip']))
    say('  graph        the same, graph replay        ' + fmt(u['graph']))
    say('  torch_probs  op sequence, probabilities    ' + fmt(u['torch_probs']))
    say('  probs        predict(probs=..), eager      ' + fmt(u['probs']))
    spread = (u['torch']['p90'] - u['torch']['p10']) + (u['hip']['p90'] - u['hip']['p10'])
    gain = u['torch']['median'] - u['hip']['median']
    say('  torch - hip = %.1f us (torch / hip = %.1f, torch / graph = %.1f, torch_probs / probs = %.1f); sum of the two p10-p90 spreads %.1f us '
        '-> hip faster than torch beyond the spreads: %s' % (gain, u['torch']['median'] / u['hip']['median'], u['torch']['median'] / u['graph']['median'],
                                                               u['torch_probs']['median'] / u['probs']['median'], spread, 'yes' if gain > spread else 'NO'))
    say('  probabilities of the PROBS form against the torch sequence on the GPU: max |difference| %.2e' % r['probs_max_err_vs_torch_gpu'])
    say('  peak memory over one call, beyond what was allocated before it: torch %.1f MB, hip %.1f MB (the label map alone is %.1f MB; the logits are %.1f MB) '
        '-> hip allocates the label map and nothing else: %s' % (mem['torch'] / 1e6, mem['hip'] / 1e6, mem['label_map'] / 1e6, mem['logits'] / 1e6,
                                                                  'yes' if mem['hip'] <= mem['label_map'] + 512 else 'NO'))
    moved = mem['logits'] + mem['label_map']
    say('  bytes that have to move: %.1f MB in + %.1f MB out; at the graph-replayed %.1f us that is %.0f GB/s' %
        (mem['logits'] / 1e6, mem['label_map'] / 1e6, u['graph']['median'], moved / u['graph']['median'] / 1e3))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
