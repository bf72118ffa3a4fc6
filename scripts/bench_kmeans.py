"""Times the prototype-generating stage of CFFM++ (k-means on the clip stack rows) on one MI355X.

    python scripts/bench_kmeans.py [--reps 25] [--out profiles/kmeans.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_kmeans.py --step trace      (per-kernel times; its own process)

Variants, at (N, K) = (14400, 100), (25920, 100), (14400, 8), 10 iterations, the same seeded initial centres:
  a      head._kmeans as the head called it before the library had a k-means: a Python loop over the clusters with a host
         synchronisation (`if sel.any()`) and a boolean-mask gather each;
  b      a synchronisation-free torch formulation: cdist / argmin / index_add_ (sums and counts) / where, no Python loop over clusters,
         no host round trip (torch.bincount is not used for the counts: on the GPU it reads the maximum back to size its output, a
         synchronisation per iteration) -- the honest baseline;
  c      vss_cffm_amd.kmeans (one library call), eager;
  graph  the same call replayed from a HIP graph;
and the prototype-generating head's whole eval forward at B1 480 x 480 (n_clusters = 100) on the old path (rows_impl = 'torch': the
reference's op sequence + head._kmeans) and the new one.

Method: the parent process never opens the GPU; every step (one shape, or the head) is a child process of its own under its own time
limit, and the first step that fails or runs out of time ends the run.  Inside a step everything is warmed up first; one repetition
times every variant once, in turn (the variants ALTERNATE), between two device events around `inner` back-to-back calls; the figure of a
variant is the median over the repetitions, its spread the distance between the 10th and the 90th percentile.  c counts as faster than b
when median(b) - median(c) exceeds the larger of the two spreads."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(14400, 100), (25920, 100), (14400, 8)]
ITERS = 10
STEP_LIMIT = {'kmeans': 240, 'head': 240, 'trace': 120}      # seconds per child process


def make_points(n, seed, dev):
    """relu(mode + 0.5 noise) around 30 random modes: post-ReLU features with structure (tests/test_kmeans.py 'relu')"""
    import torch
    g = torch.Generator().manual_seed(seed)
    modes = torch.randn(30, 256, generator=g)
    pick = torch.randint(0, 30, (n,), generator=g)
    return torch.relu(modes[pick] + 0.5 * torch.randn(n, 256, generator=g)).contiguous().to(dev)


def torch_nosync(x, init, iters):
    import torch
    c = init.clone()
    ones = torch.ones(x.shape[0], dtype=torch.float32, device=x.device)
    for _ in range(iters):
        lab = torch.cdist(x, c).argmin(dim=1)
        cnt = torch.zeros(c.shape[0], dtype=torch.float32, device=x.device).index_add_(0, lab, ones)
        s = torch.zeros_like(c).index_add_(0, lab, x)
        c = torch.where(cnt[:, None] > 0, s / cnt.clamp(min=1.0)[:, None], c)
    return c


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


def inertia(x, c):
    import torch
    return float(torch.cdist(x.double(), c.double()).min(dim=1).values.square().sum())


def step_kmeans(n, k, reps):
    import torch
    import vss_cffm_amd as V
    from vss_cffm_amd.head import _kmeans
    dev = torch.device('cuda:0')
    x = make_points(n, 1, dev)
    g = torch.Generator().manual_seed(2)
    init = x[torch.randperm(n, generator=g)[:k].to(dev)].clone()
    ws = V.kmeans_workspace(n, k, dev)

    def a():
        torch.manual_seed(2)
        return _kmeans(x, k, ITERS)

    def b():
        return torch_nosync(x, init, ITERS)

    def c():
        return V.kmeans(x, k, iters=ITERS, init=init, ws=ws)

    for _ in range(3):
        ca, cb, cc = a(), b(), c()[0]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = V.kmeans(x, k, iters=ITERS, init=init, ws=ws)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    same_graph = bool(torch.equal(out[0], cc))
    res = dict(N=n, K=k, device=torch.cuda.get_device_name(0), graph_equals_eager=same_graph,
               inertia=dict(init=inertia(x, init), b=inertia(x, cb), c=inertia(x, cc), a_own_init=inertia(x, ca)),
               ws_mb=ws.numel() / 1e6, x_mb=x.numel() * 4 / 1e6)
    t = {'a': [], 'b': [], 'c': [], 'graph': []}
    for _ in range(reps):
        t['a'].append(timed(a, 1))
        t['b'].append(timed(b, 4))
        t['c'].append(timed(c, 4))
        t['graph'].append(timed(graph.replay, 4))
    res['us'] = {key: summary(v) for key, v in t.items()}
    return res


def head_cfg():
    """the B1 head as configs/cffm_b1_480.py builds it (depths 2), prototype-generating kind"""
    return dict(type='CFFMHead_clips_resize1_8_gene_prototype', in_channels=[64, 128, 320, 512], in_index=[0, 1, 2, 3],
                feature_strides=[4, 8, 16, 32], channels=128, dropout_ratio=0.1, num_classes=124,
                norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False, decoder_params=dict(embed_dim=256, depths=2),
                loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0), num_clips=4)


def step_head(reps):
    import torch
    from vss_cffm_amd.registry import build_head
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    head = build_head(head_cfg()).to(dev).eval()
    g = torch.Generator().manual_seed(3)
    feats = [torch.randn(4, ch, 480 // s, 480 // s, generator=g).to(dev) for ch, s in zip((64, 128, 320, 512), (4, 8, 16, 32))]
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        metas = [{'filename': tmp + '/data/vid0/origin/0001.jpg'}]
        head.save_path = tmp + '/out/'

        def run(impl):
            head.rows_impl = impl
            torch.manual_seed(4)
            return head(feats, 1, 4, None, metas)

        for _ in range(2):
            y_old, y_new = run('torch'), run('hip')
        torch.cuda.synchronize()
        err = float((y_old - y_new).abs().max() / y_old.abs().max())
        t = {'old': [], 'new': []}
        for _ in range(reps):
            t['old'].append(timed(lambda: run('torch'), 1))
            t['new'].append(timed(lambda: run('hip'), 1))
    return dict(device=torch.cuda.get_device_name(0), logits_rel_err=err, us={key: summary(v) for key, v in t.items()})


def step_trace():
    import torch
    import vss_cffm_amd as V
    dev = torch.device('cuda:0')
    for n, k in SHAPES:
        x = make_points(n, 1, dev)
        g = torch.Generator().manual_seed(2)
        init = x[torch.randperm(n, generator=g)[:k].to(dev)].clone()
        ws = V.kmeans_workspace(n, k, dev)
        for _ in range(5):
            V.kmeans(x, k, iters=ITERS, init=init, ws=ws)
        torch.cuda.synchronize()
    return dict(traced='5 calls of 10 iterations per shape')


def child(spec, reps):
    kind = spec.split(':')[0]
    if kind == 'kmeans':
        _, n, k = spec.split(':')
        res = step_kmeans(int(n), int(k), reps)
    elif kind == 'head':
        res = step_head(reps)
    else:
        res = step_trace()
    print('RESULT ' + json.dumps(res), flush=True)


def fmt(s):
    return 'median %9.1f  p10 %9.1f  p90 %9.1f  min %9.1f  max %9.1f  (%d reps)' % (s['median'], s['p10'], s['p90'], s['min'], s['max'], s['reps'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--step', default=None, help='run ONE step in this process: kmeans:N:K | head | trace')
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if a.reps < 20 and a.step != 'trace':
        raise SystemExit('at least 20 repetitions')
    if a.step:
        return child(a.step, a.reps)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def run_step(spec):
        limit = STEP_LIMIT[spec.split(':')[0]]
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', spec, '--reps', str(a.reps)], capture_output=True, text=True,
                               timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit('step %s ran past its %d s limit: stopping here' % (spec, limit))
        got = [l for l in p.stdout.splitlines() if l.startswith('RESULT ')]
        if p.returncode != 0 or not got:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit('step %s failed (exit code %d): stopping here' % (spec, p.returncode))
        return json.loads(got[-1][7:])

    say('k-means of the prototype-generating stage, %d iterations, us per call; one repetition = every variant once, in turn' % ITERS)
    verdicts = []
    for n, k in SHAPES:
        r = run_step('kmeans:%d:%d' % (n, k))
        u = r['us']
        say()
        say('N=%d K=%d on %s  (x %.1f MB, workspace %.1f MB; graph replay equals the eager call bit for bit: %s)' %
            (n, k, r['device'], r['x_mb'], r['ws_mb'], r['graph_equals_eager']))
        say('  fp64 inertia: initial centres %.6e, after b %.6e, after c %.6e (same start; trajectories are not comparable bit for bit), '
            'after a (its own randperm start) %.6e' % (r['inertia']['init'], r['inertia']['b'], r['inertia']['c'], r['inertia']['a_own_init']))
        say('  a      head._kmeans (Python loop)   ' + fmt(u['a']))
        say('  b      torch, synchronisation-free  ' + fmt(u['b']))
        say('  c      vss_cffm_amd.kmeans, eager   ' + fmt(u['c']))
        say('  graph  the same, graph replay       ' + fmt(u['graph']))
        spread = max(u['b']['p90'] - u['b']['p10'], u['c']['p90'] - u['c']['p10'])
        gain = u['b']['median'] - u['c']['median']
        ok = gain > spread
        verdicts.append(ok)
        say('  b - c = %.1f us (b / c = %.2f, b / graph = %.2f, a / c = %.1f); larger p10-p90 spread of the two %.1f us -> c faster than b '
            'beyond the spread: %s' % (gain, u['b']['median'] / u['c']['median'], u['b']['median'] / u['graph']['median'],
                                       u['a']['median'] / u['c']['median'], spread, 'yes' if ok else 'NO'))
    r = run_step('head')
    u = r['us']
    say()
    say('prototype-generating head, eval forward, B1 480 x 480, T = 4, n_clusters = 100, on %s' % r['device'])
    say('  (N = 4 x 60 x 60 = 14 400 points; logits of the two paths differ by %.2e of max|logit|)' % r['logits_rel_err'])
    say('  old  rows_impl = torch: op sequence + head._kmeans   ' + fmt(u['old']))
    say('  new  rows path + vss_cffm_amd.kmeans                 ' + fmt(u['new']))
    say('  old / new = %.1f' % (u['old']['median'] / u['new']['median']))
    say()
    say('all shapes: %s' % ('c faster than b beyond the measured spread' if all(verdicts) else 'c NOT faster than b beyond the spread at every shape (see above)'))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
