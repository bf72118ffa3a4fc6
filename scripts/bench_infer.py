"""Times the CFFM layer's forward on token rows for evaluation: the training forward called under no_grad (what head.eval() ran
before the inference forward existed; still reachable through ops._LayerRowsFn.apply) against the inference forward
(ops.cffm_layer_rows_infer), eager and replayed from a HIP graph.

    python scripts/bench_infer.py [--calls 200] [--repeats 3] [--depth 2] [--out profiles/infer_forward.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_infer.py --trace      (per-kernel times; its own process)

Method: every shape is warmed up first (both variants); a measurement is the time between two device events around `calls`
back-to-back calls, divided by `calls`; the variants ALTERNATE inside one process and the whole alternation is repeated `repeats`
times, so that the spread between repeats can be set against the difference between variants.  The outputs of the two variants are
compared bit for bit at every shape before anything is timed.  --trace: a few calls of each variant and nothing else (the profiler
slows the host: no end-to-end figure is taken from such a run)."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vss_cffm_amd import _lib, ops                      # noqa: E402
from vss_cffm_amd.modules import BasicLayer3d3          # noqa: E402

SHAPES = [(1, 60, 60), (2, 60, 60), (1, 60, 108)]


def layer_params(depth, dev):
    torch.manual_seed(0)
    m = BasicLayer3d3(dim=256, depth=depth, num_heads=8, window_size=7, expand_size=3, pool_method='fc', focal_level=2, focal_window=5,
                      focal_l_clips=[1, 2, 3], focal_kernel_clips=[7, 5, 3]).to(dev)
    with torch.no_grad():
        m.blocks[0].attn.relative_position_bias_table.normal_(std=0.02)
    return [p.detach() for blk in m.blocks for p in blk.param_list()]


def forward_bytes(lib, b, h, w):
    """bytes one block's forward WRITES in the two forms, from shapes (floats x 4): training = every field of cffm_block_ws the forward
    kernels store (mean1, rstd1, zall, f16 qkv, lse, ao, x1, mean2, rstd2, z2, hraw, act, x2 + the per-call prepared data bias, M,
    w_frag); inference = zall, f16 qkv, ao, x2"""
    g = ops.make_geom(lib, b, h, w)
    L = ops.block_ws_layout(lib, g)
    order = ['mean1', 'rstd1', 'M', 'zall', 'qkv', 'bias', 'lse', 'ao', 'x1', 'mean2', 'rstd2', 'z2', 'hraw', 'act', 'x2', 'w_split', 'w_frag',
             'ao_t', 'zall_t', 'total']
    size = {k: getattr(L, order[i + 1]) - getattr(L, k) for i, k in enumerate(order[:-1])}
    train = sum(size[k] for k in ('mean1', 'rstd1', 'M', 'zall', 'qkv', 'bias', 'lse', 'ao', 'x1', 'mean2', 'rstd2', 'z2', 'hraw', 'act', 'x2'))
    train += size['w_frag']                      # both fragment-ordered forms are rewritten by every call
    infer = sum(size[k] for k in ('zall', 'qkv', 'ao', 'x2'))
    return 4 * train, 4 * infer, 4 * L.total, 4 * lib.cffm_layer_infer_ws_floats(C.byref(g))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--depth', type=int, default=2)
    ap.add_argument('--trace', action='store_true', help='a few calls of each variant for a kernel trace; no timing')
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_infer.py needs a GPU: a timing taken anywhere else says nothing')
    dev = torch.device('cuda:0')
    lib = _lib.get()
    depth = a.depth
    params = layer_params(depth, dev)
    prepared = ops.layer_prepare(depth, params)
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('CFFM layer forward on rows, depth %d, %s; %d calls between two device events, %d repeats of the alternation' %
        (depth, torch.cuda.get_device_name(0), a.calls, a.repeats))
    say('variants: train = ops._LayerRowsFn.apply under no_grad (the forward evaluation used to take); infer = ops.cffm_layer_rows_infer, '
        'eager; graph = the same call replayed from a HIP graph')
    say()
    verdicts = []
    for b, h, w in SHAPES:
        x = torch.randn(b, 4, h * w, 256, device=dev)
        g = ops.make_geom(lib, b, h, w)
        ws = torch.empty(lib.cffm_layer_infer_ws_floats(C.byref(g)), dtype=torch.float32, device=dev)
        out = torch.empty(b, h * w, 256, dtype=torch.float32, device=dev)

        def train():
            with torch.no_grad():
                return ops._LayerRowsFn.apply(x, h, w, depth, *params)

        def infer():
            return ops.cffm_layer_rows_infer(x, h, w, depth, params, prepared, ws=ws, out=out)

        for _ in range(10):                       # warm-up of this shape, both variants
            yt = train()
            yi = infer()
        torch.cuda.synchronize()
        same = torch.equal(yt, yi)
        if a.trace:
            for _ in range(20):
                train()
            torch.cuda.synchronize()
            for _ in range(20):
                infer()
            torch.cuda.synchronize()
            say('B=%d %dx%d: traced 20 + 20 calls; outputs equal bit for bit: %s' % (b, h, w, same))
            continue
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            infer()
        for _ in range(10):
            graph.replay()
        torch.cuda.synchronize()
        same_graph = torch.equal(out, yt)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.calls      # us per call

        t = {'train': [], 'infer': [], 'graph': []}
        for _ in range(a.repeats):
            t['train'].append(timed(train))
            t['infer'].append(timed(infer))
            t['graph'].append(timed(graph.replay))
        wb_t, wb_i, blk_b, ws_b = forward_bytes(lib, b, h, w)
        say('B=%d %dx%d  (outputs equal bit for bit: eager %s, graph %s)' % (b, h, w, same, same_graph))
        say('  bytes written per block, from shapes: train %.1f MB, infer %.1f MB; workspace: train %.1f MB per block (x depth), infer %.1f MB in all'
            % (wb_t / 1e6, wb_i / 1e6, blk_b / 1e6, ws_b / 1e6))
        for k in ('train', 'infer', 'graph'):
            v = t[k]
            say('  %-5s us/call: %s   mean %.1f  spread (max - min) %.1f' % (k, '  '.join('%.1f' % q for q in v), sum(v) / len(v), max(v) - min(v)))
        spread = max(max(v) - min(v) for v in t.values())
        mt, mi, mg = (sum(t[k]) / len(t[k]) for k in ('train', 'infer', 'graph'))
        faster = min(t['train']) - max(t['infer']) > 0 and mt - mi > spread
        say('  train - infer %.1f us (%.1f %%), train - graph %.1f us (%.1f %%); largest spread %.1f us -> infer faster beyond the spread: %s'
            % (mt - mi, 100 * (mt - mi) / mt, mt - mg, 100 * (mt - mg) / mt, spread, 'yes' if faster else 'NO'))
        say()
        verdicts.append(faster and same and same_graph)
    if not a.trace:
        say('all shapes: %s' % ('inference forward faster than the training forward beyond the measured spread' if all(verdicts) else
                                'NOT faster beyond the spread at every shape (see above)'))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
