"""The end of a range of block backwards: the record reductions and the dx transpose share ONE launch (k_bwd_tail,
csrc/rowops_kernels.h), where k_reduce_records_multi and k_transpose ran one behind the other with k_pool_matrix_bwd_n between them; the
pooling-matrix backward now follows the shared launch.  Everything here is bit for bit.

Stage: cffm_bwd_tail + cffm_pool_matrix_bwd against the composition of the retained stages -- cffm_reduce_records, cffm_pool_matrix_bwd,
cffm_transpose (+ the addend on the frames z % 4 != 3, one fp32 addition per element either way) -- on random records laid out as the
CFFA backward lays them out: per block a buffer [2 * count][1216] whose first 512 columns are summed over all records (total 512 =
2 x 256: dgamma | dbeta), whose columns 512.. of the first `count` records are the target tail (total 50 = LNP_TAIL_TGT: dM cell 0, pool
bias 0) and of the last `count` records the reference tail (total 689 = LNP_TAIL_REF: dM cells 1..14, pool biases 1..3).  One more set
of 100 columns has a segment that accumulates into what the buffer holds and a segment that starts at column 37, in the middle of a
workgroup's columns (32 per workgroup in the shared launch, 64 in the retained one).
Record counts 1, 63, 64, 65, 257, 449: the remainder loop alone, one and two trips of the four-accumulator loop, and both together.
1, 2 and 4 blocks (with 4, only block 0 brings its 512-column set: ten sets per call), each with cffm_grad_slices_padded 0 and 1: the
three floats behind the pooling tensors are untouched or zero (nothing behind the 4-element weight).  Transposes of 1 x 49, 2 x 56 and
3 x 50 pixels x 4 frames x 256 channels with and without the addend, and no transpose at all.  Every output starts as NaN, sentinels
behind every output survive, a repeated call gives the same bits.

Layer on the 2 x 6 x 15 grid (ragged on both axes), depth 1, 2 and 3: cffm_layer_backward_full against cffm_layer_backward_rows +
cffm_transpose (+ dy of the pass-through frames) and against cffm_layer_backward_range (depth - 1 .. 0) + dy, dx and every parameter
gradient.  On the GPU also an eager call against one replay of the same call captured in a graph; there the Linear weight gradients
are held to 2e-6 of their largest entry instead, as in tests/test_gpu_parity.py (the weight-gradient group splits its contraction
differently under capture), everything else to the bit.
CPU: emulator build of the same sources; GPU: the product library."""
import ctypes as C

import pytest
import torch

from oracle import recipe as R
from tests import emu
from vss_cffm_amd import _lib, ops

NAN = float('nan')
SENTINEL = -7.0
GUARD = 8                         # floats behind every output
RSTRIDE, TAIL_TGT, TAIL_REF = 1216, 50, 689

# (records, blocks, grad_slices_padded, transpose (clips, pixels, addend) or None)
CASES = [(1, 1, 0, (1, 49, True)),
         (63, 2, 1, (2, 56, False)),
         (64, 4, 0, None),
         (65, 1, 1, (3, 50, True)),
         (257, 2, 0, (3, 50, False)),
         (449, 4, 1, (2, 56, True)),
         (64, 1, 0, (1, 49, False))]
IDS = ['r%d-n%d-pad%d-%s' % (c, n, p, 'none' if t is None else '%dx%d%s' % (t[0], t[1], '+dy' if t[2] else '')) for c, n, p, t in CASES]


def P(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def stream_of(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == 'cuda' else None


def settle(device):
    if device.type == 'cuda':
        torch.cuda.synchronize(device)


def same(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def record_set(rec, off, count, stride, total, segs):
    s = _lib.RecordSet()
    s.rec, s.count, s.stride, s.total, s.nseg = P(rec, off), count, stride, total, len(segs)
    for k, (o, w, acc, out, out_off) in enumerate(segs):
        s.off[k], s.width[k], s.accumulate[k], s.out[k] = o, w, acc, out.data_ptr() + 4 * out_off
    return s


def run_stage(lib, device, count, n, pads, tr):
    gen = torch.Generator().manual_seed(7000 + 10 * count + n)
    rn = lambda *s: torch.randn(*s, generator=gen).to(device)
    recs = [rn(2 * count, RSTRIDE) for _ in range(n)]
    extra = rn(count, 100)
    pre = rn(37)
    st = stream_of(device)
    if tr is not None:
        clips, pix, with_add = tr
        src = rn(clips * 4, pix, 256)
        addend = rn(clips * 4, 256, pix) if with_add else None

    def outputs():
        out = {}

        def buf(name, numel, fill=None):
            t = torch.full((numel + GUARD,), NAN, device=device)
            t[numel:] = SENTINEL
            if fill is not None:
                t[:numel] = fill
            out[name] = t
            return t
        for d in range(n):
            for name, numel in (('dgamma', 256), ('dbeta', 256), ('dM', 15 * 49), ('w0', 49), ('w1', 49), ('w2', 9), ('w3', 4), ('b0', 1), ('b1', 1),
                                ('b2', 1), ('b3', 1)):
                if d == 0 or n <= 2 or not name.startswith('d') or name == 'dM':      # (four blocks: only block 0 brings dgamma | dbeta)
                    buf('%d.%s' % (d, name), numel)
        buf('x.acc', 37, pre)
        buf('x.mid', 63)
        if tr is not None:
            buf('dx', clips * 4 * 256 * pix)
        return out

    def sets_of(out):
        sets = []
        for d in range(n):
            o = lambda k: out['%d.%s' % (d, k)]
            if d == 0 or n <= 2:
                sets.append(record_set(recs[d], 0, 2 * count, RSTRIDE, 512, [(0, 256, 0, o('dgamma'), 0), (256, 256, 0, o('dbeta'), 0)]))
            sets.append(record_set(recs[d], 512, count, RSTRIDE, TAIL_TGT,
                                   [(0, 49, 0, o('dM'), 0), (49, 1, 0, o('b0'), 0)]))
            sets.append(record_set(recs[d], count * RSTRIDE + 512, count, RSTRIDE, TAIL_REF,
                                   [(0, 686, 0, o('dM'), 49)] + [(686 + i, 1, 0, o('b%d' % (i + 1)), 0) for i in range(3)]))
        sets.append(record_set(extra, 0, count, 100, 100, [(0, 37, 1, out['x.acc'], 0), (37, 63, 0, out['x.mid'], 0)]))
        return (_lib.RecordSet * len(sets))(*sets)

    def pools_of(out):
        pools = (_lib.PoolGrads * n)()
        for d in range(n):
            pools[d].dM = P(out['%d.dM' % d])
            pools[d].dpool_w = (C.c_void_p * 4)(*[out['%d.w%d' % (d, q)].data_ptr() for q in range(4)])
            pools[d].dpool_b = (C.c_void_p * 4)(*[out['%d.b%d' % (d, q)].data_ptr() for q in range(4)])
        return pools

    def fused():
        out = outputs()
        sets, pools = sets_of(out), pools_of(out)
        t = None
        if tr is not None:
            t = _lib.TailTranspose()
            t.src, t.dst, t.batch, t.rows, t.cols, t.src_bs, t.dst_bs = P(src), P(out['dx']), clips * 4, pix, 256, pix * 256, pix * 256
            t.addend, t.add_mod, t.add_skip = (P(addend) if with_add else None), 4, 3
        lib.cffm_grad_slices_padded(pads)
        try:
            _lib.check(lib.cffm_bwd_tail(len(sets), sets, C.byref(t) if t is not None else None, st), lib)
            _lib.check(lib.cffm_pool_matrix_bwd(n, pools, st), lib)
        finally:
            lib.cffm_grad_slices_padded(0)
        settle(device)
        return {k: v.cpu() for k, v in out.items()}

    def composed():
        out = outputs()
        sets, pools = sets_of(out), pools_of(out)
        lib.cffm_grad_slices_padded(pads)
        try:
            _lib.check(lib.cffm_reduce_records(len(sets), sets, st), lib)
            _lib.check(lib.cffm_pool_matrix_bwd(n, pools, st), lib)
        finally:
            lib.cffm_grad_slices_padded(0)
        if tr is not None:
            _lib.check(lib.cffm_transpose(P(src), P(out['dx']), clips * 4, pix, 256, pix * 256, pix * 256, st), lib)
            settle(device)
            if with_add:
                v = out['dx'][:clips * 4 * 256 * pix].view(clips, 4, 256, pix)
                v[:, :3] += addend.view(clips, 4, 256, pix)[:, :3]
        settle(device)
        return {k: v.cpu() for k, v in out.items()}

    a, b = fused(), composed()
    assert set(a) == set(b)
    for k in sorted(a):
        numel = a[k].numel() - GUARD
        assert torch.isfinite(a[k][:numel]).all(), '%s: not every element written' % k
        assert same(a[k], b[k]), '%s differs from the composition of the retained stages' % k
        tail = a[k][numel:]
        name = k.split('.')[-1]
        if pads and name in ('w0', 'w1', 'w2', 'b0', 'b1', 'b2', 'b3'):
            assert bool((tail[:3] == 0).all()) and not bool(torch.signbit(tail[:3]).any()), '%s: pad floats' % k
            tail = tail[3:]
        assert bool((tail == SENTINEL).all()), '%s: written past its end' % k
    again = fused()
    for k in a:
        assert same(a[k], again[k]), '%s: a repeated call gives other bits' % k


@pytest.mark.parametrize('count,n,pads,tr', CASES, ids=IDS)
def test_bwd_tail_stage_emulated(count, n, pads, tr):
    run_stage(emu.lib(), torch.device('cpu'), count, n, pads, tr)


@pytest.mark.gpu
@pytest.mark.parametrize('count,n,pads,tr', CASES, ids=IDS)
def test_bwd_tail_stage_gpu(count, n, pads, tr):
    run_stage(_lib.get(), torch.device('cuda:0'), count, n, pads, tr)


def test_bwd_tail_bad_arguments_are_reported():
    lib = emu.lib()
    buf = torch.zeros(4096)
    good = record_set(buf, 0, 2, 100, 100, [(0, 100, 0, buf, 2048)])
    for bad in (record_set(buf, 0, 0, 100, 100, []), record_set(buf, 0, 2, 98, 100, []), record_set(buf, 0, 2, 100, 100, [(90, 20, 0, buf, 2048)])):
        assert lib.cffm_bwd_tail(1, (_lib.RecordSet * 1)(bad), None, None) != 0
        assert b'bwd_tail' in lib.cffm_last_error()
        assert lib.cffm_reduce_records(1, (_lib.RecordSet * 1)(bad), None) != 0
    assert lib.cffm_bwd_tail(11, (_lib.RecordSet * 11)(*[good] * 11), None, None) != 0
    assert lib.cffm_bwd_tail(1, (_lib.RecordSet * 1)(good), C.byref(_lib.TailTranspose()), None) != 0        # (null fields of the transpose)
    assert lib.cffm_pool_matrix_bwd(0, None, None) != 0
    assert lib.cffm_pool_matrix_bwd(5, (_lib.PoolGrads * 5)(), None) != 0
    assert lib.cffm_pool_matrix_bwd(1, (_lib.PoolGrads * 1)(), None) != 0                                     # (null fields of the block)


# ---------------------------------------------------------------------------------------------- layer level
GRID = (2, 6, 15)


def flat_params(st, depth, device):
    return [st['blocks.%d.%s' % (i, k)].clone().to(device) for i in range(depth) for k, _, _ in ops.BLOCK_PARAM_KEYS]


def run_layer(lib, device, depth):
    b, h, w = GRID
    hw, img = h * w, h * w * 256
    state = R.layer_state(depth, seed=30 + depth)
    x = R.synth_input('x', (b, 4, 256, h, w), seed=31).to(device).contiguous()
    dy = R.synth_input('g', (b, 4, 256, h, w), seed=32, scale=1.0).to(device).contiguous()
    params = flat_params(state, depth, device)
    st = stream_of(device)
    g = ops.make_geom(lib, b, h, w)
    ks, qd, ip, ii = ops.device_tables(h, w, device)
    ps = ops.block_structs(params, depth)
    saved, scratch = ops._layer_buffers(lib, g, depth, device)
    y = torch.empty_like(x)
    _lib.check(lib.cffm_layer_forward_full(C.byref(g), depth, ps, P(x), P(y), P(ks), P(qd), P(saved), P(scratch), st), lib)
    settle(device)

    def fresh():
        grads = [torch.full_like(p, NAN) for p in params]
        return grads, ops.block_structs(grads, depth), torch.full((x.numel() + GUARD,), NAN, device=device)

    def full(stream):
        grads, gs, dx = fresh()
        dx[x.numel():] = SENTINEL
        _lib.check(lib.cffm_layer_backward_full(C.byref(g), depth, ps, gs, P(dy), P(dx), P(ks), P(qd), P(ip), P(ii), P(saved), P(scratch),
                                                depth - 1, 0, stream), lib)
        return grads, dx

    grads_a, dx_a = full(st)
    settle(device)
    assert bool((dx_a[x.numel():] == SENTINEL).all())
    dx_a = dx_a[:x.numel()].view_as(x)
    assert torch.isfinite(dx_a).all()
    # ---- the range entry point over the same blocks: dx without dy of the pass-through frames
    grads_b, gs, dx_b = fresh()
    _lib.check(lib.cffm_layer_backward_range(C.byref(g), depth, ps, gs, P(dy, 3 * img), 4 * img, P(dx_b), P(ks), P(qd), P(ip), P(ii), P(saved),
                                             P(scratch), depth - 1, 0, st), lib)
    settle(device)
    dx_b = dx_b[:x.numel()].view_as(x).clone()
    dx_b[:, :3] += dy[:, :3]
    # ---- token rows + transposes (the forward's saved state is that of the rows entry point as well: same kernels behind the transposes)
    grads_c, gs, _ = fresh()
    x_rows, dy_rows = torch.empty(b, 4, hw, 256, device=device), torch.empty(b, hw, 256, device=device)
    dx_rows, dx_c = torch.full((b, 4, hw, 256), NAN, device=device), torch.empty_like(x)
    saved_r, scratch_r = ops._layer_buffers(lib, g, depth, device)
    y_rows = torch.empty(b, hw, 256, device=device)
    _lib.check(lib.cffm_transpose(P(x), P(x_rows), 4 * b, 256, hw, img, img, st), lib)
    _lib.check(lib.cffm_layer_forward_rows(C.byref(g), depth, ps, P(x_rows), P(y_rows), P(ks), P(qd), P(saved_r), P(scratch_r), st), lib)
    _lib.check(lib.cffm_transpose(P(dy, 3 * img), P(dy_rows), b, 256, hw, 4 * img, img, st), lib)
    _lib.check(lib.cffm_layer_backward_rows(C.byref(g), depth, ps, gs, P(x_rows), P(dy_rows), P(dx_rows), P(ks), P(qd), P(ip), P(ii), P(saved_r),
                                            P(scratch_r), st), lib)
    _lib.check(lib.cffm_transpose(P(dx_rows), P(dx_c), 4 * b, hw, 256, img, img, st), lib)
    settle(device)
    dx_c[:, :3] += dy[:, :3]
    for what, dx_o, grads_o in (('range', dx_b, grads_b), ('rows', dx_c, grads_c)):
        assert same(dx_a, dx_o), 'input gradient differs from the %s form' % what
        for i, (ga, go) in enumerate(zip(grads_a, grads_o)):
            assert torch.isfinite(ga).all(), i
            assert same(ga, go), 'gradient of parameter %d (%s) differs from the %s form' % (i, ops.BLOCK_PARAM_KEYS[i % ops.NPB][0], what)
    if device.type != 'cuda':
        return
    # ---- eager against one replay of the captured call
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        full(stream_of(device))
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grads_g, dx_g = full(stream_of(device))
    for t in grads_g + [dx_g[:x.numel()]]:
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    assert same(dx_g[:x.numel()].view_as(x), dx_a), 'replayed input gradient differs from the eager one'
    for i, (gg, ga) in enumerate(zip(grads_g, grads_a)):
        k = ops.BLOCK_PARAM_KEYS[i % ops.NPB][0]
        if k.endswith('.weight') and gg.dim() == 2 and 'pool' not in k:
            assert float((gg - ga).abs().max()) <= 2e-6 * float(ga.abs().max()), (i, k)
        else:
            assert same(gg, ga), 'replayed gradient of parameter %d (%s) differs from the eager one' % (i, k)


@pytest.mark.parametrize('depth', [1, 2, 3])
def test_layer_backward_forms_agree_emulated(depth):
    with emu.active():
        run_layer(emu.lib(), torch.device('cpu'), depth)


@pytest.mark.gpu
@pytest.mark.parametrize('depth', [1, 2, 3])
def test_layer_backward_forms_agree_gpu(depth):
    run_layer(_lib.get(), torch.device('cuda:0'), depth)
