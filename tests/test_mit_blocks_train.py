"""The blocks of a MiT stage as one library call per direction (include/cffm_hip.h: cffm_mit_blocks_train_fwd / _bwd,
vss_cffm_amd.mit_blocks_train), the LayerNorm backward with its neighbouring adds fused in (cffm_ln_rows_bwd_add) and the backbone's
``block_impl`` switch, on the CPU through the fiber emulator.  The GPU half is tests/test_mit_blocks_train_gpu.py and shares the
run_*(device) bodies below.

A. cffm_ln_rows_bwd_add, raw C ABI.  Inputs as tests/test_ln_train.py (seed 0) plus dout_b = randn and dres = randn.  Bit-equal to
   cffm_ln_rows_bwd(x, gamma, dout_a + dout_b) followed by dres + dx with both adds done by torch in fp32 on the same device; with
   dout_b = dres = NULL bit-equal to cffm_ln_rows_bwd; and inside test_ln_train's rule against the fp64 sequence:
   max|t - t64| <= 4 noise_t + 2^-23 A_t, noise_t = max|stock fp32 sequence on the CPU - fp64|, A_t = the same backward with magnitudes.
B. The stage call against the composition of the existing ops (layer_norm_rows, linear_rows, sr_reduce, sra_attention, dwconv_gelu chained
   as Block.forward chains them with every switch on 'hip'), explicit DropPath factors: y, dx and every parameter gradient bit-equal.
   One fp64 anchor (case a): y and dx against the fp64 Block chain on the CPU, gate = 4 |split - fp64| + 2^-23 max|fp64|, split = the
   same chain with tests.test_linear_rows.split_linear_both_ways.
C. The backbone switch: mit_b0, [2,3,64,64], train mode, drop path 0.1, every other switch on 'hip' on both sides: bit-equal outputs,
   input gradient and all parameter gradients, one call per stage and direction.  (On the GPU the two parameters of patch_embed1.proj
   are compared in a second pass whose image does not require grad: see run_backbone.)

Measured, error / gate = ratio (A: the largest over dx, dgamma, dbeta; the gates move a little between machines):
    A, through the emulator (CPU)   (1,16) 0.13  (7,36) 0.17  (33,160) 0.20  (5,260) 0.25  (6,512) 0.18  (16389,64) 0.17
    A, on the MI355X                (1,16) 0.13  (7,36) 0.17  (33,160) 0.19  (5,260) 0.16  (6,512) 0.18  (16389,64) 0.20
    B, case a, through the emulator y 0.25  dx 0.21
    B, case a, on the MI355X        y 0.22  dx 0.17
"""
import ctypes as C
import functools
import os
from functools import partial

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import vss_cffm_amd as V
from tests import emu
from tests import test_backbone as TB
from tests import test_linear_rows as TL
from tests import test_ln_train as TN
from tests.test_mit_stage import MARGIN
from tests.test_mixffn import CallSpy
from vss_cffm_amd import _lib, ops
from vss_cffm_amd import backbone as B

CPU = torch.device('cpu')
ULP = 2.0 ** -23
EPS = TN.EPS
TAIL = 64
KEEP = 1 / 0.9
NAN = float('nan')
# (5, 260) and (6, 512) take the V = 2 path; the last one goes over the grid cap (the last shape of test_ln_train.ROWS)
LN_ROWS = [(1, 16), (7, 36), (33, 160), (5, 260), (6, 512), TN.ROWS[-1]]
LN_IDS = ['%dx%d' % s for s in LN_ROWS]
ADD, LN_BWD = 'cffm_ln_rows_bwd_add', 'cffm_ln_rows_bwd'
FWD, BWD = 'cffm_mit_blocks_train_fwd', 'cffm_mit_blocks_train_bwd'
SIZES = ('cffm_mit_blocks_train_saved_floats', 'cffm_mit_blocks_train_fwd_ws_floats', 'cffm_mit_blocks_train_bwd_ws_floats')


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else C.c_void_p(0)


_st, _sync = TN._st, TN._sync


# ---------------------------------------------------------------------------------------------- A. the fused LayerNorm backward
@functools.lru_cache(maxsize=None)
def ln_inputs(shape):
    """test_ln_train's x, gamma, beta, dout (= dout_a) and, from a generator of their own, dout_b and dres"""
    x, gamma, beta, dout = TN.make_inputs('rows', shape)
    g = torch.Generator().manual_seed(0)
    return x, gamma, beta, dout, torch.randn(shape, generator=g), torch.randn(shape, generator=g)


def ln_sequence(x, gamma, beta, da, db, dres):
    """F.layer_norm's backward with dout = da + db, then dres + dx, in the dtype of x"""
    x, gamma, beta = (t.detach().clone().requires_grad_(True) for t in (x, gamma, beta))
    F.layer_norm(x, (gamma.numel(),), gamma, beta, EPS).backward(da + db)
    return {'dx': dres + x.grad, 'dgamma': gamma.grad, 'dbeta': beta.grad}


class LnYard:
    """the fp64 sequence of one shape, its distance to the stock fp32 one and the magnitudes A_t; computed once and left unchanged"""

    def __init__(self, shape):
        x, gamma, beta, da, db, dres = ln_inputs(shape)
        self.want = ln_sequence(*(t.double() for t in (x, gamma, beta, da, db, dres)))
        f32 = ln_sequence(x, gamma, beta, da, db, dres)
        self.noise = {k: float((v.double() - self.want[k]).abs().max()) for k, v in f32.items()}
        xr, dr = x.double(), da.double().abs() + db.double().abs()
        d = xr - xr.mean(1, keepdim=True)
        rstd = 1 / torch.sqrt((d * d).mean(1, keepdim=True) + EPS)
        xh, g = (d * rstd).abs(), gamma.double().abs() * dr
        self.mag = {'dx': float((dres.double().abs() + rstd * (g + g.mean(1, keepdim=True) + xh * (g * xh).mean(1, keepdim=True))).max()),
                    'dgamma': float((dr * xh).sum(0).max()), 'dbeta': float(dr.sum(0).max())}

    def gate(self, k):
        return 4 * self.noise[k] + ULP * self.mag[k]


@functools.lru_cache(maxsize=None)
def ln_yard(shape):
    return LnYard(shape)


def raw_add(lib, shape, x, gamma, da, db, dres, inplace=False, ws_fill=NAN, null=(), off=None, alias=None, eps=EPS):
    """one cffm_ln_rows_bwd_add call -> (rc, dx, dgamma, dbeta), each with TAIL more floats behind it than it needs, NaN-prefilled (dx:
    dres's values with `inplace`, and dres is then dx itself).  `null`: names passed as null pointers; `off` = (name, bytes): that
    pointer moved; `alias` = name: dx is that pointer"""
    m, c = shape
    dx = torch.full((m * c + TAIL,), NAN, device=x.device)
    if inplace:
        dx[:m * c] = dres.reshape(-1)
        dres = dx
    dgamma, dbeta = (torch.full((c + TAIL,), NAN, device=x.device) for _ in range(2))
    ws = torch.full((max(lib.cffm_ln_bwd_workspace_bytes(max(m, 1), c if 16 <= c <= 512 and c % 4 == 0 else 64, 1), 16) // 4 + TAIL,),
                    ws_fill, device=x.device)
    ptrs = {'x': x, 'gamma': gamma, 'dout_a': da, 'dout_b': db, 'dres': dres, 'dx': dx, 'dgamma': dgamma, 'dbeta': dbeta, 'ws': ws}
    if alias:
        ptrs['dx'] = ptrs[alias]
    args = [_p(None if n in null else t, off[1] if off and off[0] == n else 0) for n, t in ptrs.items()]
    rc = getattr(lib, ADD)(*args, m, c, eps, _st(x))
    return rc, dx, dgamma, dbeta


def run_add(lib, device, shape, x, gamma, da, db, dres, **kw):
    """one raw call that must succeed -> dx, dgamma, dbeta in their shapes; the TAIL floats behind each are still NaN"""
    rc, dx, dgamma, dbeta = raw_add(lib, shape, x, gamma, da, db, dres, **kw)
    assert rc == 0, lib.cffm_last_error()
    _sync(device)
    out = {}
    for k, t, s in (('dx', dx, shape), ('dgamma', dgamma, (shape[1],)), ('dbeta', dbeta, (shape[1],))):
        out[k], tail = TN.split_tail(t, s)
        assert bool(tail.isnan().all()), '%s: written past the end' % k
        assert not bool(out[k].isnan().any()), '%s: not every element written' % k
    return out


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in b) and set(a) == set(b)


def run_ln_add(device, shape):
    lib = _lib.get()
    x, gamma, _, da, db, dres = (t.to(device) for t in ln_inputs(shape))
    # (i) without the two optional operands: cffm_ln_rows_bwd's bits
    plain = TN.run_raw(lib, device, 'rows', shape, x, gamma, da)
    assert same(run_add(lib, device, shape, x, gamma, da, None, None), plain)
    # (ii) all given: the per-op path's bits -- torch's add, the library's backward, torch's add
    want = TN.run_raw(lib, device, 'rows', shape, x, gamma, da + db)
    want['dx'] = dres + want['dx']
    got = run_add(lib, device, shape, x, gamma, da, db, dres)
    assert same(got, want)
    only_b = TN.run_raw(lib, device, 'rows', shape, x, gamma, da + db)
    assert same(run_add(lib, device, shape, x, gamma, da, db, None), only_b)
    # (iii) the fp64 sequence
    y = ln_yard(shape)
    for k, t in got.items():
        err = float((t.cpu().double() - y.want[k]).abs().max())
        print('ln_rows_bwd_add %s %s: max err %.3e / gate %.3e = %.2f (4 x noise %.3e + 2^-23 x %.3e)'
              % (shape, k, err, y.gate(k), err / y.gate(k), y.noise[k], y.mag[k]))
        assert err <= y.gate(k), (shape, k, err, y.gate(k))
    # (iv) in place, (v) a zero-filled and a second NaN-filled workspace
    assert same(run_add(lib, device, shape, x, gamma, da, db, dres, inplace=True), want)
    for fill in (0.0, NAN):
        assert same(run_add(lib, device, shape, x, gamma, da, db, dres, ws_fill=fill), want)


def run_ln_add_errors(device):
    """every refusal: non-zero, cffm_last_error set, the NaN-prefilled dx / dgamma / dbeta still NaN"""
    lib = _lib.get()
    x, da, db, dres = (torch.ones(4096, device=device) for _ in range(4))
    gamma = torch.ones(1024, device=device)
    cases = [((2, 12), {}), ((2, 516), {}), ((0, 64), {}), ((2, 64), {'eps': -1.0}), ((2, 64), {'eps': NAN})]
    cases += [((2, 64), {'null': (n,)}) for n in ('x', 'gamma', 'dout_a', 'dx', 'dgamma', 'dbeta', 'ws')]
    cases += [((2, 64), {'off': (n, 4)}) for n in ('x', 'gamma', 'dout_a', 'dout_b', 'dres', 'dx', 'dgamma', 'dbeta', 'ws')]
    for shape, kw in cases:
        rc, dx, dgamma, dbeta = raw_add(lib, shape, x, gamma, da, db, dres, **kw)
        assert rc != 0 and lib.cffm_last_error() != b'', (shape, kw)
        _sync(device)
        assert all(bool(t.isnan().all()) for t in (dx, dgamma, dbeta)), (shape, kw)
    for name, t in (('x', x), ('dout_a', da), ('dout_b', db)):       # dx == x / dout_a / dout_b: refused, the operand stays as it is
        rc, _, dgamma, dbeta = raw_add(lib, (2, 64), x, gamma, da, db, dres, alias=name)
        assert rc != 0 and lib.cffm_last_error() != b'', name
        _sync(device)
        assert bool((t == 1).all()) and bool(dgamma.isnan().all()) and bool(dbeta.isnan().all()), name


# ---------------------------------------------------------------------------------------------- B. the stage call
# name -> B, H, W, C, heads, hidden, sr_ratio, depth, bias on q / kv, scales
CASES = {
    'a': (2, 8, 8, 32, 1, 128, 2, 2, True, 'mixed'),
    'b': (2, 6, 10, 64, 1, 256, 1, 1, False, None),
    'c': (1, 9, 7, 64, 2, 80, 4, 1, True, 'ones'),       # edge pixels outside any sr window; a hidden size that is no multiple of 16
    'd': (1, 16, 16, 32, 1, 128, 8, 1, True, None),
    'e': (1, 4, 4, 320, 5, 1280, 2, 2, True, None),      # the V = 2 LayerNorm forms
}


def make_blocks(name, dtype=torch.float32):
    """the blocks of a case with seeded parameters of realistic sizes (the module's own init leaves every bias 0 and every gamma 1)"""
    _, _, _, c, heads, hidden, sr, depth, qkv_bias, _ = CASES[name]
    blocks = nn.ModuleList([B.Block(dim=c, num_heads=heads, mlp_ratio=hidden / c, qkv_bias=qkv_bias, sr_ratio=sr,
                                    norm_layer=partial(nn.LayerNorm, eps=1e-6)) for _ in range(depth)])
    assert blocks[0].mlp.fc1.out_features == hidden
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for k, p in blocks.named_parameters():
            r = torch.randn(p.shape, generator=g)
            if 'norm' in k:
                p.copy_(1 + 0.3 * r if k.endswith('weight') else 0.3 * r)
            elif k.endswith('bias'):
                p.copy_(0.2 * r)
            elif 'dwconv' in k:
                p.copy_(0.4 * r)
            else:
                p.copy_(r / (p[0].numel() ** 0.5))
    return blocks.to(dtype).train()


def make_scales(name):
    b, depth, kind = CASES[name][0], CASES[name][7], CASES[name][9]
    if kind is None:
        return None
    s = torch.ones(depth, 2, b)
    if kind == 'mixed':
        s[0, 0] = torch.tensor([0., KEEP])
        s[1, 1] = torch.tensor([KEEP, 0.])
    return s


@functools.lru_cache(maxsize=None)
def stage_inputs(name):
    b, h, w, c = CASES[name][:4]
    g = torch.Generator().manual_seed(12)
    return 1.5 * torch.randn(b, h * w, c, generator=g) + 0.5, torch.randn(b, h * w, c, generator=g)


def compose(x, blocks, H, W, scales):
    """the per-op path: Block.forward's chain with every switch on 'hip' and the DropPath factors handed in"""
    for i, blk in enumerate(blocks):
        a, m = blk.attn, blk.mlp
        sa, sm = (scales[i, 0], scales[i, 1]) if scales is not None else (None, None)
        z1 = V.layer_norm_rows(x, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)
        src = z1
        if a.sr_ratio > 1:
            src = V.sr_reduce(z1, a.sr.weight, a.sr.bias, a.norm.weight, a.norm.bias, H, W, a.sr_ratio, a.norm.eps)
        kv = V.linear_rows(src, a.kv.weight, a.kv.bias)
        ao = V.sra_attention(V.linear_rows(z1, a.q.weight, a.q.bias), kv, a.num_heads, a.scale)
        x = V.linear_rows(ao, a.proj.weight, a.proj.bias, x, sa)
        z2 = V.layer_norm_rows(x, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
        act = V.dwconv_gelu(V.linear_rows(z2, m.fc1.weight, m.fc1.bias), m.dwconv.dwconv.weight, m.dwconv.dwconv.bias, H, W)
        x = V.linear_rows(act, m.fc2.weight, m.fc2.bias, x, sm)
    return x


def chain64(x, blocks, H, W, scales):
    """the reference's Block chain in the dtype of x (stock ops), the factors handed in"""
    for i, blk in enumerate(blocks):
        sa, sm = (scales[i, 0].view(-1, 1, 1), scales[i, 1].view(-1, 1, 1)) if scales is not None else (1., 1.)
        x = x + sa * blk.attn(blk.norm1(x), H, W)
        x = x + sm * blk.mlp(blk.norm2(x), H, W)
    return x


def passes(fn, x, blocks, dy):
    """forward + backward of fn(x) -> (y, dx, {name: grad})"""
    blocks.zero_grad(set_to_none=True)
    xg = x.detach().clone().requires_grad_(True)
    y = fn(xg)
    y.backward(dy)
    return y.detach(), xg.grad, {k: p.grad for k, p in blocks.named_parameters()}


def stage_on(device, name):
    x, dy = (t.to(device) for t in stage_inputs(name))
    s = make_scales(name)
    return make_blocks(name).to(device), x, dy, (None if s is None else s.to(device))


def run_stage_case(device, name):
    """y, dx and every parameter gradient bit-equal to the composition of the existing ops; a second call gives the same bits"""
    h, w = CASES[name][1:3]
    blocks, x, dy, scales = stage_on(device, name)
    want = passes(lambda t: compose(t, blocks, h, w, scales), x, blocks, dy)
    got = passes(lambda t: V.mit_blocks_train(t, blocks, h, w, scales), x, blocks, dy)
    assert torch.equal(got[0], want[0]), 'y'
    assert torch.equal(got[1], want[1]), 'dx'
    assert set(got[2]) == set(want[2]) and all(g is not None for g in got[2].values())
    for k in want[2]:
        assert torch.equal(got[2][k], want[2][k]), k
    again = passes(lambda t: V.mit_blocks_train(t, blocks, h, w, scales), x, blocks, dy)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]) and all(torch.equal(again[2][k], got[2][k]) for k in got[2])


def cfg_of(name, blocks):
    b, h, w, c = CASES[name][:4]
    return ops.mit_blocks_cfg((b, h * w, c), h, w, blocks)


def raw_stage(lib, device, name, fill):
    """both calls through the raw C ABI with `saved` and both workspaces pre-filled with `fill` -> (y, dx, the gradients), TAIL floats
    behind y and dx still NaN"""
    blocks, x, dy, scales = stage_on(device, name)
    cfg = cfg_of(name, blocks)
    tensors = ops._mit_block_tensors(blocks)
    grads = [None if t is None else torch.full_like(t, NAN) for t in tensors]
    pairs = None if scales is None else [(scales[i, 0], scales[i, 1]) for i in range(cfg.depth)]
    sizes = [getattr(lib, n)(C.byref(cfg)) for n in SIZES]
    assert sizes[0] > 0 and sizes[1] >= 0 and sizes[2] > 0, sizes
    saved, wf, wb = (torch.full((n + TAIL,), fill, device=device) for n in sizes)
    y, dx = (torch.full((x.numel() + TAIL,), NAN, device=device) for _ in range(2))
    ps, ss = ops._mit_block_structs(tensors, cfg.depth), ops._mit_scale_structs(pairs, cfg.depth)
    assert lib.cffm_mit_blocks_train_fwd(C.byref(cfg), ps, ss, _p(x), _p(y), _p(saved), _p(wf), _st(x)) == 0, lib.cffm_last_error()
    assert lib.cffm_mit_blocks_train_bwd(C.byref(cfg), ps, ss, ops._mit_block_structs(grads, cfg.depth), _p(x), _p(saved), _p(dy), _p(dx),
                                         _p(wb), _st(x)) == 0, lib.cffm_last_error()
    _sync(device)
    for t in (y, dx):
        assert bool(t[x.numel():].isnan().all()) and bool(t[:x.numel()].isfinite().all())
    assert bool(saved[sizes[0]:].eq(fill).all() if fill == 0 else saved[sizes[0]:].isnan().all()), 'written past the end of saved'
    assert bool(wb[sizes[2]:].eq(fill).all() if fill == 0 else wb[sizes[2]:].isnan().all()), 'written past the end of ws'
    return y[:x.numel()], dx[:x.numel()], [g for g in grads if g is not None]


def run_stage_poison(device, name='a'):
    """NaN-filled and zero-filled saved / ws: finite results, the same bits, and those of the autograd call"""
    lib = _lib.get()
    runs = [raw_stage(lib, device, name, fill) for fill in (NAN, 0.0)]
    for a, b in zip(runs[0][:2] + tuple(runs[0][2]), runs[1][:2] + tuple(runs[1][2])):
        assert bool(a.isfinite().all()) and torch.equal(a, b)
    h, w = CASES[name][1:3]
    blocks, x, dy, scales = stage_on(device, name)
    y, dx, grads = passes(lambda t: V.mit_blocks_train(t, blocks, h, w, scales), x, blocks, dy)
    assert torch.equal(y.reshape(-1), runs[0][0]) and torch.equal(dx.reshape(-1), runs[0][1])
    for g, r in zip([p.grad for p in ops._mit_block_tensors(blocks) if p is not None], runs[0][2]):
        assert torch.equal(g, r)


def run_stage_dropped(device):
    """a sample whose factor is 0 in both lines of a block leaves the block with the input's bits (and hands its gradient through)"""
    blocks, x, dy, _ = stage_on(device, 'a')
    one = blocks[:1]
    scales = torch.tensor([[[0., KEEP], [0., KEEP]]], device=device)
    y, dx, _ = passes(lambda t: V.mit_blocks_train(t, one, 8, 8, scales), x, one, dy)
    assert torch.equal(y[0], x[0]) and not torch.equal(y[1], x[1])
    assert torch.equal(dx[0], dy[0]) and not torch.equal(dx[1], dy[1])
    pairs = [(scales[0, 0], None)]                                    # the list form, a factor missing: as ones in its place
    y2 = V.mit_blocks_train(x, one, 8, 8, pairs)
    y3 = V.mit_blocks_train(x, one, 8, 8, torch.tensor([[[0., KEEP], [1., 1.]]], device=device))
    assert torch.equal(y2, y3)


def run_stage_needs_grad(device, name='a'):
    """a parameter with requires_grad=False gets None and the others keep their bits; torch.autograd.grad with only x requiring grad"""
    h, w = CASES[name][1:3]
    blocks, x, dy, scales = stage_on(device, name)
    _, dx, grads = passes(lambda t: V.mit_blocks_train(t, blocks, h, w, scales), x, blocks, dy)
    frozen = ('0.attn.q.weight', '1.mlp.fc2.bias', '0.norm1.weight')
    for k, p in blocks.named_parameters():
        p.requires_grad_(k not in frozen)
    _, dx2, grads2 = passes(lambda t: V.mit_blocks_train(t, blocks, h, w, scales), x, blocks, dy)
    assert torch.equal(dx2, dx)
    for k in grads:
        assert (grads2[k] is None) if k in frozen else torch.equal(grads2[k], grads[k]), k
    for p in blocks.parameters():
        p.requires_grad_(False)
    xg = x.clone().requires_grad_(True)
    dx3, = torch.autograd.grad(V.mit_blocks_train(xg, blocks, h, w, scales), xg, dy)
    assert torch.equal(dx3, dx)
    with torch.no_grad():                                             # no graph, the same forward
        y = V.mit_blocks_train(xg, blocks, h, w, scales)
    assert y.grad_fn is None and torch.equal(y, compose(x, blocks, h, w, scales).detach())


@functools.lru_cache(maxsize=None)
def anchor():
    """case a in fp64 on the CPU: the Block chain, and the gates 4 |split - fp64| + 2^-23 max|fp64| of y and dx"""
    x, dy = (t.double() for t in stage_inputs('a'))
    scales = make_scales('a').double()
    with TL.no_override():
        blocks = make_blocks('a', torch.float64)
        y, dx, _ = passes(lambda t: chain64(t, blocks, 8, 8, scales), x, blocks, dy)
        with TL.counted_linear(TL.split_linear_both_ways):
            ys, dxs, _ = passes(lambda t: chain64(t, blocks, 8, 8, scales), x, blocks, dy)
    gate = lambda s, t: MARGIN * float((s - t).abs().max()) + ULP * float(t.abs().max())       # noqa: E731
    return y, dx, gate(ys, y), gate(dxs, dx)


def run_stage_anchor(device):
    y64, dx64, gy, gdx = anchor()
    blocks, x, dy, scales = stage_on(device, 'a')
    y, dx, _ = passes(lambda t: V.mit_blocks_train(t, blocks, 8, 8, scales), x, blocks, dy)
    errs = {'y': (float((y.cpu().double() - y64).abs().max()), gy), 'dx': (float((dx.cpu().double() - dx64).abs().max()), gdx)}
    for k, (err, gate) in errs.items():
        print('mit_blocks_train case a %s: err %.3e / gate %.3e = %.2f' % (k, err, gate, err / gate))
    for k, (err, gate) in errs.items():
        assert err <= gate, (k, err, gate)


def run_stage_errors(device):
    """every refusal: non-zero, cffm_last_error set, nothing enqueued (the NaN-prefilled y / dx still NaN); the size queries < 0 for a
    configuration outside the limits"""
    lib = _lib.get()
    room = 1 << 20
    par, grd, x, dy = (torch.ones(room, device=device) for _ in range(4))
    saved, ws = (torch.zeros(4 * room, device=device) for _ in range(2))
    fields = [f for f, _ in _lib.MitBlockPtrs._fields_]
    sr_fields = ('sr_w', 'sr_b', 'srn_g', 'srn_b')

    def call(cfg_kw=None, drop=(), give_sr=False, alias=None, run=('fwd', 'bwd')):
        """-> (cfg, (rc, error) of the forward, of the backward); whatever is called must refuse and leave y / dx as they were"""
        kw = dict(B=1, H=8, W=8, C=32, heads=1, hidden=128, sr_ratio=2, depth=1, scale=32 ** -0.5, eps_embed=0., eps_block=1e-6, eps_sr=1e-6,
                  eps_out=0.)
        kw.update(cfg_kw or {})
        cfg = _lib.MitStageCfg(**kw)
        ps, gs = (_lib.MitBlockPtrs * 1)(), (_lib.MitBlockPtrs * 1)()
        for f in fields:
            have = f not in drop and (f not in sr_fields or kw['sr_ratio'] > 1 or give_sr)
            setattr(ps[0], f, par.data_ptr() if have else None)
            setattr(gs[0], f, grd.data_ptr() if have else None)
        y, dx = (torch.full((room,), NAN, device=device) for _ in range(2))
        out = []
        if 'fwd' in run:
            rc = lib.cffm_mit_blocks_train_fwd(C.byref(cfg), ps, None, _p(x), _p(x if alias == 'y' else y), _p(saved), _p(ws), _st(x))
            out.append((rc, lib.cffm_last_error()))
        if 'bwd' in run:
            rc = lib.cffm_mit_blocks_train_bwd(C.byref(cfg), ps, None, gs, _p(x), _p(saved), _p(dy), _p(dy if alias == 'dx' else dx), _p(ws),
                                               _st(x))
            out.append((rc, lib.cffm_last_error()))
        _sync(device)
        assert all(rc != 0 and err != b'' for rc, err in out), (cfg_kw, drop, alias, out)
        assert bool(y.isnan().all()) and bool(dx.isnan().all()) and bool((x == 1).all()) and bool((dy == 1).all()), (cfg_kw, drop, alias)
        return cfg

    for cfg_kw in (dict(heads=2), dict(C=24), dict(sr_ratio=3), dict(H=1), dict(W=1), dict(hidden=130), dict(depth=0)):
        cfg = call(cfg_kw)
        assert all(getattr(lib, n)(C.byref(cfg)) < 0 for n in SIZES), cfg_kw
    for kw in (dict(drop=('proj_b',)), dict(drop=('n1_g',)), dict(drop=('sr_w',)), dict(cfg_kw=dict(sr_ratio=1), give_sr=True)):
        cfg = call(**kw)
        assert all(getattr(lib, n)(C.byref(cfg)) >= 0 for n in SIZES), kw       # (the configuration itself is inside the limits)
    call(alias='y', run=('fwd',))
    cfg = call(alias='dx', run=('bwd',))
    assert all(lib.cffm_mit_blocks_train_saved_floats(None) < 0 for _ in range(1))
    # a gradient pointer must be there exactly where the parameter is
    ps, gs = (_lib.MitBlockPtrs * 1)(), (_lib.MitBlockPtrs * 1)()
    for fl in fields:
        setattr(ps[0], fl, par.data_ptr())
        setattr(gs[0], fl, None if fl == 'fc1_w' else grd.data_ptr())
    dx = torch.full((room,), NAN, device=device)
    assert lib.cffm_mit_blocks_train_bwd(C.byref(cfg), ps, None, gs, _p(x), _p(saved), _p(dy), _p(dx), _p(ws), _st(x)) != 0
    _sync(device)
    assert bool(dx.isnan().all())
    # the Python entry
    blocks, xs, _, _ = stage_on(device, 'a')
    for bad in (lambda: V.mit_blocks_train(xs, blocks, 8, 7), lambda: V.mit_blocks_train(xs, [], 8, 8),
                lambda: V.mit_blocks_train(xs.double(), blocks, 8, 8), lambda: V.mit_blocks_train(xs, blocks, 8, 8, torch.ones(2, 2, 3, device=device)),
                lambda: V.mit_blocks_train(xs[:, :, :24].contiguous(), blocks, 8, 8)):
        with pytest.raises(_lib.CffmError):
            bad()


# ---------------------------------------------------------------------------------------------- C. the backbone switch
SPIED = (FWD, BWD, 'cffm_linear_rows_fwd', 'cffm_linear_rows_bwd', 'cffm_ln_rows', 'cffm_ln_rows_bwd', 'cffm_sra_attn_fwd', 'cffm_sra_attn_bwd')


def all_hip(m, block_impl):
    m.set_norm_impl('hip')
    m.set_conv_impl('hip')
    m.set_linear_impl('hip')
    for mod in m.modules():
        if hasattr(type(mod), 'sr_impl'):
            mod.sr_impl = 'hip'
    m.set_block_impl(block_impl)
    return m


STOCK_CONV = ('patch_embed1.proj.weight', 'patch_embed1.proj.bias')


def model_pass(device, block_impl, img_grad=True):
    """tests.test_backbone.train_pass (its image, its loss) with every switch on 'hip'.  img_grad: whether the image requires grad -- it
    then gets a gradient, and the 7 x 7 embedding, which has no input gradient in the library, is stock Conv2d in both directions"""
    m = all_hip(TB.make(device, 'mit_b0'), block_impl)
    m.reset_drop_path(0.1)
    m.train()
    img = TB.R.synth_input('img', (2, 3, 64, 64), seed=41, scale=1.0).to(device).requires_grad_(img_grad)
    with TL.fixed_rand(TL.DROP_SEED) as drawn, CallSpy(_lib.get(), SPIED) as spy:
        outs = m(img)
        sum((o * TB.R.synth_input('w%d' % i, o.shape, seed=42, scale=1.0).to(device)).sum() for i, o in enumerate(outs)).backward()
    return [o.detach() for o in outs], img.grad, {k: p.grad for k, p in m.named_parameters()}, [d.clone() for d in drawn], spy.calls


def run_backbone(device):
    """block_impl = 'hip' against 'torch': the four outputs, the input gradient and all parameter gradients bit-equal, the same samples
    dropped, one call per stage and direction.  On the GPU the stock Conv2d weight gradient of patch_embed1 (what an image that requires
    grad leaves that embedding with) is summed with atomics and is not the same from one run to the next, whatever block_impl is: there
    the parameters of patch_embed1.proj are compared in a second pass whose image does not require grad, where conv_impl = 'hip' takes
    that embedding too, and everything else in both."""
    assert B.MixVisionTransformer.block_impl == 'torch'
    for img_grad in ((True, False) if device.type == 'cuda' else (True,)):
        outs_t, dimg_t, grads_t, drawn_t, calls_t = model_pass(device, 'torch', img_grad)
        outs_h, dimg_h, grads_h, drawn_h, calls_h = model_pass(device, 'hip', img_grad)
        nblocks = 8
        assert calls_t[FWD] == 0 and calls_t[BWD] == 0 and calls_t['cffm_linear_rows_fwd'] == 5 * nblocks and calls_t['cffm_ln_rows'] == 2 * nblocks
        assert calls_h == {n: (4 if n in (FWD, BWD) else 0) for n in SPIED}, calls_h
        assert len(drawn_h) == len(drawn_t) == 14 and all(torch.equal(a, b) for a, b in zip(drawn_h, drawn_t))
        assert any(float(v) + 0.9 < 1 for d in drawn_h for v in d)               # (a sample is dropped somewhere)
        for a, b in zip(outs_h, outs_t):
            assert torch.equal(a, b)
        assert (dimg_h is None and dimg_t is None) if not img_grad else torch.equal(dimg_h, dimg_t)
        assert set(grads_h) == set(grads_t)
        for k in grads_t:
            if img_grad and device.type == 'cuda' and k in STOCK_CONV:
                continue
            assert grads_h[k] is not None and torch.equal(grads_h[k], grads_t[k]), (k, img_grad)


def run_backbone_dispatch(device):
    """under no_grad and with an fp64 model the switch changes nothing; a stage outside the limits takes today's path, the others the call"""
    lib = _lib.get()
    img = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).to(device)
    m = all_hip(TB.make(device, 'mit_b0'), 'torch').train()
    with pytest.raises(ValueError):
        m.set_block_impl('x')
    calls = {}
    for impl in ('torch', 'hip'):
        m.set_block_impl(impl)
        with CallSpy(lib, SPIED) as spy, torch.no_grad():
            m(img)
        calls[impl] = spy.calls
    assert calls['hip'] == calls['torch'] and calls['hip'][FWD] == 0 and calls['hip']['cffm_linear_rows_fwd'] == 40
    for p in m.parameters():                                                 # grad mode on, nothing to differentiate: today's path
        p.requires_grad_(False)
    with CallSpy(lib, SPIED) as spy:
        m(img)
    assert spy.calls[FWD] == 0 and spy.calls['cffm_linear_rows_fwd'] == 40
    kw = dict(img_size=32, patch_size=4, num_heads=[1, 1, 1, 1], mlp_ratios=[1, 1, 1, 1], depths=[1, 1, 1, 1], sr_ratios=[2, 1, 1, 1], qkv_bias=True)
    small = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(device)
    md = all_hip(B.MixVisionTransformer(embed_dims=[32, 32, 32, 32], **kw).to(device), 'hip').train()
    with CallSpy(lib, SPIED) as spy:
        sum(o.sum() for o in md.double()(small.double())).backward()
    assert all(v == 0 for v in spy.calls.values()), spy.calls
    torch.manual_seed(0)
    mo = all_hip(B.MixVisionTransformer(embed_dims=[32, 48, 64, 64], **kw).to(device), 'hip').train()      # stage 2: head size 48
    with CallSpy(lib, SPIED) as spy:
        outs = mo(small)
        sum(o.sum() for o in outs).backward()
    assert spy.calls[FWD] == 3 and spy.calls[BWD] == 3 and spy.calls['cffm_linear_rows_fwd'] == 5 and spy.calls['cffm_ln_rows'] == 2, spy.calls
    grads = {k: p.grad.clone() for k, p in mo.named_parameters()}
    mo.zero_grad(set_to_none=True)
    mo.set_block_impl('torch')
    outs_t = mo(small)
    sum(o.sum() for o in outs_t).backward()
    assert all(torch.equal(a, b) for a, b in zip(outs, outs_t))
    assert all(torch.equal(grads[k], p.grad) for k, p in mo.named_parameters())
    mdp = all_hip(B.MixVisionTransformer(embed_dims=[32, 32, 32, 32], drop_rate=0.1, **kw).to(device), 'hip').train()    # dropout: not plain
    with CallSpy(lib, SPIED) as spy:
        mdp(small)
    assert spy.calls[FWD] == 0


# ---------------------------------------------------------------------------------------------- emulator
def test_symbols_and_exports():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cffm_hip.h')).read()
    lib = emu.lib()
    for n in (ADD, FWD, BWD) + SIZES:
        assert n + '(' in text and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert 'cffm_mit_block_grad_ptrs' in text and 'cffm_mit_block_scales' in text
    assert lib.cffm_abi_version() == 13
    assert callable(V.mit_blocks_train) and callable(V.mit_blocks_train_supported) and callable(B.MixVisionTransformer.set_block_impl)


@pytest.mark.parametrize('shape', LN_ROWS, ids=LN_IDS)
def test_ln_rows_bwd_add(shape):
    with emu.active():
        run_ln_add(CPU, shape)


def test_ln_rows_bwd_add_errors():
    with emu.active():
        run_ln_add_errors(CPU)


@pytest.mark.parametrize('name', list(CASES))
def test_stage_against_the_composition(name):
    with emu.active():
        run_stage_case(CPU, name)


def test_stage_poisoned_buffers():
    with emu.active():
        run_stage_poison(CPU)


def test_stage_dropped_sample():
    with emu.active():
        run_stage_dropped(CPU)


def test_stage_needs_input_grad():
    with emu.active():
        run_stage_needs_grad(CPU)


def test_stage_against_fp64():
    with emu.active():
        run_stage_anchor(CPU)


def test_stage_errors():
    with emu.active():
        run_stage_errors(CPU)


def test_backbone_block_impl():
    with emu.active():
        run_backbone(CPU)


def test_backbone_dispatch():
    with emu.active():
        run_backbone_dispatch(CPU)


def test_no_cpu_fallback():
    """a CPU tensor without the emulator raises, GPU present or not"""
    blocks = make_blocks('a')
    with pytest.raises(_lib.CffmError):
        V.mit_blocks_train(torch.zeros(2, 64, 32), blocks, 8, 8)
