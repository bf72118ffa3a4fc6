"""MiT's overlapping patch embedding for a training pass (include/cffm_hip.h: cffm_patch_embed_fwd_train / cffm_patch_embed_bwd,
vss_cffm_amd.overlap_patch_embed) and the backbone's ``conv_impl`` switch, on the CPU through the fiber emulator.  The GPU half is
tests/test_patch_embed_train_gpu.py and shares the run_*(device) bodies below.

Reference: the stock sequence norm(proj(x).flatten(2).transpose(1, 2)) with autograd, in fp64 on the CPU.  Yardstick: the same in fp64 with
the convolution replaced by SplitConv below -- forward conv(x_hi, w_hi) + conv(x_hi, w_lo) + conv(x_lo, w_hi) + bias of bf16-split operands,
backward the same three terms of torch.nn.grad.conv2d_weight(x, ., dz) and conv2d_input(., w, dz).  Inputs: R.synth_input / R.synth_state as
tests/test_patch_embed.py (gamma perturbed as its make_embed), dout = randn of torch.Generator().manual_seed(0).

Rule, for each t of out, dx, dw, db, dgamma, dbeta:  max|t - t64| <= 4 dist(yard_t, t64) + 2^-23 A_t.  A_out = max|out64|; for a gradient A_t is
the largest element of the same fp64 backward evaluated with magnitudes, every minus a plus (the Yard construction of tests/test_ln_train.py):
|dz| = rstd (g + mean(g) + |xhat| mean(g |xhat|)) with g = |gamma dout|, then conv2d_weight(|x|, |dz|), conv2d_input(|w|, |dz|), sum |dz|,
sum |dout| |xhat|, sum |dout|.  (3, 2) cases run with dx, (7, 4) cases without.

Measured, error / gate (every run prints error, gate and ratio per tensor: pytest -s; the same figures are in DESIGN.md section 3w):
    through the emulator (CPU)  out    dx     dw     db     dgamma dbeta
    k7_1x3x32x32_32             0.25   -      0.23   0.23   0.24   0.28
    k7_2x3x68x76_64             0.25   -      0.22   0.14   0.24   0.08
    k7_1x3x30x27_32             0.25   -      0.25   0.22   0.24   0.27
    k3_2x64x18x22_128           0.26   0.23   0.24   0.17   0.26   0.22
    k3_2x64x12x9_160            0.25   0.23   0.25   0.21   0.25   0.21
    k3_2x128x10x14_320          0.24   0.23   0.24   0.18   0.26   0.25
    k3_2x320x5x6_512            0.25   0.23   0.25   0.20   0.24   0.36
    k3_1x32x1x1_64              0.25   0.24   0.25   0.25   0.25   0.00
    k3_1x256x7x7_16             0.25   0.26   0.23   0.23   0.25   0.42
    k3_2x64x12x9_160+30         0.26   0.23   0.25   0.22   0.23   0.21
    k7_1x3x260x260_16           0.25   -      0.21   0.10   0.21   0.06
    on the MI355X               out    dx     dw     db     dgamma dbeta
    k7_1x3x32x32_32             0.25   -      0.20   0.23   0.25   0.28
    k7_2x3x68x76_64             0.25   -      0.23   0.14   0.24   0.08
    k7_1x3x30x27_32             0.25   -      0.25   0.22   0.24   0.27
    k3_2x64x18x22_128           0.25   0.23   0.24   0.15   0.24   0.22
    k3_2x64x12x9_160            0.25   0.23   0.25   0.21   0.25   0.21
    k3_2x128x10x14_320          0.25   0.23   0.24   0.16   0.25   0.25
    k3_2x320x5x6_512            0.25   0.22   0.25   0.20   0.26   0.36
    k3_1x32x1x1_64              0.25   0.24   0.25   0.25   0.25   0.00
    k3_1x256x7x7_16             0.25   0.25   0.25   0.24   0.24   0.42
    k3_2x64x12x9_160+30         0.26   0.21   0.25   0.20   0.25   0.21
    k7_1x3x260x260_16           0.25   -      0.21   0.11   0.22   0.06
The largest ratio: 0.42 on both (dbeta of k3_1x256x7x7_16: an fp32 sum of 16 terms against one rounding unit of their magnitudes).
z against proj's fp64 output, of the forward's gate: 0.25, 0.25 through the emulator; 0.25, 0.23 on the MI355X.
Backbone (mit_b0, [2,3,64,64], train mode, conv_impl 'hip'), out0-3 | patch_embed1.proj.weight | patch_embed3.proj.weight |
patch_embed2.norm.weight | block1.0.mlp.fc2.weight:
    through the emulator  0.24 0.21 0.25 0.21 | 0.22 | 0.24 | 0.26 | 0.24
    on the MI355X         0.23 0.22 0.23 0.20 | 0.21 | 0.21 | 0.23 | 0.22
"""
import ctypes as C
import functools
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import vss_cffm_amd as V
from oracle import recipe as R
from tests import emu
from tests import test_backbone as TB
from tests import test_mit_stage as TS
from tests.test_ln_train import no_override
from tests.test_mit_stage import dist
from tests.test_mixffn import CallSpy
from tests.test_patch_embed import KERNEL_CASES
from vss_cffm_amd import _lib
from vss_cffm_amd import backbone as B

CPU = torch.device('cpu')
MARGIN = 4.0
ULP = 2.0 ** -23
SLAB_CAP, DW_ROWS = 128, 32      # PEMB_DW_SLAB_CAP, PEMB_DW_ROWS of csrc/pembed_kernels.h
# the cases of the forward's test and one more: 65 x 65 = 4225 output pixels, just past SLAB_CAP x DW_ROWS = 4096 and no multiple of it or
# of the slab (34 rows, 125 slabs, the last one 9 rows); Cout = 16 and K = 147 make 3 workgroups per slab, so the split runs into its cap
CASES = dict(KERNEL_CASES, k7_1x3x260x260_16=((7, 4), (1, 3, 260, 260), 16, 0.0))
NAMES = ('out', 'dx', 'dw', 'db', 'dgamma', 'dbeta')
FWD, FWD_TRAIN, BWD, BWD_WS = 'cffm_patch_embed_fwd', 'cffm_patch_embed_fwd_train', 'cffm_patch_embed_bwd', 'cffm_patch_embed_bwd_workspace_bytes'
TAIL = 64        # floats behind every output that must stay as they were


# ---------------------------------------------------------------------------------------------- inputs and the yardstick
def make_embed(name, dtype=torch.float32):
    """tests.test_patch_embed.make_embed over CASES"""
    (k, s), shape, cout, shift = CASES[name]
    m = B.OverlapPatchEmbed(img_size=64, patch_size=k, stride=s, in_chans=shape[1], embed_dim=cout)
    m.load_state_dict(R.synth_state(m, seed=60), strict=True)
    with torch.no_grad():
        m.proj.bias += shift
        m.norm.weight.mul_(4.0).add_(1.0)          # gamma = 1 + 0.2 N(0, 1)
    return m.to(dtype).eval()


def out_hw(name):
    (k, s), (_, _, h, w), _, _ = CASES[name]
    return tuple((v + 2 * (k // 2) - k) // s + 1 for v in (h, w))


@functools.lru_cache(maxsize=None)
def inputs(name):
    (k, s), shape, cout, _ = CASES[name]
    ho, wo = out_hw(name)
    x = R.synth_input('pembed_x', shape, seed=61, scale=1.0)
    dout = torch.randn((shape[0], ho * wo, cout), generator=torch.Generator().manual_seed(0))
    return x, dout


class SplitConv(torch.autograd.Function):
    """the yardstick's convolution: three products of bf16-split operands, forward and backward"""

    @staticmethod
    def forward(ctx, x, w, b, stride, padding):
        ctx.save_for_backward(x, w)
        ctx.kw = dict(stride=stride, padding=padding)
        (xh, xl), (wh, wl) = TS._split(x), TS._split(w)
        return F.conv2d(xh, wh, **ctx.kw) + F.conv2d(xh, wl, **ctx.kw) + F.conv2d(xl, wh, **ctx.kw) + b.view(1, -1, 1, 1)

    @staticmethod
    def backward(ctx, dz):
        x, w = ctx.saved_tensors
        (xh, xl), (wh, wl), (dh, dl) = TS._split(x), TS._split(w), TS._split(dz)
        cw, ci = torch.nn.grad.conv2d_weight, torch.nn.grad.conv2d_input
        dw = cw(xh, w.shape, dh, **ctx.kw) + cw(xh, w.shape, dl, **ctx.kw) + cw(xl, w.shape, dh, **ctx.kw)
        dx = ci(x.shape, wh, dh, **ctx.kw) + ci(x.shape, wh, dl, **ctx.kw) + ci(x.shape, wl, dh, **ctx.kw) if ctx.needs_input_grad[0] else None
        return dx, dw, dz.sum((0, 2, 3)), None, None


def split_forward(conv):
    return lambda x: SplitConv.apply(x, conv.weight, conv.bias, conv.stride, conv.padding)


def sequence_grads(m, x, dout, with_dx):
    """the module's own forward and autograd in the module's dtype -> the six tensors (dx None without with_dx)"""
    m.zero_grad()
    for p in m.parameters():
        p.requires_grad_(True)
    xg = x.detach().clone().requires_grad_(with_dx)
    out = m(xg)[0]
    out.backward(dout)
    return {'out': out.detach(), 'dx': xg.grad, 'dw': m.proj.weight.grad.clone(), 'db': m.proj.bias.grad.clone(),
            'dgamma': m.norm.weight.grad.clone(), 'dbeta': m.norm.bias.grad.clone()}


class Yard:
    """fp64 reference of one case (optionally of some of its images alone), the yardstick's distance to it and the magnitudes A_t; computed
    once and left unchanged"""

    def __init__(self, name, images=None):
        (k, s), shape, cout, _ = CASES[name]
        x, dout = inputs(name)
        if images is not None:
            x, dout = x[slice(*images)], dout[slice(*images)]
        self.with_dx = k == 3
        x64, d64 = x.double(), dout.double()
        m = make_embed(name, torch.float64)
        self.want = sequence_grads(m, x64, d64, self.with_dx)
        with torch.no_grad():
            self.z = m.proj(x64)
        m.proj.forward = split_forward(m.proj)
        yard = sequence_grads(m, x64, d64, self.with_dx)
        with torch.no_grad():
            self.z_gate = MARGIN * dist(m.proj(x64), self.z) + ULP * float(self.z.abs().max())
        del m.proj.forward
        # the same backward with magnitudes
        with torch.no_grad():
            zr, dr = self.z.flatten(2).transpose(1, 2).reshape(-1, cout), d64.reshape(-1, cout)
            d = zr - zr.mean(1, keepdim=True)
            rstd = 1 / torch.sqrt((d * d).mean(1, keepdim=True) + m.norm.eps)
            xh, g = (d * rstd).abs(), (m.norm.weight * dr).abs()
            dz = rstd * (g + g.mean(1, keepdim=True) + xh * (g * xh).mean(1, keepdim=True))
            dzm = dz.reshape(x.shape[0], -1, cout).transpose(1, 2).reshape(self.z.shape)
            kw = dict(stride=m.proj.stride, padding=m.proj.padding)
            mag = {'out': float(self.want['out'].abs().max()), 'db': float(dz.sum(0).max()), 'dgamma': float((dr.abs() * xh).sum(0).max()),
                   'dbeta': float(dr.abs().sum(0).max()),
                   'dw': float(torch.nn.grad.conv2d_weight(x64.abs(), m.proj.weight.shape, dzm, **kw).max())}
            if self.with_dx:
                mag['dx'] = float(torch.nn.grad.conv2d_input(x64.shape, m.proj.weight.abs(), dzm, **kw).max())
        self.mag = mag
        self.noise = {n: dist(yard[n], self.want[n]) for n in mag}

    def gate(self, n):
        return MARGIN * self.noise[n] + ULP * self.mag[n]


@functools.lru_cache(maxsize=None)
def yard(name, images=None):
    return Yard(name, images)


def check(tag, y, got):
    """print error / gate of every tensor, then assert; -> the ratios"""
    lines = []
    for n in NAMES:
        if got.get(n) is None:
            continue
        assert tuple(got[n].shape) == tuple(y.want[n].shape), (tag, n, tuple(got[n].shape))
        err = dist(got[n], y.want[n])
        lines.append((n, err, y.gate(n)))
        print('%s %s: max err %.3e / gate %.3e = %.2f (4 x %.3e + 2^-23 x %.3e)' % (tag, n, err, y.gate(n), err / y.gate(n), y.noise[n], y.mag[n]))
    for n, err, gate in lines:
        assert err <= gate, (tag, n, err, gate)
    return {n: err / gate for n, err, gate in lines}


# ---------------------------------------------------------------------------------------------- the C ABI, called directly
def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else C.c_void_p(0)


def _st(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def _sync(device):
    if device.type == 'cuda':
        torch.cuda.synchronize()


def dims_of(name, batch=None):
    (k, s), (b, cin, h, w), cout, _ = CASES[name]
    return [batch or b, cin, h, w, cout, k, s]


def nan(n, device):
    return torch.full((n + TAIL,), float('nan'), device=device)


def split_tail(t, shape, what):
    n = 1
    for v in shape:
        n *= v
    assert bool(t[n:].isnan().all()), '%s: written past the end' % what
    assert not bool(t[:n].isnan().any()), '%s: not every element written' % what
    return t[:n].reshape(shape)


def raw_fwd(lib, device, name, m, x):
    """cffm_patch_embed_fwd_train on NaN-filled outputs -> out, z"""
    dims = dims_of(name, x.shape[0])
    ho, wo = out_hw(name)
    shape = (x.shape[0], ho * wo, dims[4])
    out, z = nan(shape[0] * shape[1] * shape[2], device), nan(shape[0] * shape[1] * shape[2], device)
    rc = lib.cffm_patch_embed_fwd_train(_p(x), _p(m.proj.weight), _p(m.proj.bias), _p(m.norm.weight), _p(m.norm.bias), _p(out), _p(z), *dims,
                                        m.norm.eps, _st(x))
    assert rc == 0, lib.cffm_last_error()
    _sync(device)
    return split_tail(out, shape, 'out'), split_tail(z, shape, 'z')


def raw_bwd(lib, name, m, x, z, dout, with_dx, ws_fill=float('nan'), null=(), off=None, dims=None, eps=None):
    """cffm_patch_embed_bwd -> (rc, the NaN-prefilled dx, dw, db, dgamma, dbeta with TAIL floats behind each)"""
    dev = x.device
    dims = dims or dims_of(name, x.shape[0])
    cout = m.proj.out_channels
    outs = {'dx': nan(x.numel(), dev), 'dw': nan(m.proj.weight.numel(), dev), 'db': nan(cout, dev), 'dgamma': nan(cout, dev), 'dbeta': nan(cout, dev)}
    nbytes = lib.cffm_patch_embed_bwd_workspace_bytes(*dims_of(name, x.shape[0]), int(with_dx))
    assert nbytes > 0, lib.cffm_last_error()
    ws = torch.full((nbytes // 4 + TAIL,), ws_fill, device=dev)
    ptrs = {'x': x, 'w': m.proj.weight, 'gamma': m.norm.weight, 'z': z, 'dout': dout, 'dx': outs['dx'] if with_dx else None, 'dw': outs['dw'],
            'db': outs['db'], 'dgamma': outs['dgamma'], 'dbeta': outs['dbeta'], 'ws': ws}
    args = [_p(None if n in null else t, off[1] if off and off[0] == n else 0) for n, t in ptrs.items()]
    rc = lib.cffm_patch_embed_bwd(*args, *dims, m.norm.eps if eps is None else eps, _st(x))
    return rc, outs


def run_raw(lib, device, name, m, x, z, dout, with_dx, ws_fill=float('nan')):
    rc, outs = raw_bwd(lib, name, m, x, z, dout, with_dx, ws_fill)
    assert rc == 0, lib.cffm_last_error()
    _sync(device)
    cout = m.proj.out_channels
    shapes = {'dx': tuple(x.shape), 'dw': tuple(m.proj.weight.shape), 'db': (cout,), 'dgamma': (cout,), 'dbeta': (cout,)}
    got = {n: split_tail(t, shapes[n], n) for n, t in outs.items() if n != 'dx' or with_dx}
    if not with_dx:
        assert bool(outs['dx'].isnan().all())
    return got


def on(device, name):
    """the module with trainable parameters and the inputs on `device`"""
    m = make_embed(name).to(device)
    return (m,) + tuple(t.to(device) for t in inputs(name))


def autograd_grads(m, x, dout, with_dx):
    m.zero_grad()
    xg = x.detach().clone().requires_grad_(with_dx)
    out, ho, wo = V.overlap_patch_embed(xg, m.proj, m.norm)
    out.backward(dout)
    return {'out': out.detach(), 'dx': xg.grad, 'dw': m.proj.weight.grad.clone(), 'db': m.proj.bias.grad.clone(),
            'dgamma': m.norm.weight.grad.clone(), 'dbeta': m.norm.bias.grad.clone()}, (ho, wo)


class ArgSpy:
    """records the arguments of every call of one entry point made through the binding"""

    def __init__(self, lib, name):
        self.lib, self.name, self.real, self.args = lib, name, getattr(lib, name), []

    def __enter__(self):
        setattr(self.lib, self.name, lambda *a: (self.args.append(a), self.real(*a))[1])
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.real)


# ---------------------------------------------------------------------------------------------- bodies shared with the GPU half
def run_case(device, name):
    """autograd and the raw C ABI against the gate; the same bits from both; the sentinels behind every output stay"""
    lib = _lib.get()
    y = yard(name)
    m, x, dout = on(device, name)
    with ArgSpy(lib, BWD) as spy:
        auto, hw = autograd_grads(m, x, dout, y.with_dx)
    assert hw == out_hw(name) and len(spy.args) == 1 and (spy.args[0][5].value is not None) == y.with_dx
    ratios = check('%s (autograd)' % name, y, auto)
    out, z = raw_fwd(lib, device, name, m, x)
    assert torch.equal(out, auto['out'])
    raw = run_raw(lib, device, name, m, x, z, dout, y.with_dx)
    for n, t in raw.items():
        assert torch.equal(t, auto[n]), n
    return ratios


def run_without_dx(device, name='k3_2x64x12x9_160'):
    """x does not require grad: the dx argument is NULL and the other four gradients have the bits of the run with dx"""
    lib = _lib.get()
    m, x, dout = on(device, name)
    want, _ = autograd_grads(m, x, dout, True)
    with ArgSpy(lib, BWD) as spy:
        got, _ = autograd_grads(m, x, dout, False)
    assert len(spy.args) == 1 and spy.args[0][5].value is None and got['dx'] is None and want['dx'] is not None
    for n in ('out', 'dw', 'db', 'dgamma', 'dbeta'):
        assert torch.equal(got[n], want[n]), n


def run_forward(device, name):
    """out of the training forward IS the inference call's; z is proj's output within the forward's gate; no_grad: the inference call"""
    lib = _lib.get()
    y = yard(name)
    m, x, _ = on(device, name)
    with torch.no_grad():
        want = V.patch_embed(x, m.proj, m.norm)[0]
    out, z = raw_fwd(lib, device, name, m, x)
    assert torch.equal(out, want)
    zmap = z.reshape(x.shape[0], *out_hw(name), -1).permute(0, 3, 1, 2)
    err = dist(zmap, y.z)
    print('%s z: max err %.3e / gate %.3e = %.2f' % (name, err, y.z_gate, err / y.z_gate))
    assert err <= y.z_gate
    res = V.overlap_patch_embed(x, m.proj, m.norm)[0]
    assert res.grad_fn is not None and torch.equal(res.detach(), want)
    with pytest.raises(_lib.CffmError):           # the inference function keeps its contract
        V.patch_embed(x, m.proj, m.norm)
    with CallSpy(lib, (FWD, FWD_TRAIN, BWD, BWD_WS)) as spy:
        with torch.no_grad():
            a = V.overlap_patch_embed(x.clone().requires_grad_(True), m.proj, m.norm)[0]
        for p in m.parameters():
            p.requires_grad_(False)
        b = V.overlap_patch_embed(x, m.proj, m.norm)[0]
    assert spy.calls == {FWD: 2, FWD_TRAIN: 0, BWD: 0, BWD_WS: 0}, spy.calls
    assert a.grad_fn is None and b.grad_fn is None and torch.equal(a, want) and torch.equal(b, want)


def run_poison_and_determinism(device, name):
    """a NaN-filled and a zero-filled workspace, NaN-filled outputs before each call: finite results, the same bits"""
    lib = _lib.get()
    m, x, dout = on(device, name)
    with_dx = CASES[name][0][0] == 3
    _, z = raw_fwd(lib, device, name, m, x)
    runs = [run_raw(lib, device, name, m, x, z, dout, with_dx, fill) for fill in (float('nan'), 0.0)]
    assert len(runs[0]) == (5 if with_dx else 4)
    for n, t in runs[0].items():
        assert bool(t.isfinite().all()) and torch.equal(t, runs[1][n]), n


def run_no_leak(device, name='k3_2x64x12x9_160'):
    """dout non-zero in image 1 only: dx of image 0 is exactly zero, and dw is the B = 1 result on image 1 alone within the gate"""
    lib = _lib.get()
    m, x, dout = on(device, name)
    dout = dout.clone()
    dout[0] = 0.0
    _, z = raw_fwd(lib, device, name, m, x)
    both = run_raw(lib, device, name, m, x, z, dout, True)
    assert not bool(both['dx'][0].any()) and bool(both['dx'][1].any())
    x1, d1 = x[1:].contiguous(), dout[1:].contiguous()
    _, z1 = raw_fwd(lib, device, name, m, x1)
    assert torch.equal(z1[0], z[1])
    alone = run_raw(lib, device, name, m, x1, z1, d1, True)
    y = yard(name, images=(1, 2))
    for tag, got in (('both images', both), ('image 1 alone', alone)):
        err = dist(got['dw'], y.want['dw'])
        print('%s dw, %s: max err %.3e / gate %.3e = %.2f' % (name, tag, err, y.gate('dw'), err / y.gate('dw')))
        assert err <= y.gate('dw')
    assert torch.equal(both['dx'][1], alone['dx'][0])


def run_refusals(device):
    """every refusal: non-zero, cffm_last_error set, nothing enqueued -- the NaN-prefilled outputs still NaN; the workspace query < 0"""
    lib = _lib.get()
    name = 'k3_2x64x12x9_160'
    m, x, dout = on(device, name)
    _, z = raw_fwd(lib, device, name, m, x)
    good = dims_of(name)

    def dims(**kw):
        d = list(good)
        for k, v in kw.items():
            d[dict(B=0, Cin=1, H=2, W=3, Cout=4, k=5, stride=6)[k]] = v
        return d
    sizes = dict(cout24=dims(Cout=24), cout528=dims(Cout=528), k5s2=dims(k=5, stride=2), cin6=dims(Cin=6), b0=dims(B=0), h0=dims(H=0),
                 k7cin64=dims(k=7, stride=4), k3s4=dims(stride=4), cin516=dims(Cin=516))
    cases = [dict(dims=d) for d in sizes.values()] + [dict(eps=-1.0), dict(eps=float('nan')), dict(eps=float('inf'))]
    cases += [dict(null=(n,)) for n in ('x', 'w', 'gamma', 'z', 'dout', 'dw', 'db', 'dgamma', 'dbeta', 'ws')]
    cases += [dict(off=(n, 4)) for n in ('x', 'w', 'gamma', 'z', 'dout', 'dx', 'dw', 'db', 'dgamma', 'dbeta', 'ws')]
    for kw in cases:
        rc, outs = raw_bwd(lib, name, m, x, z, dout, True, **kw)
        assert rc != 0 and lib.cffm_last_error() != b'', kw
        _sync(device)
        assert all(bool(t.isnan().all()) for t in outs.values()), kw
    for tag, d in sizes.items():
        assert lib.cffm_patch_embed_bwd_workspace_bytes(*d, 1) < 0 and lib.cffm_patch_embed_bwd_workspace_bytes(*d, 0) < 0, tag
    # (7, 4) with dx
    n7 = 'k7_1x3x32x32_32'
    m7, x7, d7 = on(device, n7)
    _, z7 = raw_fwd(lib, device, n7, m7, x7)
    rc, outs = raw_bwd(lib, n7, m7, x7, z7, d7, False, dims=dims_of(n7))
    assert rc == 0
    _sync(device)
    assert bool(outs['dx'].isnan().all()) and not bool(outs['dw'][:-TAIL].isnan().any())
    assert lib.cffm_patch_embed_bwd_workspace_bytes(*dims_of(n7), 1) < 0 and lib.cffm_patch_embed_bwd_workspace_bytes(*dims_of(n7), 0) > 0
    ws = torch.empty(lib.cffm_patch_embed_bwd_workspace_bytes(*dims_of(n7), 0) // 4, device=device)
    outs = {n: nan(k, device) for n, k in (('dx', x7.numel()), ('dw', m7.proj.weight.numel()), ('db', 32), ('dgamma', 32), ('dbeta', 32))}
    rc = lib.cffm_patch_embed_bwd(_p(x7), _p(m7.proj.weight), _p(m7.norm.weight), _p(z7), _p(d7), *(_p(outs[n]) for n in outs), _p(ws),
                                  *dims_of(n7), m7.norm.eps, _st(x7))
    assert rc != 0 and b'(3, 2)' in lib.cffm_last_error()
    _sync(device)
    assert all(bool(t.isnan().all()) for t in outs.values())
    # the forward's refusals: the outputs stay NaN
    out, zz = nan(z.numel(), device), nan(z.numel(), device)
    p = [x, m.proj.weight, m.proj.bias, m.norm.weight, m.norm.bias, out, zz]
    for tag, a, d in [('null z', [_p(t) for t in p[:6]] + [_p(None)], good), ('odd z', [_p(t) for t in p[:6]] + [_p(zz, 4)], good),
                      ('null out', [_p(t) for t in p[:5]] + [_p(None), _p(zz)], good), ('alias', [_p(t) for t in p[:6]] + [_p(out)], good),
                      ('cout24', [_p(t) for t in p], dims(Cout=24)), ('k5', [_p(t) for t in p], dims(k=5))]:
        assert lib.cffm_patch_embed_fwd_train(*a, *d, 1e-5, _st(x)) != 0 and lib.cffm_last_error() != b'', tag
    _sync(device)
    assert bool(out.isnan().all()) and bool(zz.isnan().all())
    # the Python layer
    with pytest.raises(_lib.CffmError):
        V.overlap_patch_embed(x, nn.Conv2d(64, 160, 3, 2, 0).to(device), m.norm)          # padding != k // 2
    with pytest.raises(_lib.CffmError):
        V.overlap_patch_embed(x7.clone().requires_grad_(True), m7.proj, m7.norm)          # (7, 4): no input gradient
    with pytest.raises(_lib.CffmError):
        V.overlap_patch_embed(x.double(), m.proj, m.norm)


def run_non_contiguous(device, name='k3_2x64x12x9_160'):
    """x as an NHWC-permuted view and dout as a transposed view: the bits of the contiguous call"""
    m, x, dout = on(device, name)
    want, _ = autograd_grads(m, x, dout, True)
    xv = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    dv = dout.transpose(1, 2).contiguous().transpose(1, 2)
    assert not xv.is_contiguous() and not dv.is_contiguous() and torch.equal(xv, x) and torch.equal(dv, dout)
    got, _ = autograd_grads(m, xv, dv, True)
    for n in NAMES:
        assert torch.equal(got[n], want[n]), n


# ---- the backbone
COMPARED = ('patch_embed1.proj.weight', 'patch_embed3.proj.weight', 'patch_embed2.norm.weight', 'block1.0.mlp.fc2.weight')
SPIED = (FWD, FWD_TRAIN, BWD)


def train_pass(m, device, dtype=torch.float32, shape=(2, 3, 64, 64)):
    """tests.test_backbone.train_pass with an image that does not require grad (what a training step feeds)"""
    m.train()
    img = R.synth_input('img', shape, seed=41, scale=1.0, dtype=dtype).to(device)
    outs = m(img)
    sum((o * R.synth_input('w%d' % i, o.shape, seed=42, scale=1.0, dtype=dtype).to(device)).sum() for i, o in enumerate(outs)).backward()
    return outs, {k: p.grad for k, p in m.named_parameters()}


def picked(outs, grads):
    d = {'out%d' % i: o.detach() for i, o in enumerate(outs)}
    d.update({k: grads[k] for k in COMPARED})
    return {k: v.detach().cpu().double() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def backbone_yard():
    """-> (the fp64 'torch' model's results, the gate per tensor): 4 x (distance of the fp64 model with the yardstick convolutions +
    distance of the fp32 'torch' model) + 2^-23 max|fp64|, all on the CPU in stock PyTorch"""
    with no_override():
        want = picked(*train_pass(TB.make(CPU, 'mit_b0', torch.float64), CPU, torch.float64))
        m = TB.make(CPU, 'mit_b0', torch.float64)
        for i in range(1, 5):
            conv = getattr(m, 'patch_embed%d' % i).proj
            conv.forward = split_forward(conv)
        split = picked(*train_pass(m, CPU, torch.float64))
        f32 = picked(*train_pass(TB.make(CPU, 'mit_b0'), CPU))
    return want, {k: MARGIN * (dist(split[k], want[k]) + dist(f32[k], want[k])) + ULP * float(want[k].abs().max()) for k in want}


def stock_forward(self, x):
    """OverlapPatchEmbed.forward before the switch existed"""
    x = self.proj(x)
    H, W = x.shape[2:]
    if B._norm_fused(self.norm_impl, self.norm, x, x.shape[1]):
        return B.nchw_layer_norm_rows(x, self.norm.weight, self.norm.bias, self.norm.eps), H, W
    return self.norm(x.flatten(2).transpose(1, 2)), H, W


def run_backbone(device):
    lib = _lib.get()
    want, gates = backbone_yard()
    m = TB.make(device, 'mit_b0')
    assert m.conv_impl == 'torch' and B.OverlapPatchEmbed.conv_impl == 'torch' and B.MixVisionTransformer.conv_impl == 'torch'
    with CallSpy(lib, SPIED) as spy:
        outs_t, grads_t = train_pass(m, device)
    assert sum(spy.calls.values()) == 0
    if device.type == 'cpu':          # (two calls of the stock Conv2d need not return the same bits on the GPU)
        real = B.OverlapPatchEmbed.forward
        B.OverlapPatchEmbed.forward = stock_forward
        try:
            outs_s, grads_s = train_pass(TB.make(device, 'mit_b0'), device)
        finally:
            B.OverlapPatchEmbed.forward = real
        assert all(torch.equal(a, b) for a, b in zip(outs_t, outs_s)) and all(torch.equal(grads_t[k], grads_s[k]) for k in grads_t)
    with pytest.raises(ValueError):
        m.set_conv_impl('cuda')
    m.set_conv_impl('hip')
    assert all(getattr(m, 'patch_embed%d' % i).conv_impl == 'hip' for i in range(1, 5)) and m.conv_impl == 'hip'
    m.zero_grad()
    with CallSpy(lib, SPIED) as spy, ArgSpy(lib, BWD) as args:
        got = picked(*train_pass(m, device))
    assert spy.calls == {FWD: 0, FWD_TRAIN: 4, BWD: 4}, spy.calls
    # autograd runs the stages backwards: the last call is stage 1's, the image's gradient is not asked for
    assert [a[5].value is None for a in args.args] == [False, False, False, True]
    for k in want:
        err = dist(got[k], want[k])
        print('mit_b0 conv_impl=hip %s: err %.3e / gate %.3e = %.2f' % (k, err, gates[k], err / gates[k]))
    for k in want:
        assert dist(got[k], want[k]) <= gates[k], k
    with CallSpy(lib, SPIED) as spy, torch.no_grad():
        m(R.synth_input('img', (2, 3, 64, 64), seed=41, scale=1.0).to(device))
    assert spy.calls == {FWD: 4, FWD_TRAIN: 0, BWD: 0}, spy.calls
    m.set_conv_impl('torch')
    assert all(mod.conv_impl == 'torch' for mod in m.modules() if hasattr(type(mod), 'conv_impl'))


def run_backbone_outside_the_limits(device):
    """a padding = 0 patch_embed2.proj takes the stock line while the other three take the library; an image that requires grad keeps the
    7 x 7 embedding on the stock line"""
    lib = _lib.get()
    m = TB.make(device, 'mit_b0')
    old = m.patch_embed2.proj
    new = nn.Conv2d(old.in_channels, old.out_channels, 3, 2, 0).to(device)
    with torch.no_grad():
        new.weight.copy_(old.weight)
        new.bias.copy_(old.bias)
    m.patch_embed2.proj = new
    ref, _ = train_pass(m, device)
    ref = [o.detach() for o in ref]
    m.set_conv_impl('hip')
    m.zero_grad()
    with CallSpy(lib, SPIED) as spy:
        outs, grads = train_pass(m, device)
    assert spy.calls == {FWD: 0, FWD_TRAIN: 3, BWD: 3}, spy.calls
    assert grads['patch_embed2.proj.weight'] is not None and float(grads['patch_embed2.proj.weight'].abs().max()) > 0
    for o, r in zip(outs, ref):
        assert o.shape == r.shape and dist(o, r) <= 1e-4 * max(1., float(r.abs().max()))
    m = TB.make(device, 'mit_b0')
    m.set_conv_impl('hip')
    with CallSpy(lib, SPIED) as spy:
        _, dimg, _ = TB.train_pass(m, device)
    assert spy.calls == {FWD: 0, FWD_TRAIN: 3, BWD: 3} and dimg is not None and float(dimg.abs().max()) > 0, spy.calls


# ---------------------------------------------------------------------------------------------- emulator
def test_symbols_and_exports():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cffm_hip.h')).read()
    lib = emu.lib()
    for n in (FWD_TRAIN, BWD, BWD_WS):
        assert n + '(' in text and n in _lib.SIGNATURES and hasattr(lib, n)
    assert lib.cffm_abi_version() == 13 and callable(V.overlap_patch_embed) and callable(B.MixVisionTransformer.set_conv_impl)
    # the ragged case runs into the slab cap: slabs of ceil(4225 / 128) = 34 rows, the last of 125 holds 9
    (_, shape, cout, _), (ho, wo) = CASES['k7_1x3x260x260_16'], out_hw('k7_1x3x260x260_16')
    m = ho * wo
    assert m > SLAB_CAP * DW_ROWS and m % (SLAB_CAP * DW_ROWS) and m % 34 == 9 and -(-m // 34) == 125


@pytest.mark.parametrize('name', list(CASES))
def test_case_against_the_gate(name):
    with emu.active():
        run_case(CPU, name)


def test_without_dx_the_other_gradients_keep_their_bits():
    with emu.active():
        run_without_dx(CPU)


@pytest.mark.parametrize('name', ['k7_1x3x30x27_32', 'k3_2x64x12x9_160+30'])
def test_forward_is_the_inference_call(name):
    with emu.active():
        run_forward(CPU, name)


@pytest.mark.parametrize('name', ['k7_2x3x68x76_64', 'k3_2x64x12x9_160', 'k3_2x320x5x6_512'])
def test_poisoned_workspace_and_determinism(name):
    with emu.active():
        run_poison_and_determinism(CPU, name)


def test_nothing_leaks_across_images():
    with emu.active():
        run_no_leak(CPU)


def test_refusals_enqueue_nothing():
    with emu.active():
        run_refusals(CPU)


def test_non_contiguous_inputs():
    with emu.active():
        run_non_contiguous(CPU)


def test_backbone_conv_impl():
    with emu.active():
        run_backbone(CPU)


def test_backbone_convolutions_outside_the_limits():
    with emu.active():
        run_backbone_outside_the_limits(CPU)


def test_no_cpu_fallback():
    """a CPU tensor without the emulator raises, GPU present or not"""
    m = make_embed('k3_1x32x1x1_64')
    with pytest.raises(_lib.CffmError):
        V.overlap_patch_embed(torch.zeros(1, 32, 1, 1), m.proj, m.norm)
