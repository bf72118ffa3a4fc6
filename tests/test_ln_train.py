"""The backwards of the three LayerNorm calls (include/cffm_hip.h: cffm_ln_rows_bwd / cffm_nchw_ln_rows_bwd / cffm_ln_rows_nchw_bwd,
vss_cffm_amd.layer_norm_rows / nchw_layer_norm_rows / layer_norm_rows_nchw) and the backbone's ``norm_impl`` switch, on the CPU through the
fiber emulator.  The GPU half is tests/test_ln_train_gpu.py and shares the run_*(device) bodies below.

The yardstick is the stock op sequence in fp64 on the CPU: F.layer_norm, behind x.flatten(2).transpose(1, 2) for the NCHW -> rows form and
in front of reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous() for the rows -> NCHW form.  Inputs from torch.Generator().manual_seed(0),
in this order: x = 1.5 randn + 2, gamma = 1 + 0.3 randn, beta = 0.3 randn, dout = randn; eps = 1e-6.

Rule, for each t of dx, dgamma, dbeta:  max|t - t64| <= 4 noise_t + 2^-23 A_t.  noise_t = max|fp32 stock sequence on the CPU - fp64|,
computed inside the test; A_t = the largest element of the same fp64 backward evaluated with magnitudes (|gamma dy|, |xhat|, |dy|): one
rounding unit of the sum of magnitudes, which keeps the gate above zero where the stock fp32 result happens to be exact (dbeta at M = 1).
The forward is not gated here: it is the inference call, bit for bit (tests/test_mit_stage.py gates that one).

Measured, error / gate = ratio (noise_t is the stock fp32 result of the machine the test runs on, so a gate moves a little between machines):
    through the emulator (CPU)    dx                             dgamma                         dbeta
    rows (1,16)                1.686e-07 / 1.116e-06 = 0.15  1.989e-07 / 2.163e-06 = 0.09  0.000e+00 / 4.066e-07 = 0.00
    rows (70,16)               3.718e-07 / 2.874e-06 = 0.13  2.376e-06 / 1.297e-05 = 0.18  2.580e-06 / 1.293e-05 = 0.20
    rows (7,36)                2.864e-07 / 1.362e-06 = 0.21  4.410e-07 / 4.603e-06 = 0.10  4.917e-07 / 3.019e-06 = 0.16
    rows (33,160)              3.622e-07 / 2.007e-06 = 0.18  1.676e-06 / 1.360e-05 = 0.12  1.192e-06 / 1.019e-05 = 0.12
    rows (9,256)               2.524e-07 / 2.691e-06 = 0.09  9.566e-07 / 6.876e-06 = 0.14  6.557e-07 / 3.953e-06 = 0.17
    rows (5,260)               3.342e-07 / 1.383e-06 = 0.24  6.139e-07 / 5.526e-06 = 0.11  5.364e-07 / 3.104e-06 = 0.17
    rows (6,512)               3.329e-07 / 1.929e-06 = 0.17  7.559e-07 / 3.620e-06 = 0.21  5.364e-07 / 3.378e-06 = 0.16
    rows (16389,64)            7.546e-07 / 3.773e-06 = 0.20  3.673e-05 / 2.577e-03 = 0.01  3.633e-05 / 2.493e-03 = 0.01
    from_nchw (1,16,1,1)       1.686e-07 / 1.116e-06 = 0.15  1.989e-07 / 2.163e-06 = 0.09  0.000e+00 / 4.066e-07 = 0.00
    from_nchw (2,160,6,5)      3.806e-07 / 2.225e-06 = 0.17  2.744e-06 / 1.619e-05 = 0.17  1.505e-06 / 1.492e-05 = 0.10
    from_nchw (2,64,9,9)       3.884e-07 / 2.786e-06 = 0.14  5.001e-06 / 3.114e-05 = 0.16  3.742e-06 / 3.239e-05 = 0.12
    from_nchw (1,260,3,3)      3.724e-07 / 1.960e-06 = 0.19  1.201e-06 / 5.711e-06 = 0.21  5.066e-07 / 4.462e-06 = 0.11
    from_nchw (1,512,5,5)      3.819e-07 / 2.537e-06 = 0.15  1.386e-06 / 1.585e-05 = 0.09  1.268e-06 / 8.613e-06 = 0.15
    to_nchw (1,16,1,1)         1.686e-07 / 1.116e-06 = 0.15  1.989e-07 / 2.163e-06 = 0.09  0.000e+00 / 4.066e-07 = 0.00
    to_nchw (2,160,6,5)        5.881e-07 / 2.288e-06 = 0.26  2.070e-06 / 1.604e-05 = 0.13  1.635e-06 / 1.346e-05 = 0.12
    to_nchw (2,64,9,9)         4.769e-07 / 2.317e-06 = 0.21  3.167e-06 / 3.870e-05 = 0.08  3.700e-06 / 3.170e-05 = 0.12
    to_nchw (1,260,3,3)        3.585e-07 / 1.986e-06 = 0.18  9.469e-07 / 8.433e-06 = 0.11  8.345e-07 / 3.956e-06 = 0.21
    to_nchw (1,512,5,5)        5.085e-07 / 2.881e-06 = 0.18  2.365e-06 / 1.381e-05 = 0.17  1.222e-06 / 8.737e-06 = 0.14
    on the MI355X                 dx                             dgamma                         dbeta
    rows (1,16)                1.686e-07 / 1.116e-06 = 0.15  1.989e-07 / 2.163e-06 = 0.09  0.000e+00 / 4.066e-07 = 0.00
    rows (70,16)               3.718e-07 / 2.874e-06 = 0.13  2.376e-06 / 1.161e-05 = 0.20  2.580e-06 / 1.313e-05 = 0.20
    rows (7,36)                2.171e-07 / 1.362e-06 = 0.16  4.397e-07 / 4.603e-06 = 0.10  4.917e-07 / 3.019e-06 = 0.16
    rows (33,160)              4.216e-07 / 2.007e-06 = 0.21  1.492e-06 / 1.112e-05 = 0.13  1.192e-06 / 1.129e-05 = 0.11
    rows (9,256)               3.657e-07 / 2.691e-06 = 0.14  9.161e-07 / 6.725e-06 = 0.14  6.557e-07 / 4.728e-06 = 0.14
    rows (5,260)               2.304e-07 / 1.383e-06 = 0.17  5.187e-07 / 5.526e-06 = 0.09  5.364e-07 / 3.104e-06 = 0.17
    rows (6,512)               2.817e-07 / 1.929e-06 = 0.15  7.559e-07 / 3.620e-06 = 0.21  5.364e-07 / 3.378e-06 = 0.16
    rows (16389,64)            1.051e-06 / 3.773e-06 = 0.28  4.642e-05 / 2.016e-03 = 0.02  3.633e-05 / 2.294e-03 = 0.02
    from_nchw (1,16,1,1)       1.686e-07 / 1.116e-06 = 0.15  1.989e-07 / 2.163e-06 = 0.09  0.000e+00 / 4.066e-07 = 0.00
    from_nchw (2,160,6,5)      3.617e-07 / 2.225e-06 = 0.16  3.221e-06 / 1.977e-05 = 0.16  1.505e-06 / 1.673e-05 = 0.09
    from_nchw (2,64,9,9)       3.332e-07 / 2.786e-06 = 0.12  4.047e-06 / 3.944e-05 = 0.10  3.742e-06 / 3.239e-05 = 0.12
    from_nchw (1,260,3,3)      3.854e-07 / 1.960e-06 = 0.20  7.724e-07 / 7.122e-06 = 0.11  5.066e-07 / 4.883e-06 = 0.10
    from_nchw (1,512,5,5)      3.878e-07 / 2.537e-06 = 0.15  1.439e-06 / 1.337e-05 = 0.11  1.268e-06 / 1.223e-05 = 0.10
    to_nchw (1,16,1,1)         1.686e-07 / 1.116e-06 = 0.15  1.989e-07 / 2.163e-06 = 0.09  0.000e+00 / 4.066e-07 = 0.00
    to_nchw (2,160,6,5)        4.225e-07 / 2.288e-06 = 0.18  2.102e-06 / 1.468e-05 = 0.14  1.635e-06 / 1.612e-05 = 0.10
    to_nchw (2,64,9,9)         4.769e-07 / 2.317e-06 = 0.21  3.167e-06 / 3.706e-05 = 0.09  3.700e-06 / 3.426e-05 = 0.11
    to_nchw (1,260,3,3)        3.263e-07 / 1.986e-06 = 0.16  7.062e-07 / 8.433e-06 = 0.08  8.345e-07 / 5.223e-06 = 0.16
    to_nchw (1,512,5,5)        5.085e-07 / 2.881e-06 = 0.18  1.940e-06 / 1.381e-05 = 0.14  1.222e-06 / 1.026e-05 = 0.12
The largest ratio: 0.26 through the emulator, 0.28 on the MI355X.  (1,16,1,1) runs as the rows form (a map of one pixel per image is a
set of rows), hence the figures of rows (1,16).
Backbone (mit_b0, [2,3,64,64], train mode): (distance of the 'hip' model to the fp64 'torch' model) / (4 x distance of the fp32 'torch'
model to it), out0-3 | patch_embed1.proj.weight | block1.0.norm1.weight | block3.1.mlp.fc2.weight | input:
    through the emulator  0.35 0.25 0.21 0.20 | 0.13 | 0.16 | 0.39 | 0.18
    on the MI355X         0.24 0.21 0.37 0.25 | 0.09-0.10 | 0.09-0.18 | 0.28 | 0.26-0.28   (two runs: stock backward kernels with atomics)
"""
import contextlib
import ctypes as C
import functools
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import vss_cffm_amd as V
from tests import emu
from tests import test_backbone as TB
from tests.test_mixffn import CallSpy
from vss_cffm_amd import _lib
from vss_cffm_amd import backbone as B

CPU = torch.device('cpu')
EPS = 1e-6
ULP = 2.0 ** -23
GRID_CAP = 1024          # MLN_BWD_GRID_CAP of csrc/mitln_kernels.h: the rows form's records at most
# (M, C).  The last one: C = 64 runs 16 rows per workgroup; M is just past cap x 16 and no multiple of 16, so a workgroup walks more than
# one group of rows and the finalize sees the full record count
ROWS = [(1, 16), (70, 16), (7, 36), (33, 160), (9, 256), (5, 260), (6, 512), (GRID_CAP * 16 + 5, 64)]
# (B, C, H, W), both map forms
MAPS = [(1, 16, 1, 1), (2, 160, 6, 5), (2, 64, 9, 9), (1, 260, 3, 3), (1, 512, 5, 5)]
FORMS = ('rows', 'from_nchw', 'to_nchw')
CASES = [('rows', s) for s in ROWS] + [(f, s) for f in ('from_nchw', 'to_nchw') for s in MAPS]
IDS = ['%s-%s' % (f, 'x'.join(str(v) for v in s)) for f, s in CASES]
FWD = {'rows': 'cffm_ln_rows', 'from_nchw': 'cffm_nchw_ln_rows', 'to_nchw': 'cffm_ln_rows_nchw'}
BWD = {f: n + '_bwd' for f, n in FWD.items()}


# ---------------------------------------------------------------------------------------------- inputs and the yardstick
def shapes_of(form, shape):
    """-> (shape of x, shape of dout, C)"""
    if form == 'rows':
        return shape, shape, shape[1]
    b, c, h, w = shape
    return ((b, c, h, w), (b, h * w, c), c) if form == 'from_nchw' else ((b, h * w, c), (b, c, h, w), c)


@functools.lru_cache(maxsize=None)
def make_inputs(form, shape):
    xs, ds, c = shapes_of(form, shape)
    g = torch.Generator().manual_seed(0)
    x = 1.5 * torch.randn(xs, generator=g) + 2.0
    gamma = 1 + 0.3 * torch.randn(c, generator=g)
    beta = 0.3 * torch.randn(c, generator=g)
    dout = torch.randn(ds, generator=g)
    return x, gamma, beta, dout


def sequence(form, x, gamma, beta, shape):
    """the stock op sequence in the dtype of x"""
    c = gamma.numel()
    if form == 'rows':
        return F.layer_norm(x, (c,), gamma, beta, EPS)
    if form == 'from_nchw':
        return F.layer_norm(x.flatten(2).transpose(1, 2), (c,), gamma, beta, EPS)
    b, _, h, w = shape
    return F.layer_norm(x, (c,), gamma, beta, EPS).reshape(b, h, w, c).permute(0, 3, 1, 2).contiguous()


def sequence_grads(form, x, gamma, beta, dout, shape):
    x, gamma, beta = (t.detach().clone().requires_grad_(True) for t in (x, gamma, beta))
    out = sequence(form, x, gamma, beta, shape)
    out.backward(dout)
    return out.detach(), {'dx': x.grad, 'dgamma': gamma.grad, 'dbeta': beta.grad}


def as_rows(form, t, c, side):
    """x (side 'x') or dout (side 'dout') of a form as [rows][C]"""
    nchw = (form == 'from_nchw') == (side == 'x') and form != 'rows'
    return t.flatten(2).transpose(1, 2).reshape(-1, c) if nchw else t.reshape(-1, c)


class Yard:
    """fp64 yardstick of one case, its distance to the fp32 one and the magnitudes A_t; computed once and left unchanged"""

    def __init__(self, form, shape):
        x, gamma, beta, dout = make_inputs(form, shape)
        c = gamma.numel()
        self.out, self.grads = sequence_grads(form, x.double(), gamma.double(), beta.double(), dout.double(), shape)
        _, grads32 = sequence_grads(form, x, gamma, beta, dout, shape)
        self.noise = {k: float((v.double() - self.grads[k]).abs().max()) for k, v in grads32.items()}
        # the same backward with magnitudes: g -> |gamma dy|, xhat -> |xhat|, dy -> |dy|, every minus a plus
        xr, dr = as_rows(form, x.double(), c, 'x'), as_rows(form, dout.double(), c, 'dout')
        d = xr - xr.mean(1, keepdim=True)
        rstd = 1 / torch.sqrt((d * d).mean(1, keepdim=True) + EPS)
        xh, g = (d * rstd).abs(), (gamma.double() * dr).abs()
        self.mag = {'dx': float((rstd * (g + g.mean(1, keepdim=True) + xh * (g * xh).mean(1, keepdim=True))).max()),
                    'dgamma': float((dr.abs() * xh).sum(0).max()), 'dbeta': float(dr.abs().sum(0).max())}

    def gate(self, k):
        return 4 * self.noise[k] + ULP * self.mag[k]


@functools.lru_cache(maxsize=None)
def yard(form, shape):
    return Yard(form, shape)


def check(form, shape, got, tag=''):
    y = yard(form, shape)
    for k, t in got.items():
        assert tuple(t.shape) == tuple(y.grads[k].shape), (form, shape, k, tuple(t.shape))
        err = float((t.detach().cpu().double() - y.grads[k]).abs().max())
        print('%s %s%s %s: max err %.3e / gate %.3e = %.2f (4 x noise %.3e + 2^-23 x %.3e)'
              % (form, shape, tag, k, err, y.gate(k), err / y.gate(k), y.noise[k], y.mag[k]))
        assert err <= y.gate(k), (form, shape, k, err, y.gate(k))


# ---------------------------------------------------------------------------------------------- the C ABI, called directly
def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else C.c_void_p(0)


def _st(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def _sync(device):
    if device.type == 'cuda':
        torch.cuda.synchronize()


def ws_dims(form, shape):
    if form == 'rows':
        return shape[0], shape[1], 1
    b, c, h, w = shape
    return b * h * w, c, h * w


TAIL = 64        # floats behind dx, dgamma and dbeta that must stay as they were


def raw_bwd(lib, form, shape, x, gamma, dout, ws_fill=float('nan'), null=(), off=None, eps=EPS):
    """-> (rc, dx, dgamma, dbeta), each with TAIL more floats behind it than it needs; outputs and workspace pre-filled with NaN (or
    `ws_fill`).  `null`: names passed as null pointers; `off` = (name, bytes): that pointer moved"""
    dx = torch.full((x.numel() + TAIL,), float('nan'), device=x.device)
    dgamma, dbeta = (torch.full((gamma.numel() + TAIL,), float('nan'), device=x.device) for _ in range(2))
    nbytes = lib.cffm_ln_bwd_workspace_bytes(*ws_dims(form, shape))
    ws = torch.full((max(nbytes, 16) // 4 + TAIL,), ws_fill, device=x.device)
    ptrs = {'x': x, 'gamma': gamma, 'dout': dout, 'dx': dx, 'dgamma': dgamma, 'dbeta': dbeta, 'ws': ws}
    args = [_p(None if n in null else t, off[1] if off and off[0] == n else 0) for n, t in ptrs.items()]
    rc = getattr(lib, BWD[form])(*args, *shape, eps, _st(x))
    return rc, dx, dgamma, dbeta


def split_tail(t, shape):
    n = 1
    for v in shape:
        n *= v
    return t[:n].reshape(shape), t[n:]


def on(device, form, shape):
    return tuple(t.to(device) for t in make_inputs(form, shape))


def run_raw(lib, device, form, shape, x, gamma, dout, ws_fill=float('nan')):
    """one raw call that must succeed -> dx, dgamma, dbeta in their shapes; the TAIL floats behind each are still NaN"""
    rc, dx, dgamma, dbeta = raw_bwd(lib, form, shape, x, gamma, dout, ws_fill)
    assert rc == 0, lib.cffm_last_error()
    _sync(device)
    out = {}
    for k, t, s in (('dx', dx, tuple(x.shape)), ('dgamma', dgamma, (gamma.numel(),)), ('dbeta', dbeta, (gamma.numel(),))):
        out[k], tail = split_tail(t, s)
        assert bool(tail.isnan().all()), '%s: written past the end' % k
        assert not bool(out[k].isnan().any()), '%s: not every element written' % k
    return out


# ---------------------------------------------------------------------------------------------- bodies shared with the GPU half
def fn_of(form, shape):
    if form == 'rows':
        return V.layer_norm_rows, V.ln_rows, ()
    fn, inf = (V.nchw_layer_norm_rows, V.nchw_ln_rows) if form == 'from_nchw' else (V.layer_norm_rows_nchw, V.ln_rows_nchw)
    return fn, inf, (() if form == 'from_nchw' else (shape[2], shape[3]))


def autograd_grads(form, shape, x, gamma, beta, dout):
    fn, _, hw = fn_of(form, shape)
    xg, gg, bg = (t.detach().clone().requires_grad_(True) for t in (x, gamma, beta))
    out = fn(xg, gg, bg, *hw, eps=EPS)
    out.backward(dout)
    return out.detach(), {'dx': xg.grad, 'dgamma': gg.grad, 'dbeta': bg.grad}


def run_shape(device, form, shape):
    """the raw C ABI and autograd against the yardstick; the sentinels behind dx / dgamma / dbeta stay"""
    lib = _lib.get()
    x, gamma, beta, dout = on(device, form, shape)
    raw = run_raw(lib, device, form, shape, x, gamma, dout)
    check(form, shape, raw, ' (C ABI)')
    _, auto = autograd_grads(form, shape, x, gamma, beta, dout)
    check(form, shape, auto, ' (autograd)')
    for k in raw:
        assert torch.equal(raw[k], auto[k]), k


def run_forward(device, form, shape):
    """the differentiable function's output has the bits of the inference function's, grad mode on or off; no_grad: no grad_fn"""
    fn, inf, hw = fn_of(form, shape)
    x, gamma, beta, _ = on(device, form, shape)
    with torch.no_grad():
        want = inf(x, gamma, beta, *hw, eps=EPS)
        got = fn(x.clone().requires_grad_(True), gamma, beta, *hw, eps=EPS)
    assert got.grad_fn is None and not got.requires_grad and torch.equal(got, want) and got.is_contiguous()
    xg = x.clone().requires_grad_(True)
    out = fn(xg, gamma, beta, *hw, eps=EPS)
    assert out.grad_fn is not None and torch.equal(out.detach(), want)
    with pytest.raises(_lib.CffmError):           # the inference functions keep their contract
        inf(xg, gamma, beta, *hw, eps=EPS)
    with CallSpy(_lib.get(), (FWD[form], BWD[form], 'cffm_ln_bwd_workspace_bytes')) as spy:
        with torch.no_grad():
            fn(xg, gamma, beta, *hw, eps=EPS)
    assert spy.calls == {FWD[form]: 1, BWD[form]: 0, 'cffm_ln_bwd_workspace_bytes': 0}


def run_poison_and_determinism(device, form, shape):
    """a NaN-filled, a zero-filled and a second NaN-filled workspace: finite results, the same bits of dx, dgamma and dbeta"""
    lib = _lib.get()
    x, gamma, _, dout = on(device, form, shape)
    runs = [run_raw(lib, device, form, shape, x, gamma, dout, fill) for fill in (float('nan'), 0.0, float('nan'))]
    for r in runs:
        for k, t in r.items():
            assert bool(t.isfinite().all()) and torch.equal(t, runs[0][k]), k


def run_no_leak(device, form, shape=(2, 64, 9, 9)):
    """image 0 of x and of dout all NaN: the dx of image 1 has the bits it had before, that of image 0 is NaN"""
    lib = _lib.get()
    x, gamma, _, dout = on(device, form, shape)
    want = run_raw(lib, device, form, shape, x, gamma, dout)
    x, dout = x.clone(), dout.clone()
    x[0], dout[0] = float('nan'), float('nan')
    rc, dx, _, _ = raw_bwd(lib, form, shape, x, gamma, dout)
    assert rc == 0
    _sync(device)
    dx, tail = split_tail(dx, tuple(x.shape))
    assert bool(tail.isnan().all()) and bool(dx[0].isnan().all()) and torch.equal(dx[1], want['dx'][1])


def run_errors(device):
    """every refusal: non-zero, cffm_last_error set, the NaN-prefilled dx / dgamma / dbeta still NaN"""
    lib = _lib.get()
    n = 4096                                                      # room for every shape below, were one of them to run after all
    x, dout = torch.ones(n, device=device), torch.ones(n, device=device)
    gamma = torch.ones(1024, device=device)
    nan = float('nan')
    cases = [('rows', (2, 12), {}), ('rows', (2, 18), {}), ('rows', (2, 516), {}), ('rows', (0, 64), {}),
             ('rows', (2, 64), {'eps': -1.0}), ('rows', (2, 64), {'eps': nan}), ('rows', (2, 64), {'eps': float('inf')})]
    for form in ('from_nchw', 'to_nchw'):
        cases += [(form, s, {}) for s in ((1, 12, 2, 2), (1, 18, 2, 2), (1, 516, 1, 2), (0, 64, 2, 2), (1, 64, 0, 2), (1, 64, 2, 0))]
        cases += [(form, (1, 64, 2, 2), {'eps': -1.0}), (form, (1, 64, 2, 2), {'eps': nan})]
    for form in FORMS:
        s = (2, 64) if form == 'rows' else (1, 64, 2, 1)
        cases += [(form, s, {'null': (name,)}) for name in ('x', 'gamma', 'dout', 'dx', 'dgamma', 'dbeta', 'ws')]
        cases += [(form, s, {'off': (name, 4)}) for name in ('x', 'gamma', 'dout', 'dx', 'dgamma', 'dbeta', 'ws')]
    for form, shape, kw in cases:
        rc, dx, dgamma, dbeta = raw_bwd(lib, form, shape, x, gamma, dout, **kw)
        assert rc != 0 and lib.cffm_last_error() != b'', (form, shape, kw)
        _sync(device)
        assert all(bool(t.isnan().all()) for t in (dx, dgamma, dbeta)), (form, shape, kw)
    for m, c, hw in ((0, 64, 1), (4, 12, 1), (4, 18, 1), (4, 516, 1), (10, 64, 3), (4, 64, 0), (4, 64, -1), (2 ** 31 // 64, 64, 1)):
        assert lib.cffm_ln_bwd_workspace_bytes(m, c, hw) < 0, (m, c, hw)
    assert lib.cffm_ln_bwd_workspace_bytes(4, 64, 1) == 2 * 64 * 4 and lib.cffm_ln_bwd_workspace_bytes(162, 64, 81) == 2 * 2 * 2 * 64 * 4
    w, b = torch.ones(64, device=device), torch.zeros(64, device=device)
    rows, img = torch.zeros(2, 6, 64, device=device), torch.zeros(2, 64, 3, 2, device=device)
    for bad in (lambda: V.layer_norm_rows(rows, w[:32], b), lambda: V.layer_norm_rows(rows, w, b[:32]),
                lambda: V.layer_norm_rows(rows, w.reshape(1, 64), b), lambda: V.layer_norm_rows(rows.double(), w, b),
                lambda: V.layer_norm_rows(rows[:, :, :12], w[:12], b[:12]), lambda: V.layer_norm_rows(rows[:0], w, b),
                lambda: V.nchw_layer_norm_rows(img, w[:32], b[:32]), lambda: V.nchw_layer_norm_rows(rows, w, b),
                lambda: V.layer_norm_rows_nchw(rows, w, b, 2, 2), lambda: V.layer_norm_rows_nchw(rows, w[:32], b, 3, 2),
                lambda: V.layer_norm_rows_nchw(img, w, b, 3, 2)):
        with pytest.raises(_lib.CffmError):
            bad()


def run_non_contiguous(device, form, shape):
    """x and dout as a transposed view and as a slice of a wider tensor: the bits of their contiguous copies"""
    x, gamma, beta, dout = on(device, form, shape)
    want_out, want = autograd_grads(form, shape, x, gamma, beta, dout)

    def transposed(t):
        v = t.transpose(-1, -2).contiguous().transpose(-1, -2)
        assert not v.is_contiguous() and torch.equal(v, t)
        return v

    def sliced(t):
        wide = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + 3,), float('nan'), device=t.device)
        wide[..., 1:-2] = t
        v = wide[..., 1:-2]
        assert not v.is_contiguous() and v.data_ptr() % 16 != 0
        return v

    for view in (transposed, sliced):
        out, got = autograd_grads(form, shape, view(x), gamma, beta, view(dout))
        assert torch.equal(out, want_out)
        for k in want:
            assert torch.equal(got[k], want[k]), (view.__name__, k)


# ---- the backbone
LN_FWD, LN_BWD = tuple(FWD.values()), tuple(BWD.values())
COMPARED = ('patch_embed1.proj.weight', 'block1.0.norm1.weight', 'block3.1.mlp.fc2.weight')


@contextlib.contextmanager
def no_override():
    prev, _lib._override = _lib._override, None
    try:
        yield
    finally:
        _lib._override = prev


def picked(outs, dimg, grads):
    d = {'out%d' % i: o.detach() for i, o in enumerate(outs)}
    d.update({k: grads[k] for k in COMPARED})
    d['input'] = dimg
    return {k: v.detach().cpu().double() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def backbone_yard():
    """the 'torch' model on the CPU in fp64 and in fp32 (stock PyTorch throughout) -> (fp64 results, 4 x their distance)"""
    with no_override():
        want = picked(*TB.train_pass(TB.make(CPU, 'mit_b0', torch.float64), CPU, torch.float64))
        f32 = picked(*TB.train_pass(TB.make(CPU, 'mit_b0'), CPU))
    return want, {k: 4 * float((f32[k] - want[k]).abs().max()) for k in want}


def run_backbone(device):
    lib = _lib.get()
    want, gates = backbone_yard()
    m = TB.make(device, 'mit_b0')
    assert m.norm_impl == 'torch' and B.Block.norm_impl == 'torch' and B.OverlapPatchEmbed.norm_impl == 'torch' and B.Attention.norm_impl == 'torch'
    with CallSpy(lib, LN_FWD + LN_BWD) as spy:
        outs_t, _, _ = TB.train_pass(m, device)
    assert sum(spy.calls.values()) == 0
    # a model in which the switch cannot act: the two helpers the call sites go through replaced by the stock lines
    fused, rows = B._norm_fused, B._norm_rows
    B._norm_fused, B._norm_rows = (lambda *a: False), (lambda impl, norm, x: norm(x))
    try:
        outs_s, _, _ = TB.train_pass(TB.make(device, 'mit_b0'), device)
    finally:
        B._norm_fused, B._norm_rows = fused, rows
    assert all(torch.equal(a, b) for a, b in zip(outs_t, outs_s))
    with pytest.raises(ValueError):
        m.set_norm_impl('cuda')
    m.set_norm_impl('hip')
    m.zero_grad()
    with CallSpy(lib, LN_FWD + LN_BWD) as spy:
        got = picked(*TB.train_pass(m, device))
    # 4 embeddings, 16 block norms + 6 behind an `sr` convolution (stages 1-3), 4 stage norms
    assert [spy.calls[n] for n in LN_FWD] == [22, 4, 4] and [spy.calls[n] for n in LN_BWD] == [22, 4, 4], spy.calls
    for k in want:
        err = float((got[k] - want[k]).abs().max())
        print('mit_b0 norm_impl=hip %s: err %.3e / gate %.3e = %.2f' % (k, err, gates[k], err / gates[k]))
        assert err <= gates[k], (k, err, gates[k])
    m.set_norm_impl('torch')
    assert all(mod.norm_impl == 'torch' for mod in m.modules() if hasattr(type(mod), 'norm_impl'))


def run_backbone_outside_the_limits(device):
    """norms the kernels cannot take -- a width above 512, a subclass of nn.LayerNorm -- take the stock line without raising"""
    lib = _lib.get()
    kw = dict(img_size=32, patch_size=4, num_heads=[1, 1, 1, 1], mlp_ratios=[1, 1, 1, 1], depths=[1, 1, 1, 1], sr_ratios=[2, 1, 1, 1],
              qkv_bias=True)
    g = torch.Generator().manual_seed(3)
    img = torch.randn(1, 3, 32, 32, generator=g).to(device)

    class OtherNorm(nn.LayerNorm):
        pass

    for extra, hip_calls in ((dict(embed_dims=[32, 64, 64, 576]), 13), (dict(embed_dims=[32, 32, 32, 32], norm_layer=OtherNorm), 5)):
        m = B.MixVisionTransformer(**kw, **extra).to(device).train()
        ref = [o.detach() for o in m(img)]
        m.set_norm_impl('hip')
        with CallSpy(lib, LN_FWD) as spy:
            outs = m(img)
            sum(o.sum() for o in outs).backward()
        # widths inside the limits still take the library: (embedding + norm1 + norm2 + stage) x 3 stages + stage 1's sr norm = 13;
        # with another norm_layer only the embeddings' norms and the `sr` norm (always plain nn.LayerNorm) qualify = 5
        assert sum(spy.calls.values()) == hip_calls, spy.calls
        for o, r in zip(outs, ref):
            assert o.shape == r.shape and float((o.detach() - r).abs().max()) <= 1e-4 * max(1., float(r.abs().max()))


# ---------------------------------------------------------------------------------------------- emulator
def test_symbols_and_exports():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cffm_hip.h')).read()
    lib = emu.lib()
    for n in ('cffm_ln_bwd_workspace_bytes',) + LN_BWD:
        assert n + '(' in text and n in _lib.SIGNATURES and hasattr(lib, n)
    assert lib.cffm_abi_version() == 13
    for n in ('layer_norm_rows', 'nchw_layer_norm_rows', 'layer_norm_rows_nchw'):
        assert callable(getattr(V, n))


@pytest.mark.parametrize('form,shape', CASES, ids=IDS)
def test_shapes_against_the_stock_sequence(form, shape):
    with emu.active():
        run_shape(CPU, form, shape)


@pytest.mark.parametrize('form,shape', [('rows', (7, 36)), ('rows', (5, 260)), ('from_nchw', (2, 160, 6, 5)), ('to_nchw', (2, 160, 6, 5))])
def test_forward_is_the_inference_call(form, shape):
    with emu.active():
        run_forward(CPU, form, shape)


@pytest.mark.parametrize('form', FORMS)
def test_poisoned_workspace_and_determinism(form):
    with emu.active():
        for shape in ((70, 16), (5, 260)) if form == 'rows' else ((2, 64, 9, 9), (1, 260, 3, 3)):
            run_poison_and_determinism(CPU, form, shape)


@pytest.mark.parametrize('form', ('from_nchw', 'to_nchw'))
def test_nothing_leaks_across_images(form):
    with emu.active():
        run_no_leak(CPU, form)


def test_errors_leave_the_outputs_untouched():
    with emu.active():
        run_errors(CPU)


@pytest.mark.parametrize('form,shape', [('rows', (33, 160)), ('from_nchw', (2, 64, 9, 9)), ('to_nchw', (2, 160, 6, 5))])
def test_non_contiguous_inputs(form, shape):
    with emu.active():
        run_non_contiguous(CPU, form, shape)


def test_backbone_norm_impl():
    with emu.active():
        run_backbone(CPU)


def test_backbone_norms_outside_the_limits():
    with emu.active():
        run_backbone_outside_the_limits(CPU)


def test_no_cpu_fallback():
    """a CPU tensor without the emulator raises, GPU present or not"""
    w, b = torch.ones(16), torch.zeros(16)
    for bad in (lambda: V.layer_norm_rows(torch.zeros(2, 16), w, b), lambda: V.nchw_layer_norm_rows(torch.zeros(1, 16, 2, 2), w, b),
                lambda: V.layer_norm_rows_nchw(torch.zeros(1, 4, 16), w, b, 2, 2)):
        with pytest.raises(_lib.CffmError):
            bad()
