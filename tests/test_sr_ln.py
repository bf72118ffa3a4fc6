"""The fused spatial-reduction convolution + LayerNorm (include/cffm_hip.h: cffm_sr_ln_fwd / _bwd, vss_cffm_amd.sr_reduce) on the CPU through
the fiber emulator.  The GPU half is tests/test_sr_ln_gpu.py and shares the run_*(device) bodies below.

The yardstick is the reference's lines (backbones/mix_transformer.py Attention.forward, sr_ratio > 1): permute / reshape to NCHW,
Conv2d(C, C, kernel_size=s, stride=s), reshape / permute back, LayerNorm(C) with eps = 1e-5, in fp64 on the CPU.  Inputs from
torch.Generator().manual_seed(0), drawn in this order: x = randn(B,H*W,C), w = randn(C,C,s,s) / sqrt(s*s*C), b = randn(C) (+ 30 for
`offset`), gamma = 1 + 0.1 randn(C), beta = 0.1 randn(C), dout = randn(B,Ho*Wo,C).

Rule, for each t of out, dx, dw, db, dgamma, dbeta:  max|t - t64| <= 4 noise_t + 2.5e-7 A_t, noise_t = max|fp32 op sequence - fp64 op
sequence| computed inside the test; A_t = the same fp64 computation on magnitudes with the true normalised rows xhat and rstd:
A_out = max(|xhat| |gamma| + |beta|); with dz_a = rstd (|dout gamma| + mean|dout gamma| + |xhat| mean(|dout gamma| |xhat|)):
A_dx = max(dz_a |W|^T), A_dw = max(dz_a^T |x patches|), A_db = max(sum_m dz_a), A_dgamma = max(sum_m |dout| |xhat|),
A_dbeta = max(sum_m |dout|).  The dx of the dropped last rows / columns (`tail`) must be exactly 0.  The saved rows z are held to the same
rule (noise = the fp32 convolution's distance to fp64, A = the convolution on magnitudes), their means to it plus the roundings of the sum.

Measured through the emulator (error / gate):
    shape    out                  dx                   dw                   db                   dgamma               dbeta
    one      3.29e-07 / 1.34e-06  2.40e-07 / 1.93e-06  4.71e-07 / 4.23e-06  1.48e-07 / 1.15e-06  4.79e-07 / 2.26e-06  0.00e+00 / 6.67e-07
    b0s1     6.94e-07 / 7.82e-06  8.79e-08 / 7.60e-07  1.81e-06 / 1.49e-05  9.79e-07 / 6.44e-06  8.73e-07 / 1.92e-05  3.35e-07 / 4.32e-06
    s4       1.07e-06 / 5.26e-06  4.58e-07 / 3.11e-06  2.18e-06 / 1.47e-05  7.17e-07 / 5.64e-06  2.83e-06 / 8.59e-06  4.92e-07 / 4.00e-06
    tail     5.85e-07 / 5.18e-06  3.15e-07 / 3.34e-06  1.45e-06 / 1.75e-05  5.22e-07 / 9.45e-06  1.36e-06 / 1.21e-05  6.93e-07 / 6.37e-06
    c160     7.48e-07 / 4.55e-06  5.98e-07 / 4.76e-06  1.79e-06 / 1.16e-05  5.65e-07 / 5.36e-06  1.65e-06 / 9.22e-06  5.07e-07 / 4.59e-06
    c320     6.93e-07 / 5.11e-06  7.39e-07 / 6.09e-06  1.22e-06 / 1.38e-05  3.57e-07 / 4.15e-06  1.20e-06 / 9.64e-06  3.58e-07 / 3.48e-06
    rows     8.21e-07 / 8.21e-06  4.43e-07 / 4.21e-06  5.58e-06 / 1.07e-04  2.12e-06 / 6.51e-05  4.56e-06 / 5.13e-05  4.37e-06 / 3.17e-05
    offset   2.83e-06 / 1.90e-05  2.73e-07 / 3.51e-06  1.99e-06 / 2.89e-05  6.84e-07 / 1.24e-05  4.82e-06 / 5.45e-05  4.92e-07 / 4.00e-06
    c48      3.71e-07 / 3.11e-06  2.41e-07 / 2.60e-06  6.91e-07 / 7.72e-06  2.19e-07 / 3.34e-06  9.41e-07 / 6.02e-06  1.73e-07 / 2.16e-06
    c512     6.62e-07 / 3.26e-06  9.97e-07 / 5.70e-06  8.81e-07 / 9.87e-06  1.93e-07 / 2.05e-06  1.13e-06 / 4.44e-06  0.00e+00 / 8.22e-07
On the MI355X (error / gate):
    shape    out                  dx                   dw                   db                   dgamma               dbeta
    one      3.29e-07 / 2.39e-06  2.40e-07 / 1.84e-06  4.71e-07 / 4.23e-06  1.48e-07 / 1.15e-06  4.79e-07 / 2.11e-06  0.00e+00 / 6.67e-07
    b0s1     6.94e-07 / 7.82e-06  8.79e-08 / 7.60e-07  1.97e-06 / 1.49e-05  5.03e-07 / 6.44e-06  8.73e-07 / 1.92e-05  3.35e-07 / 4.32e-06
    s4       1.04e-06 / 5.26e-06  4.58e-07 / 3.11e-06  2.18e-06 / 1.47e-05  7.17e-07 / 5.64e-06  2.83e-06 / 8.59e-06  4.92e-07 / 4.00e-06
    tail     4.40e-07 / 5.03e-06  3.55e-07 / 3.02e-06  1.44e-06 / 1.64e-05  5.71e-07 / 1.03e-05  1.36e-06 / 1.29e-05  6.93e-07 / 6.61e-06
    c160     6.29e-07 / 1.24e-05  5.98e-07 / 4.54e-06  1.79e-06 / 1.24e-05  3.89e-07 / 5.83e-06  1.65e-06 / 2.14e-05  5.07e-07 / 4.59e-06
    c320     6.79e-07 / 2.66e-05  7.39e-07 / 5.79e-06  1.22e-06 / 1.24e-05  4.03e-07 / 4.64e-06  1.20e-06 / 4.13e-05  3.58e-07 / 3.48e-06
    rows     7.92e-07 / 8.21e-06  4.86e-07 / 4.21e-06  5.58e-06 / 1.07e-04  2.23e-06 / 6.70e-05  4.55e-06 / 5.29e-05  4.37e-06 / 3.69e-05
    offset   2.83e-06 / 1.90e-05  3.12e-07 / 3.51e-06  1.68e-06 / 2.89e-05  6.76e-07 / 1.24e-05  4.82e-06 / 5.45e-05  4.92e-07 / 4.00e-06
    c48      3.71e-07 / 8.09e-06  2.07e-07 / 3.07e-06  6.91e-07 / 1.04e-05  2.59e-07 / 3.47e-06  9.41e-07 / 2.09e-05  1.73e-07 / 2.16e-06
    c512     6.62e-07 / 6.20e-06  1.06e-06 / 7.33e-06  8.80e-07 / 9.01e-06  1.93e-07 / 1.96e-06  1.13e-06 / 1.08e-05  0.00e+00 / 8.22e-07
(the gates differ a little from the emulator's table: the fp32 yardstick, whose noise sets them, runs on the CPU of the machine.)
"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import vss_cffm_amd as V
from tests import emu
from tests.test_mixffn import CallSpy
from vss_cffm_amd import _lib

# (B, H, W, C, s, bias offset): the smallest shapes at which each mechanism can go wrong
SHAPES = {
    'one': (1, 2, 2, 32, 2, 0),           # one output row, one K slab
    'b0s1': (2, 16, 16, 32, 8, 0),        # K = 2048, narrowest C, two images, 4 rows per image: far fewer rows than a tile
    's4': (1, 8, 12, 128, 4, 0),          # s = 4, H != W
    'tail': (1, 9, 7, 64, 2, 0),          # a dropped last row and column
    'c160': (1, 6, 4, 160, 2, 0),         # C not a power of two: 10 column tiles (two groups of 5)
    'c320': (1, 4, 4, 320, 2, 0),         # the widest workload C, K = 1280
    'rows': (3, 10, 14, 64, 2, 0),        # M = 105: several row tiles, a ragged last one, rows crossing image boundaries
    'offset': (1, 8, 12, 128, 4, 30),     # row mean >> row spread: a variance from E[z^2] - mean^2 fails this
    'c48': (1, 4, 4, 48, 2, 0),           # 3 column tiles: the forward's one-tile-per-wave column groups
    'c512': (1, 2, 2, 512, 2, 0),         # the widest C of the limits: 16 values per lane in the LayerNorm, 8 column groups
}
APPROX = 2.5e-7
EPS = 1e-5
NAMES = tuple(SHAPES)
KEYS = ('out', 'dx', 'dw', 'db', 'dgamma', 'dbeta')
GUARD = 8           # words past the end of every output
NAMES_ABI = ('cffm_sr_ln_fwd', 'cffm_sr_ln_bwd_workspace_bytes', 'cffm_sr_ln_bwd')


# ---------------------------------------------------------------------------------------------- inputs and the yardstick
@functools.lru_cache(maxsize=None)
def make_inputs(shape):
    b, h, w, c, s, off = shape
    g = torch.Generator().manual_seed(0)
    x = torch.randn(b, h * w, c, generator=g)
    wt = torch.randn(c, c, s, s, generator=g) / (s * s * c) ** 0.5
    bias = torch.randn(c, generator=g) + off
    gamma = 1 + 0.1 * torch.randn(c, generator=g)
    beta = 0.1 * torch.randn(c, generator=g)
    dout = torch.randn(b, (h // s) * (w // s), c, generator=g)
    return x, wt, bias, gamma, beta, dout


def conv_rows(x, wt, bias, h, w, s):
    """the reference's lines up to the LayerNorm, in the dtype of x -> [B, Ho*Wo, C]"""
    b, _, c = x.shape
    return F.conv2d(x.permute(0, 2, 1).reshape(b, c, h, w), wt, bias, stride=s).reshape(b, c, -1).permute(0, 2, 1)


def op_sequence(x, wt, bias, gamma, beta, h, w, s):
    return F.layer_norm(conv_rows(x, wt, bias, h, w, s), (x.shape[2],), gamma, beta, EPS)


def sequence_grads(ts, h, w, s):
    x, wt, bias, gamma, beta = (t.detach().clone().requires_grad_(True) for t in ts[:5])
    out = op_sequence(x, wt, bias, gamma, beta, h, w, s)
    out.backward(ts[5])
    return {'out': out.detach(), 'dx': x.grad, 'dw': wt.grad, 'db': bias.grad, 'dgamma': gamma.grad, 'dbeta': beta.grad}


class Yard:
    """fp64 yardstick of one shape, its distance to the fp32 one and the magnitudes A_t; computed once and left unchanged"""

    def __init__(self, shape):
        b, h, w, c, s, _ = shape
        ts = make_inputs(shape)
        t64 = tuple(t.double() for t in ts)
        self.want = sequence_grads(t64, h, w, s)
        got32 = sequence_grads(ts, h, w, s)
        self.noise = {k: float((got32[k].double() - self.want[k]).abs().max()) for k in KEYS}
        x, wt, bias, gamma, beta, dout = t64
        z = conv_rows(x, wt, bias, h, w, s)
        rstd = (z.var(dim=-1, unbiased=False, keepdim=True) + EPS).rsqrt()
        xh = ((z - z.mean(dim=-1, keepdim=True)) * rstd).abs()
        dy = (dout * gamma).abs()
        dz = rstd * (dy + dy.mean(dim=-1, keepdim=True) + xh * (dy * xh).mean(dim=-1, keepdim=True))          # [B, L, C]
        ho, wo = h // s, w // s
        xa = x.abs().permute(0, 2, 1).reshape(b, c, h, w)[:, :, :ho * s, :wo * s]
        patches = F.unfold(xa, kernel_size=s, stride=s)                                                          # [B, C s s, L], (ci, ky, kx)
        # the saved rows z (and their means) under the same rule: the fp32 convolution's own distance to fp64, the convolution on magnitudes
        self.z = z.reshape(-1, c)
        z32 = conv_rows(*ts[:3], h, w, s).reshape(-1, c).double()
        self.z_gate = 4 * float((z32 - self.z).abs().max()) + APPROX * float((patches.transpose(1, 2) @ wt.abs().reshape(c, -1).t()
                                                                              + bias.abs()).max())
        self.mag = {'out': float((xh * gamma.abs() + beta.abs()).max()),
                    'dx': float((dz @ wt.abs().reshape(c, -1)).max()),
                    'dw': float(torch.einsum('blo,bkl->ok', dz, patches).max()),
                    'db': float(dz.sum(dim=(0, 1)).max()),
                    'dgamma': float((dout.abs() * xh).sum(dim=(0, 1)).max()),
                    'dbeta': float(dout.abs().sum(dim=(0, 1)).max())}

    def gate(self, k):
        return 4 * self.noise[k] + APPROX * self.mag[k]


@functools.lru_cache(maxsize=None)
def yard(name):
    return Yard(SHAPES[name])


def check(name, got, tag=''):
    y = yard(name)
    for k, t in got.items():
        err = float((t.detach().cpu().double() - y.want[k]).abs().max())
        print('%s%s %s: max err %.3e (gate %.3e = 4 x noise %.3e + 2.5e-7 x %.3e), max|%s| %.3e'
              % (name, tag, k, err, y.gate(k), y.noise[k], y.mag[k], k, float(y.want[k].abs().max())))
        assert bool(t.isfinite().all()), (name, k)
        assert err <= y.gate(k), (name, k, err, y.gate(k))


def tail_mask(shape):
    """[H*W] bool: the pixels no window covers"""
    _, h, w, _, s, _ = shape
    m = torch.ones(h, w, dtype=torch.bool)
    m[:h // s * s, :w // s * s] = False
    return m.reshape(-1)


# ---------------------------------------------------------------------------------------------- the C ABI, called directly
def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else C.c_void_p(0)


def _st(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def _sync(device):
    if device.type == 'cuda':
        torch.cuda.synchronize()


def dims(shape):
    return shape[:5]


def guarded(shape, device, fill=float('nan')):
    """a `fill`-filled tensor of `shape` whose storage goes on for GUARD words holding 12345 -> (tensor, guard words)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), fill, device=device)
    buf[n:] = 12345.0
    return buf[:n].view(shape), buf[n:]


def guards_intact(guards):
    return all(bool((g == 12345.0).all()) for g in guards)


def raw_fwd(lib, ts, shape, saved=True, x_off=0):
    """-> (rc, out, z, stats, guards); the outputs pre-filled with NaN"""
    b, h, w, c, s = dims(shape)
    x, wt, bias, gamma, beta = ts[:5]
    m = b * (h // s) * (w // s)
    out, g0 = guarded((b, m // b, c), x.device)
    z, g1 = guarded((m, c), x.device)
    stats, g2 = guarded((m, 2), x.device)
    rc = lib.cffm_sr_ln_fwd(_p(x, x_off), _p(wt), _p(bias), _p(gamma), _p(beta), _p(out), _p(z if saved else None),
                            _p(stats if saved else None), b, h, w, c, s, EPS, _st(x))
    return rc, out, z, stats, (g0, g1, g2)


def raw_bwd(lib, ts, z, stats, shape, ws_fill=float('nan'), x_off=0):
    """-> (rc, grads dict, workspace, guards); the outputs and the workspace are pre-filled with NaN (or `ws_fill`)"""
    b, h, w, c, s = dims(shape)
    x, wt, bias, gamma, beta, dout = ts
    dx, g0 = guarded(tuple(x.shape), x.device)
    dw, g1 = guarded(tuple(wt.shape), x.device)
    db, g2 = guarded((c,), x.device)
    dgamma, g3 = guarded((c,), x.device)
    dbeta, g4 = guarded((c,), x.device)
    nbytes = lib.cffm_sr_ln_bwd_workspace_bytes(b, h, w, c, s)
    ws, g5 = guarded((max(nbytes, 16) // 4,), x.device, ws_fill)
    rc = lib.cffm_sr_ln_bwd(_p(x, x_off), _p(wt), _p(gamma), _p(z), _p(stats), _p(dout), _p(dx), _p(dw), _p(db), _p(dgamma), _p(dbeta), _p(ws),
                            b, h, w, c, s, EPS, _st(x))
    return rc, {'dx': dx, 'dw': dw, 'db': db, 'dgamma': dgamma, 'dbeta': dbeta}, ws, (g0, g1, g2, g3, g4, g5)


def on(device, shape):
    return tuple(t.to(device) for t in make_inputs(shape))


# ---------------------------------------------------------------------------------------------- bodies shared with the GPU half
def run_shape(device, name):
    """forward with and without z / stats, backward; NaN-poisoned outputs and workspace, guard words; everything against the yardstick"""
    lib = _lib.get()
    shape = SHAPES[name]
    ts = on(device, shape)
    rc, out, z, stats, gf = raw_fwd(lib, ts, shape)
    assert rc == 0, lib.cffm_last_error()
    rc, out2, z2, stats2, gf2 = raw_fwd(lib, ts, shape, saved=False)
    assert rc == 0, lib.cffm_last_error()
    rc, grads, ws, gb = raw_bwd(lib, ts, z, stats, shape)
    assert rc == 0, lib.cffm_last_error()
    _sync(device)
    assert guards_intact(gf + gf2 + gb)
    assert torch.equal(out2, out) and bool(z2.isnan().all()) and bool(stats2.isnan().all())
    assert bool(z.isfinite().all()) and bool(stats.isfinite().all())
    check(name, dict(grads, out=out))
    # the saved rows are the convolution's, the statistics theirs
    y = yard(name)
    b, h, w, c, s = dims(shape)
    ez = float((z.cpu().double() - y.z).abs().max())
    em = float((stats[:, 0].cpu().double() - y.z.mean(dim=1)).abs().max())
    # the mean is a sum of C values, each within the gate, taken in at most C / 32 + 5 additions and one division of fp32
    slack = (c // 32 + 6) * 2.0 ** -24 * float(y.z.abs().max())
    print('%s z: max err %.3e (gate %.3e), row mean: max err %.3e (gate + %.3e)' % (name, ez, y.z_gate, em, slack))
    assert ez <= y.z_gate and em <= y.z_gate + slack
    tm = tail_mask(shape).to(device)
    assert not bool(grads['dx'][:, tm].any()) and int(tm.sum()) == h * w - (h // s * s) * (w // s * s)
    return out, grads


def run_determinism(device, name):
    """a NaN-filled, a zero-filled and a second NaN-filled workspace: the same bits of every gradient"""
    lib = _lib.get()
    shape = SHAPES[name]
    ts = on(device, shape)
    rc, out, z, stats, _ = raw_fwd(lib, ts, shape)
    assert rc == 0
    runs = [raw_bwd(lib, ts, z, stats, shape, fill) for fill in (float('nan'), 0.0, float('nan'))]
    _sync(device)
    for rc, grads, ws, g in runs:
        assert rc == 0 and guards_intact(g)
        for k, t in grads.items():
            assert bool(t.isfinite().all()) and torch.equal(t, runs[0][1][k]), k


def run_autograd(device, name='tail'):
    """sr_reduce(...).backward gives the tensors of the direct call; so do a non-contiguous x and a weight sliced out of a larger buffer"""
    lib = _lib.get()
    shape = SHAPES[name]
    b, h, w, c, s = dims(shape)
    ts = on(device, shape)
    rc, out, z, stats, _ = raw_fwd(lib, ts, shape)
    assert rc == 0
    rc, grads, _, _ = raw_bwd(lib, ts, z, stats, shape)
    assert rc == 0
    leaves = [t.clone().requires_grad_(True) for t in ts[:5]]
    o = V.sr_reduce(*leaves, h, w, s, EPS)
    o.backward(ts[5])
    _sync(device)
    got = dict(zip(('dx', 'dw', 'db', 'dgamma', 'dbeta'), (t.grad for t in leaves)))
    assert torch.equal(o, out) and all(torch.equal(got[k], grads[k]) for k in got)
    check(name, dict(got, out=o), ' (autograd)')
    xt = ts[0].transpose(1, 2).contiguous().transpose(1, 2).detach().requires_grad_(True)          # the same values, channel not fastest
    assert not xt.is_contiguous()
    flat = torch.zeros(ts[1].numel() + 1, device=device)                                           # starts off a 16-byte boundary
    flat[1:] = ts[1].reshape(-1)
    flat.requires_grad_(True)
    o2 = V.sr_reduce(xt, flat[1:].view(ts[1].shape), *leaves[2:], h, w, s, EPS)
    o2.backward(ts[5].transpose(1, 2).contiguous().transpose(1, 2))
    _sync(device)
    assert torch.equal(o2, out) and torch.equal(xt.grad, grads['dx']) and torch.equal(flat.grad[1:].view(ts[1].shape), grads['dw'])
    # only x requires grad (the weights frozen): still the same dx
    xg = ts[0].clone().requires_grad_(True)
    V.sr_reduce(xg, *ts[1:5], h, w, s, EPS).backward(ts[5])
    assert torch.equal(xg.grad, grads['dx'])


def run_call_counts(device, name='one'):
    shape = SHAPES[name]
    b, h, w, c, s = dims(shape)
    ts = on(device, shape)
    leaves = [t.clone().requires_grad_(True) for t in ts[:5]]
    with CallSpy(_lib.get(), NAMES_ABI) as spy:
        with torch.no_grad():
            o1 = V.sr_reduce(*leaves, h, w, s, EPS)
    assert spy.calls == {'cffm_sr_ln_fwd': 1, 'cffm_sr_ln_bwd_workspace_bytes': 0, 'cffm_sr_ln_bwd': 0}
    assert o1.grad_fn is None and not o1.requires_grad
    with CallSpy(_lib.get(), NAMES_ABI) as spy:
        o2 = V.sr_reduce(*ts[:5], h, w, s, EPS)          # nothing requires grad
    assert spy.calls['cffm_sr_ln_fwd'] == 1 and o2.grad_fn is None
    with CallSpy(_lib.get(), NAMES_ABI) as spy:
        o3 = V.sr_reduce(*leaves, h, w, s, EPS)
        assert len(o3.grad_fn.saved_tensors) == 5
        o3.backward(ts[5])
    assert spy.calls['cffm_sr_ln_fwd'] == 1 and spy.calls['cffm_sr_ln_bwd'] == 1
    _sync(device)
    assert torch.equal(o1, o3) and torch.equal(o2, o3)


def run_refusals(device):
    """every stated limit, null and misaligned pointers: non-zero with a message, and the NaN-prefilled outputs stay NaN"""
    lib = _lib.get()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4096, generator=g).to(device)
    wt = torch.randn(16384, generator=g).to(device)
    vec = torch.ones(1024, device=device)
    #        B, H, W, C, s, eps, x_off
    for b, h, w, c, s, eps, off in ((1, 6, 6, 32, 3, EPS, 0), (1, 4, 4, 32, 1, EPS, 0), (1, 16, 16, 16, 16, EPS, 0), (1, 4, 4, 24, 2, EPS, 0),
                                    (1, 2, 2, 528, 2, EPS, 0), (1, 4, 4, 0, 2, EPS, 0), (1, 3, 8, 32, 4, EPS, 0), (1, 8, 3, 32, 4, EPS, 0),
                                    (0, 4, 4, 32, 2, EPS, 0), (1, 4, 4, 32, 2, -1.0, 0), (1, 4, 4, 32, 2, float('inf'), 0),
                                    (1, 4, 4, 32, 2, EPS, 4)):
        outs = [torch.full((2048,), float('nan'), device=device) for _ in range(9)]
        out, z, stats, dx, dw, db, dgamma, dbeta, ws = outs
        args = (b, h, w, c, s, eps, _st(x))
        assert lib.cffm_sr_ln_fwd(_p(x, off), _p(wt), _p(vec), _p(vec), _p(vec), _p(out), _p(z), _p(stats), *args) != 0
        assert lib.cffm_last_error() != b''
        assert lib.cffm_sr_ln_bwd(_p(x, off), _p(wt), _p(vec), _p(vec), _p(vec), _p(vec), _p(dx), _p(dw), _p(db), _p(dgamma), _p(dbeta), _p(ws),
                                  *args) != 0
        assert lib.cffm_last_error() != b''
        _sync(device)
        assert all(bool(t.isnan().all()) for t in outs)
        if off == 0 and eps == EPS:
            assert lib.cffm_sr_ln_bwd_workspace_bytes(b, h, w, c, s) < 0
    out, z = torch.full((2048,), float('nan'), device=device), torch.full((2048,), float('nan'), device=device)
    ok = (1, 4, 4, 32, 2, EPS, _st(x))
    assert lib.cffm_sr_ln_fwd(_p(x), None, _p(vec), _p(vec), _p(vec), _p(out), None, None, *ok) != 0             # a null weight
    assert lib.cffm_sr_ln_fwd(_p(x), _p(wt), _p(vec), _p(vec), _p(vec), None, None, None, *ok) != 0             # a null out
    assert lib.cffm_sr_ln_fwd(_p(x), _p(wt), _p(vec), _p(vec), _p(vec), _p(out), _p(z), None, *ok) != 0         # z without stats
    assert lib.cffm_sr_ln_bwd(_p(x), _p(wt), _p(vec), _p(vec), _p(vec), _p(vec), _p(out), _p(z), _p(z), _p(z), _p(z), None, *ok) != 0   # no workspace
    _sync(device)
    assert bool(out.isnan().all()) and bool(z.isnan().all())
    assert lib.cffm_sr_ln_bwd_workspace_bytes(64, 1024, 1024, 32, 2) < 0          # B H W C = 2^31
    assert lib.cffm_sr_ln_bwd_workspace_bytes(1, 4, 4, 32, 2) > 0
    zz = lambda *s: torch.zeros(*s, device=device)
    good = lambda c=32, s=2: (zz(c, c, s, s), zz(c), zz(c), zz(c))
    with CallSpy(lib, NAMES_ABI) as spy:
        for bad in (lambda: V.sr_reduce(zz(1, 36, 32), *good(32, 3), 6, 6, 3),                        # s = 3
                    lambda: V.sr_reduce(zz(1, 16, 24), *good(24), 4, 4, 2),                           # C % 16
                    lambda: V.sr_reduce(zz(1, 4, 528), *good(528), 2, 2, 2),                          # C > 512
                    lambda: V.sr_reduce(zz(1, 24, 32), *good(32, 4), 3, 8, 4),                        # H < s
                    lambda: V.sr_reduce(zz(1, 16, 32), *good(), 4, 5, 2),                             # N != H W
                    lambda: V.sr_reduce(zz(1, 16, 32), *good(32, 4), 4, 4, 2),                        # weight of another s
                    lambda: V.sr_reduce(zz(1, 16, 32), zz(32, 32, 2, 2), zz(32), zz(32), zz(16), 4, 4, 2),
                    lambda: V.sr_reduce(zz(1, 16, 32).double(), *(t.double() for t in good()), 4, 4, 2),
                    lambda: V.sr_reduce(zz(1, 16, 32), zz(32, 32, 2, 2).double(), zz(32), zz(32), zz(32), 4, 4, 2),
                    lambda: V.sr_reduce(zz(1, 16, 32), *good(), 4, 4, 2, -1.0),                       # eps < 0
                    lambda: V.sr_reduce(zz(16, 32), *good(), 4, 4, 2)):
            with pytest.raises(_lib.CffmError):
                bad()
    assert spy.calls == {n: 0 for n in NAMES_ABI}


# ---------------------------------------------------------------------------------------------- emulator
def test_symbols_and_export():
    assert callable(V.sr_reduce)
    lib = emu.lib()
    header = open(emu.ROOT + '/include/cffm_hip.h').read()
    for n in NAMES_ABI:
        assert hasattr(lib, n) and n in _lib.SIGNATURES and n + '(' in header
    assert lib.cffm_abi_version() == 13


@pytest.mark.parametrize('name', NAMES)
def test_shapes_against_the_op_sequence(name):
    with emu.active():
        run_shape(torch.device('cpu'), name)


@pytest.mark.parametrize('name', ('rows', 'b0s1'))
def test_backward_is_deterministic(name):
    with emu.active():
        run_determinism(torch.device('cpu'), name)


def test_autograd_matches_the_direct_call():
    with emu.active():
        run_autograd(torch.device('cpu'))


def test_call_counts():
    with emu.active():
        run_call_counts(torch.device('cpu'))


def test_refusals_launch_nothing():
    with emu.active():
        run_refusals(torch.device('cpu'))


def test_no_cpu_fallback():
    """a CPU tensor without the emulator raises, GPU present or not (the model: tests/test_predict.py::test_no_cpu_fallback)"""
    with pytest.raises(_lib.CffmError):
        V.sr_reduce(torch.zeros(1, 16, 32), torch.zeros(32, 32, 2, 2), torch.zeros(32), torch.zeros(32), torch.zeros(32), 4, 4, 2)
