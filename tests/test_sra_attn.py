"""The fused spatial-reduction attention core (include/cffm_hip.h: cffm_sra_attn_fwd / _bwd, vss_cffm_amd.sra_attention) on the CPU through
the fiber emulator.  The GPU half is tests/test_sra_attn_gpu.py and shares the run_*(device) bodies below.

The yardstick is the reference's op sequence (backbones/mix_transformer.py Attention.forward: reshape / permute, q @ k^T, * scale, softmax,
attn @ v, transpose / reshape) on q [B,N,C] and kv [B,Nk,2C], in fp64 on the CPU.  Inputs from torch.Generator().manual_seed(0), drawn in
this order: q = qs randn(B,N,C), kv = randn(B,Nk,2C), dout = randn(B,N,C); scale = hd ** -0.5.

Rule, for each t of out, dq, dkv:  max|t - t64| <= 4 noise_t + 2.5e-7 A_t, noise_t = max|fp32 op sequence - fp64 op sequence| computed
inside the test; A_out = max|v|; A_dq, A_dkv = the largest elements of the same fp64 backward evaluated with |q|, |k|, |v|, |dout| in place
of the signed values and the true probabilities (the second term covers the hardware exp2 and reciprocal; for `one` it is the whole gate:
out == v and dq == 0).  lse against the fp64 logsumexp under the rule of `out` with A = 1.

Measured through the emulator (error / gate):
    shape    out                  lse                  dq                   dkv
    one      0.00e+00 / 6.42e-07  2.23e-09 / 2.50e-07  0.00e+00 / 5.36e-22  0.00e+00 / 6.53e-07
    b0s3     3.37e-07 / 2.92e-06  5.29e-07 / 2.25e-06  7.77e-07 / 2.08e-06  1.40e-06 / 4.59e-06
    b0s4     2.42e-07 / 2.19e-06  2.44e-07 / 1.41e-06  5.51e-07 / 1.94e-06  8.66e-07 / 2.68e-06
    odd      7.03e-07 / 3.15e-06  2.73e-07 / 2.32e-06  7.36e-07 / 3.10e-06  7.73e-07 / 4.18e-06
    k225     1.89e-07 / 2.12e-06  3.32e-07 / 1.29e-06  3.36e-07 / 1.34e-06  2.91e-07 / 1.03e-06
    k405     2.84e-07 / 1.84e-06  3.84e-07 / 1.00e-06  3.24e-07 / 1.02e-06  3.24e-07 / 1.52e-06
    hot      1.51e-05 / 4.37e-05  1.49e-05 / 4.29e-05  1.11e-05 / 2.76e-05  2.03e-04 / 5.35e-04
    n4100    7.76e-07 / 4.76e-06  1.07e-06 / 4.30e-06  1.93e-06 / 4.78e-06  2.18e-05 / 4.32e-04
On the MI355X (error / gate):
    one      0.00e+00 / 6.42e-07  2.23e-09 / 2.50e-07  0.00e+00 / 5.36e-22  0.00e+00 / 6.53e-07
    b0s3     3.06e-07 / 2.92e-06  5.29e-07 / 2.25e-06  7.77e-07 / 2.08e-06  1.40e-06 / 6.34e-06
    b0s4     2.42e-07 / 2.40e-06  2.44e-07 / 1.63e-06  5.51e-07 / 1.75e-06  8.66e-07 / 2.73e-06
    odd      6.43e-07 / 3.15e-06  2.56e-07 / 2.32e-06  6.33e-07 / 3.10e-06  7.16e-07 / 4.18e-06
    k225     1.89e-07 / 2.00e-06  2.91e-07 / 1.16e-06  3.36e-07 / 1.28e-06  2.91e-07 / 1.03e-06
    k405     2.84e-07 / 1.84e-06  3.84e-07 / 1.00e-06  3.43e-07 / 1.07e-06  4.29e-07 / 1.52e-06
    hot      1.51e-05 / 4.37e-05  1.49e-05 / 4.29e-05  1.11e-05 / 2.76e-05  2.03e-04 / 5.35e-04
    n4100    7.76e-07 / 2.35e-06  1.07e-06 / 1.89e-06  1.93e-06 / 4.00e-06  1.80e-05 / 8.38e-04
(the gates differ a little between the two tables: the fp32 yardstick, whose noise sets them, runs on the CPU of the machine.)
"""
import ctypes as C
import functools

import pytest
import torch

import vss_cffm_amd as V
from tests import emu
from tests.test_mixffn import CallSpy
from vss_cffm_amd import _lib

# (B, heads, N, Nk, hd, qs): the smallest shapes at which each mechanism can go wrong
SHAPES = {
    'one': (1, 1, 1, 1, 32, 1),           # one query, one key: out == v, dq == 0
    'b0s3': (2, 5, 16, 4, 32, 1),         # B0 stage 3 at 64 x 64: keys below one tile, 5 heads (C = 160), two images
    'b0s4': (1, 8, 4, 4, 32, 1),          # fewer queries than a tile, 8 heads
    'odd': (1, 2, 37, 19, 64, 1),         # hd = 64; query and key tails not multiples of 16 or 4
    'k225': (1, 1, 80, 225, 64, 1),       # the workload's key count: 14 full key tiles + 1 key, online rescale across tiles
    'k405': (1, 2, 130, 405, 32, 1),      # evaluation key count with hd = 32; more keys than one LDS stage holds
    'hot': (1, 2, 37, 19, 64, 30),        # max|score| = 118 > 88.7: exp overflows fp32 without the running-max subtraction
    'n4100': (1, 1, 4100, 3, 32, 1),      # many query chunks per head (the ordered dk / dv reduction), Nk below one MFMA k-step
}
APPROX = 2.5e-7
NAMES = tuple(SHAPES)
GUARD = 8           # words past the end of every output


# ---------------------------------------------------------------------------------------------- inputs and the yardstick
@functools.lru_cache(maxsize=None)
def make_inputs(shape):
    b, heads, n, nk, hd, qs = shape
    c = heads * hd
    g = torch.Generator().manual_seed(0)
    q = qs * torch.randn(b, n, c, generator=g)
    kv = torch.randn(b, nk, 2 * c, generator=g)
    dout = torch.randn(b, n, c, generator=g)
    return q, kv, dout


def heads_view(q, kv, heads):
    b, n, c = q.shape
    hd = c // heads
    qh = q.reshape(b, n, heads, hd).permute(0, 2, 1, 3)
    k, v = kv.reshape(b, -1, 2, heads, hd).permute(2, 0, 3, 1, 4)
    return qh, k, v


def op_sequence(q, kv, heads, scale):
    """the reference's attention lines in the dtype of q -> (out [B,N,C], lse [B,heads,N], attn [B,heads,N,Nk])"""
    b, n, c = q.shape
    qh, k, v = heads_view(q, kv, heads)
    s = (qh @ k.transpose(-2, -1)) * scale
    attn = s.softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(b, n, c), torch.logsumexp(s, dim=-1), attn


def sequence_grads(q, kv, dout, heads, scale):
    q, kv = (t.detach().clone().requires_grad_(True) for t in (q, kv))
    out, lse, attn = op_sequence(q, kv, heads, scale)
    out.backward(dout)
    return {'out': out.detach(), 'lse': lse.detach(), 'dq': q.grad, 'dkv': kv.grad}, attn.detach()


class Yard:
    """fp64 yardstick of one shape, its distance to the fp32 one and the magnitudes A_t; computed once and left unchanged"""

    def __init__(self, shape):
        b, heads, n, nk, hd, qs = shape
        self.scale = hd ** -0.5
        q, kv, dout = make_inputs(shape)
        self.want, p = sequence_grads(q.double(), kv.double(), dout.double(), heads, self.scale)
        got32, _ = sequence_grads(q, kv, dout, heads, self.scale)
        self.noise = {k: float((got32[k].double() - self.want[k]).abs().max()) for k in ('out', 'dq', 'dkv')}
        self.noise['lse'] = self.noise['out']
        # the same backward with magnitudes and the true probabilities
        qa, ka, va = heads_view(q.double().abs(), kv.double().abs(), heads)
        da = dout.double().abs().reshape(b, n, heads, hd).permute(0, 2, 1, 3)
        dv = p.transpose(-2, -1) @ da
        ds = p * (da @ va.transpose(-2, -1) - (da * (p @ va)).sum(-1, keepdim=True))
        dq, dk = self.scale * (ds @ ka), self.scale * (ds.transpose(-2, -1) @ qa)
        self.mag = {'out': float(va.max()), 'lse': 1.0, 'dq': float(dq.abs().max()), 'dkv': float(max(dk.abs().max(), dv.abs().max()))}

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


# ---------------------------------------------------------------------------------------------- the C ABI, called directly
def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else C.c_void_p(0)


def _st(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def _sync(device):
    if device.type == 'cuda':
        torch.cuda.synchronize()


def dims(shape):
    b, heads, n, nk, hd, _ = shape
    return b, n, nk, heads, hd


def guarded(shape, device, fill=float('nan')):
    """a `fill`-filled tensor of `shape` whose storage goes on for GUARD words holding 12345 -> (tensor, guard words)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), fill, device=device)
    buf[n:] = 12345.0
    return buf[:n].view(shape), buf[n:]


def raw_fwd(lib, q, kv, shape, with_lse=True, q_off=0):
    """-> (rc, out, lse, guards); out and lse pre-filled with NaN"""
    b, n, nk, heads, hd = dims(shape)
    out, g0 = guarded((b, n, heads * hd), q.device)
    lse, g1 = guarded((b, heads, n), q.device)
    rc = lib.cffm_sra_attn_fwd(_p(q, q_off), _p(kv), _p(out), _p(lse if with_lse else None), b, n, nk, heads, hd, hd ** -0.5, _st(q))
    return rc, out, lse, (g0, g1)


def raw_bwd(lib, q, kv, out, lse, dout, shape, ws_fill=float('nan'), q_off=0):
    """-> (rc, dq, dkv, guards); the outputs and the workspace are pre-filled with NaN (or `ws_fill`)"""
    b, n, nk, heads, hd = dims(shape)
    dq, g0 = guarded(tuple(q.shape), q.device)
    dkv, g1 = guarded(tuple(kv.shape), q.device)
    nbytes = lib.cffm_sra_attn_bwd_workspace_bytes(b, n, nk, heads, hd)
    ws, g2 = guarded((max(nbytes, 16) // 4,), q.device, ws_fill)
    rc = lib.cffm_sra_attn_bwd(_p(q, q_off), _p(kv), _p(out), _p(lse), _p(dout), _p(dq), _p(dkv), _p(ws), b, n, nk, heads, hd, hd ** -0.5, _st(q))
    return rc, dq, dkv, (g0, g1, g2)


def on(device, shape):
    return tuple(t.to(device) for t in make_inputs(shape))


def guards_intact(guards):
    return all(bool((g == 12345.0).all()) for g in guards)


# ---------------------------------------------------------------------------------------------- bodies shared with the GPU half
def run_shape(device, name):
    """forward with and without lse, backward; NaN-poisoned outputs and workspace, guard words; everything against the yardstick"""
    lib = _lib.get()
    shape = SHAPES[name]
    q, kv, dout = on(device, shape)
    rc, out, lse, gf = raw_fwd(lib, q, kv, shape)
    assert rc == 0, lib.cffm_last_error()
    rc, out2, lse2, gf2 = raw_fwd(lib, q, kv, shape, with_lse=False)
    assert rc == 0, lib.cffm_last_error()
    rc, dq, dkv, gb = raw_bwd(lib, q, kv, out, lse, dout, shape)
    assert rc == 0, lib.cffm_last_error()
    _sync(device)
    assert guards_intact(gf + gf2 + gb)
    assert torch.equal(out2, out) and bool(lse2.isnan().all())
    c = q.shape[2]
    assert bool(dkv[..., :c].isfinite().all()) and bool(dkv[..., c:].isfinite().all())
    check(name, {'out': out, 'lse': lse, 'dq': dq, 'dkv': dkv})
    if name == 'one':
        assert torch.equal(out, kv[:, :, c:]) and not bool(dq.any())
    return out, lse, dq, dkv


def run_determinism(device, name):
    """a NaN-filled, a zero-filled and a second NaN-filled workspace: the same bits of dq and dkv"""
    lib = _lib.get()
    shape = SHAPES[name]
    q, kv, dout = on(device, shape)
    rc, out, lse, _ = raw_fwd(lib, q, kv, shape)
    assert rc == 0
    runs = [raw_bwd(lib, q, kv, out, lse, dout, shape, fill) for fill in (float('nan'), 0.0, float('nan'))]
    _sync(device)
    for rc, dq, dkv, g in runs:
        assert rc == 0 and guards_intact(g) and bool(dq.isfinite().all()) and bool(dkv.isfinite().all())
        assert torch.equal(dq, runs[0][1]) and torch.equal(dkv, runs[0][2])


def run_autograd(device, name='odd'):
    """sra_attention(...).backward gives the tensors of the direct call; so do a non-contiguous q and a kv sliced out of a larger buffer"""
    lib = _lib.get()
    shape = SHAPES[name]
    b, n, nk, heads, hd = dims(shape)
    q, kv, dout = on(device, shape)
    rc, out, lse, _ = raw_fwd(lib, q, kv, shape)
    assert rc == 0
    rc, dq, dkv, _ = raw_bwd(lib, q, kv, out, lse, dout, shape)
    assert rc == 0
    qg, kvg = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    o = V.sra_attention(qg, kvg, heads, hd ** -0.5)
    o.backward(dout)
    _sync(device)
    assert torch.equal(o, out) and torch.equal(qg.grad, dq) and torch.equal(kvg.grad, dkv)
    check(name, {'out': o, 'dq': qg.grad, 'dkv': kvg.grad}, ' (autograd)')
    qt = q.transpose(1, 2).contiguous().transpose(1, 2).detach().requires_grad_(True)          # the same values, channel not fastest
    assert not qt.is_contiguous()
    big = torch.zeros(b, nk + 3, 2 * heads * hd + 8, device=device)
    big[:, 1:nk + 1, 4:-4] = kv
    big.requires_grad_(True)
    o2 = V.sra_attention(qt, big[:, 1:nk + 1, 4:-4], heads, hd ** -0.5)
    o2.backward(dout.transpose(1, 2).contiguous().transpose(1, 2))
    _sync(device)
    assert torch.equal(o2, out) and torch.equal(qt.grad, dq) and torch.equal(big.grad[:, 1:nk + 1, 4:-4], dkv)
    assert not bool(big.grad[:, 0].any()) and not bool(big.grad[..., :4].any())
    # a contiguous slice that starts off a 16-byte boundary
    flat = torch.zeros(kv.numel() + 1, device=device)
    flat[1:] = kv.reshape(-1)
    o3 = V.sra_attention(q, flat[1:].view(kv.shape), heads, hd ** -0.5)
    assert torch.equal(o3, out)


NAMES_ABI = ('cffm_sra_attn_fwd', 'cffm_sra_attn_bwd_workspace_bytes', 'cffm_sra_attn_bwd')


def run_call_counts(device, name='b0s3'):
    shape = SHAPES[name]
    b, n, nk, heads, hd = dims(shape)
    q, kv, dout = on(device, shape)
    qg, kvg = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    with CallSpy(_lib.get(), NAMES_ABI) as spy:
        with torch.no_grad():
            o1 = V.sra_attention(qg, kvg, heads, hd ** -0.5)
    assert spy.calls == {'cffm_sra_attn_fwd': 1, 'cffm_sra_attn_bwd_workspace_bytes': 0, 'cffm_sra_attn_bwd': 0}
    assert o1.grad_fn is None and not o1.requires_grad
    with CallSpy(_lib.get(), NAMES_ABI) as spy:
        o2 = V.sra_attention(q, kv, heads, hd ** -0.5)          # nothing requires grad
    assert spy.calls['cffm_sra_attn_fwd'] == 1 and o2.grad_fn is None
    with CallSpy(_lib.get(), NAMES_ABI) as spy:
        o3 = V.sra_attention(qg, kvg, heads, hd ** -0.5)
        o3.backward(dout)
    assert spy.calls['cffm_sra_attn_fwd'] == 1 and spy.calls['cffm_sra_attn_bwd'] == 1
    _sync(device)
    assert torch.equal(o1, o3) and torch.equal(o2, o3)


def run_refusals(device):
    """bad sizes, a bad head size, null and misaligned pointers: non-zero with a message, and the NaN-prefilled outputs stay NaN"""
    lib = _lib.get()
    g = torch.Generator().manual_seed(1)
    q, kv = torch.randn(1, 8, 200, generator=g).to(device), torch.randn(1, 8, 400, generator=g).to(device)
    dout = torch.ones_like(q)
    #        B, heads, N, Nk, hd, q_off
    for b, heads, n, nk, hd, off in ((1, 2, 4, 4, 48, 0), (1, 1, 0, 4, 32, 0), (1, 1, 4, 0, 32, 0), (0, 1, 4, 4, 32, 0), (1, 0, 4, 4, 32, 0),
                                     (1, 1, 4, 4, 32, 4)):
        shape = (max(b, 1), max(heads, 1), max(n, 1), max(nk, 1), hd, 1)
        out, _ = guarded((shape[0], shape[2], shape[1] * hd), device)
        lse, _ = guarded((shape[0], shape[1], shape[2]), device)
        dq, dkv, ws = torch.full_like(q, float('nan')), torch.full_like(kv, float('nan')), torch.full((4096,), float('nan'), device=device)
        args = (b, n, nk, heads, hd, hd ** -0.5, _st(q))
        assert lib.cffm_sra_attn_fwd(_p(q, off), _p(kv), _p(out), _p(lse), *args) != 0
        assert lib.cffm_last_error() != b''
        assert lib.cffm_sra_attn_bwd(_p(q, off), _p(kv), _p(out), _p(lse), _p(dout), _p(dq), _p(dkv), _p(ws), *args) != 0
        assert lib.cffm_last_error() != b''
        _sync(device)
        assert all(bool(t.isnan().all()) for t in (out, lse, dq, dkv, ws))
        if off == 0:
            assert lib.cffm_sra_attn_bwd_workspace_bytes(b, n, nk, heads, hd) < 0
    out = torch.full_like(q, float('nan'))
    assert lib.cffm_sra_attn_fwd(_p(q), None, _p(out), None, 1, 4, 4, 1, 32, 32 ** -0.5, _st(q)) != 0            # a null kv
    assert lib.cffm_sra_attn_fwd(_p(q), _p(kv), _p(out), None, 1, 4, 4, 1, 32, -1.0, _st(q)) != 0               # a scale that is not positive
    _sync(device)
    assert bool(out.isnan().all())
    assert lib.cffm_sra_attn_bwd_workspace_bytes(8, 1 << 20, 4, 8, 64) < 0          # B N C = 2^32
    assert lib.cffm_sra_attn_bwd_workspace_bytes(8, 4, 1 << 19, 8, 64) < 0          # B Nk 2C = 2^32
    assert lib.cffm_sra_attn_bwd_workspace_bytes(1, 16, 4, 2, 32) > 0
    z = lambda *s: torch.zeros(*s, device=device)
    with CallSpy(lib, NAMES_ABI) as spy:
        for bad in (lambda: V.sra_attention(z(1, 4, 96), z(1, 4, 192), 2, 1.0),             # hd = 48
                    lambda: V.sra_attention(z(1, 4, 64), z(1, 4, 128), 3, 1.0),             # heads * hd != C
                    lambda: V.sra_attention(z(1, 4, 64), z(1, 4, 64), 2, 1.0),              # kv width != 2C
                    lambda: V.sra_attention(z(2, 4, 64), z(1, 4, 128), 2, 1.0),             # mismatched batch
                    lambda: V.sra_attention(z(1, 4, 64).double(), z(1, 4, 128).double(), 2, 1.0),
                    lambda: V.sra_attention(z(1, 4, 64).long(), z(1, 4, 128).long(), 2, 1.0),
                    lambda: V.sra_attention(z(1, 4, 64), z(1, 4, 128).double(), 2, 1.0),
                    lambda: V.sra_attention(z(1, 0, 64), z(1, 4, 128), 2, 1.0),             # N = 0
                    lambda: V.sra_attention(z(1, 4, 64), z(1, 0, 128), 2, 1.0),
                    lambda: V.sra_attention(z(4, 64), z(4, 128), 2, 1.0)):
            with pytest.raises(_lib.CffmError):
                bad()
    assert spy.calls == {n: 0 for n in NAMES_ABI}


# ---------------------------------------------------------------------------------------------- emulator
def test_symbols_and_export():
    assert callable(V.sra_attention)
    lib = emu.lib()
    header = open(emu.ROOT + '/include/cffm_hip.h').read()
    for n in NAMES_ABI:
        assert hasattr(lib, n) and n in _lib.SIGNATURES and n + '(' in header
    assert lib.cffm_abi_version() == 13


@pytest.mark.parametrize('name', NAMES)
def test_shapes_against_the_op_sequence(name):
    with emu.active():
        run_shape(torch.device('cpu'), name)


@pytest.mark.parametrize('name', ('n4100', 'k225'))
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
        V.sra_attention(torch.zeros(1, 4, 64), torch.zeros(1, 4, 128), 2, 1.0)
