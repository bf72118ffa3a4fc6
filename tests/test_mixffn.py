"""The fused Mix-FFN middle (include/cffm_hip.h: cffm_dwconv_gelu_fwd / _bwd, vss_cffm_amd.dwconv_gelu) on the CPU through the fiber
emulator.  The GPU half is tests/test_mixffn_gpu.py and shares the run_*(device) bodies below.

The yardstick is the reference's op sequence (backbones/mix_transformer.py:48-55, 358-369): F.conv2d(groups=C, padding=1) on the NCHW
view, then F.gelu, in fp64 on the CPU.  Inputs from torch.Generator().manual_seed(0): h = 1.5 randn, w = 0.4 randn, b = 0.3 randn,
dout = randn.

Forward rule:  max|out - out64| <= 4 noise + 2.5e-7 max|u64|, noise = max|fp32 yardstick - fp64 yardstick| computed inside the test; the
second term is the Abramowitz & Stegun bound of gelu_erf (csrc/cffm_common.h) plus 1e-7 for the hardware reciprocal and exp2.
Gradient rule, for each t of dh, dw, db:  max|t - t64| <= 4 noise_t + 2.5e-7 A_t, where A_t is the largest element of the same fp64
backward evaluated with |dout| (1 + |u|), |w| and |h| in place of the signed values (what the approximation errors are multiplied by).

Measured through the emulator (error / gate):
    shape            out                  dh                   dw                   db
    (1,1,1,8)        6.95e-08 / 4.42e-07  1.36e-07 / 1.44e-06  2.89e-07 / 4.63e-06  2.45e-07 / 2.40e-06
    (2,5,7,36)       6.21e-07 / 4.06e-06  6.31e-07 / 7.08e-06  4.60e-06 / 8.18e-05  2.01e-06 / 5.17e-05
    (2,16,16,128)    1.04e-06 / 7.05e-06  1.07e-06 / 1.31e-05  1.13e-05 / 5.32e-04  5.59e-06 / 3.68e-04
    (1,3,40,260)     1.25e-06 / 7.17e-06  7.74e-07 / 1.23e-05  5.76e-06 / 2.16e-04  4.42e-06 / 1.28e-04
    (1,2,2,2048)     7.06e-07 / 6.14e-06  6.92e-07 / 7.05e-06  2.21e-06 / 2.64e-05  7.31e-07 / 9.46e-06
On the MI355X the largest error / gate over all shapes and tensors is 0.28 ((1,1,1,8) out: 1.23e-07 / 4.42e-07).
The yardstick noise of `out` at the five shapes: 4.98e-8, 5.15e-7, 1.13e-6, 1.25e-6, 1.07e-6.
"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import vss_cffm_amd as V
from tests import emu
from vss_cffm_amd import _lib

# (M, H, W, C): the smallest shapes at which each mechanism can go wrong
SHAPES = {
    'one': (1, 1, 1, 8),           # every neighbour is outside the image
    'odd': (2, 5, 7, 36),          # odd sizes; C below one wave's coverage and not a multiple of it; two images
    'b0s1': (2, 16, 16, 128),      # B0 stage 1 at a 64 x 64 input: two pixels per wave, more than one workgroup
    'wide': (1, 3, 40, 260),       # C over 256; H shorter than any y-strip; long rows
    'b1s4': (1, 2, 2, 2048),       # the widest hidden size, B1 stage 4
}
APPROX = 2.5e-7
NAMES = tuple(SHAPES)


# ---------------------------------------------------------------------------------------------- inputs and the yardstick
@functools.lru_cache(maxsize=None)
def make_inputs(shape):
    m, hh, ww, c = shape
    g = torch.Generator().manual_seed(0)
    h = 1.5 * torch.randn(m, hh * ww, c, generator=g)
    w = 0.4 * torch.randn(c, 1, 3, 3, generator=g)
    b = 0.3 * torch.randn(c, generator=g)
    dout = torch.randn(m, hh * ww, c, generator=g)
    return h, w, b, dout


def op_sequence(h, w, b, hh, ww):
    """the reference's op sequence in the dtype of h -> (out, u) as token rows"""
    m, n, c = h.shape
    u = F.conv2d(h.transpose(1, 2).reshape(m, c, hh, ww), w, b, padding=1, groups=c)
    return F.gelu(u).flatten(2).transpose(1, 2), u.flatten(2).transpose(1, 2)


def sequence_grads(h, w, b, dout, hh, ww):
    h, w, b = (t.detach().clone().requires_grad_(True) for t in (h, w, b))
    out, u = op_sequence(h, w, b, hh, ww)
    out.backward(dout)
    return out.detach(), u.detach(), {'dh': h.grad, 'dw': w.grad, 'db': b.grad}


class Yard:
    """fp64 yardstick of one shape, its distance to the fp32 one and the magnitudes A_t; computed once and left unchanged"""

    def __init__(self, shape):
        m, hh, ww, c = shape
        h, w, b, dout = make_inputs(shape)
        self.out, self.u, self.grads = sequence_grads(h.double(), w.double(), b.double(), dout.double(), hh, ww)
        out32, _, grads32 = sequence_grads(h, w, b, dout, hh, ww)
        self.noise = {'out': float((out32.double() - self.out).abs().max())}
        for k, v in grads32.items():
            self.noise[k] = float((v.double() - self.grads[k]).abs().max())
        # the linear part of the same backward with magnitudes: g -> |dout| (1 + |u|), w -> |w|, h -> |h|
        ha, wa, ba = (t.double().abs().requires_grad_(True) for t in (h, w, b))
        lin = F.conv2d(ha.transpose(1, 2).reshape(m, c, hh, ww), wa, ba, padding=1, groups=c).flatten(2).transpose(1, 2)
        lin.backward(dout.double().abs() * (1 + self.u.abs()))
        self.mag = {'out': float(self.u.abs().max()), 'dh': float(ha.grad.max()), 'dw': float(wa.grad.max()), 'db': float(ba.grad.max())}

    def gate(self, k):
        return 4 * self.noise[k] + APPROX * self.mag[k]


@functools.lru_cache(maxsize=None)
def yard(name):
    return Yard(SHAPES[name])


def check(name, got, tag=''):
    y = yard(name)
    want = dict(y.grads, out=y.out)
    for k, t in got.items():
        err = float((t.detach().cpu().double() - want[k]).abs().max())
        print('%s%s %s: max err %.3e (gate %.3e = 4 x noise %.3e + 2.5e-7 x %.3e), max|%s| %.3e'
              % (name, tag, k, err, y.gate(k), y.noise[k], y.mag[k], k, float(want[k].abs().max())))
        assert err <= y.gate(k), (name, k, err, y.gate(k))


# ---------------------------------------------------------------------------------------------- the C ABI, called directly
def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def _st(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def _sync(device):
    if device.type == 'cuda':
        torch.cuda.synchronize()


def raw_fwd(lib, h, w, b, out, dims, h_off=0):
    return lib.cffm_dwconv_gelu_fwd(_p(h, h_off), _p(w), _p(b), _p(out), *dims, _st(h))


def raw_bwd(lib, h, w, b, dout, dims, ws_fill=float('nan'), h_off=0):
    """-> (rc, dh, dw, db); the outputs and the workspace are pre-filled with NaN (or `ws_fill`)"""
    dh, dw, db = (torch.full_like(t, float('nan')) for t in (h, w, b))
    nbytes = lib.cffm_dwconv_gelu_bwd_workspace_bytes(*dims)
    ws = torch.full((max(nbytes, 16) // 4,), ws_fill, device=h.device)
    rc = lib.cffm_dwconv_gelu_bwd(_p(h, h_off), _p(w), _p(b), _p(dout), _p(dh), _p(dw), _p(db), _p(ws), *dims, _st(h))
    return rc, dh, dw, db


def on(device, shape):
    return tuple(t.to(device) for t in make_inputs(shape))


# ---------------------------------------------------------------------------------------------- bodies shared with the GPU half
def run_shape(device, name):
    lib = _lib.get()
    shape = SHAPES[name]
    h, w, b, dout = on(device, shape)
    out = torch.full_like(h, float('nan'))
    assert raw_fwd(lib, h, w, b, out, shape) == 0, lib.cffm_last_error()
    rc, dh, dw, db = raw_bwd(lib, h, w, b, dout, shape)
    assert rc == 0, lib.cffm_last_error()
    _sync(device)
    check(name, {'out': out, 'dh': dh, 'dw': dw, 'db': db})
    return out, dh, dw, db


def run_no_leak(device):
    """image 0 of h and of dout all NaN: the out and dh of image 1 are the bits of the one-image call"""
    lib = _lib.get()
    m, hh, ww, c = SHAPES['odd']
    h, w, b, dout = on(device, SHAPES['odd'])
    h, dout = h.clone(), dout.clone()
    h[0], dout[0] = float('nan'), float('nan')
    out = torch.empty_like(h)
    assert raw_fwd(lib, h, w, b, out, (m, hh, ww, c)) == 0
    rc, dh, _, _ = raw_bwd(lib, h, w, b, dout, (m, hh, ww, c))
    assert rc == 0
    h1, d1 = h[1:].contiguous(), dout[1:].contiguous()
    out1 = torch.empty_like(h1)
    assert raw_fwd(lib, h1, w, b, out1, (1, hh, ww, c)) == 0
    rc, dh1, _, _ = raw_bwd(lib, h1, w, b, d1, (1, hh, ww, c))
    assert rc == 0
    _sync(device)
    assert bool(out[0].isnan().all()) and not bool(out1.isnan().any()) and not bool(dh1.isnan().any())
    assert torch.equal(out[1:], out1) and torch.equal(dh[1:], dh1)


def run_poison_and_determinism(device, name='b0s1'):
    """a NaN-filled, a zero-filled and a second NaN-filled workspace: the same bits of dh, dw and db"""
    lib = _lib.get()
    shape = SHAPES[name]
    h, w, b, dout = on(device, shape)
    runs = [raw_bwd(lib, h, w, b, dout, shape, fill) for fill in (float('nan'), 0.0, float('nan'))]
    _sync(device)
    for rc, dh, dw, db in runs:
        assert rc == 0 and not bool(dh.isnan().any()) and not bool(dw.isnan().any()) and not bool(db.isnan().any())
        assert torch.equal(dh, runs[0][1]) and torch.equal(dw, runs[0][2]) and torch.equal(db, runs[0][3])


def run_errors(device):
    """C = 6, C = 2, H = 0, a misaligned pointer: non-zero, and the NaN-prefilled outputs stay NaN"""
    lib = _lib.get()
    for m, hh, ww, c, off in ((1, 2, 2, 6, 0), (1, 2, 2, 2, 0), (1, 0, 2, 8, 0), (1, 2, 2, 8, 4)):
        n = max(1, m * hh * ww * c)
        g = torch.Generator().manual_seed(1)
        h = torch.randn(1, 1, n + 4, generator=g).to(device)
        w, b, dout = torch.randn(max(c, 4), 1, 3, 3, generator=g).to(device), torch.randn(max(c, 4), generator=g).to(device), torch.ones_like(h)
        out = torch.full_like(h, float('nan'))
        assert raw_fwd(lib, h, w, b, out, (m, hh, ww, c), h_off=off) != 0
        assert lib.cffm_last_error() != b''
        rc, dh, dw, db = raw_bwd(lib, h, w, b, dout, (m, hh, ww, c), h_off=off)
        assert rc != 0
        _sync(device)
        assert all(bool(t.isnan().all()) for t in (out, dh, dw, db))
    assert lib.cffm_dwconv_gelu_bwd_workspace_bytes(1, 2, 2, 6) < 0 and lib.cffm_dwconv_gelu_bwd_workspace_bytes(1, 2, 0, 8) < 0
    assert lib.cffm_dwconv_gelu_bwd_workspace_bytes(2, 32768, 32768, 4) < 0         # M H W C = 2^33
    x = torch.zeros(1, 4, 8, device=device)
    for bad in (lambda: V.dwconv_gelu(x, torch.zeros(8, 1, 3, 3, device=device), torch.zeros(8, device=device), 2, 3),
                lambda: V.dwconv_gelu(x, torch.zeros(8, 3, 3, device=device), torch.zeros(8, device=device), 2, 2),
                lambda: V.dwconv_gelu(x.double(), torch.zeros(8, 1, 3, 3, device=device), torch.zeros(8, device=device), 2, 2),
                lambda: V.dwconv_gelu(x[0], torch.zeros(8, 1, 3, 3, device=device), torch.zeros(8, device=device), 2, 2),
                lambda: V.dwconv_gelu(torch.zeros(1, 4, 6, device=device), torch.zeros(6, 1, 3, 3, device=device), torch.zeros(6, device=device), 2, 2)):
        with pytest.raises(_lib.CffmError):
            bad()


class CallSpy:
    """counts the calls of some entry points made through the binding"""

    def __init__(self, lib, names):
        self.lib, self.real, self.calls = lib, {n: getattr(lib, n) for n in names}, {n: 0 for n in names}

    def __enter__(self):
        for n, fn in self.real.items():
            def spied(*a, _n=n, _fn=fn):
                self.calls[_n] += 1
                return _fn(*a)
            setattr(self.lib, n, spied)
        return self

    def __exit__(self, *exc):
        for n, fn in self.real.items():
            setattr(self.lib, n, fn)


def run_autograd(device, name='odd'):
    """dwconv_gelu(...).backward against the op sequence's autograd (the fp64 yardstick) under the gradient rule; a non-contiguous h
    gives the same bits; under no_grad only the forward runs"""
    m, hh, ww, c = SHAPES[name]
    h, w, b, dout = on(device, SHAPES[name])
    hg, wg, bg = (t.clone().requires_grad_(True) for t in (h, w, b))
    out = V.dwconv_gelu(hg, wg, bg, hh, ww)
    out.backward(dout)
    check(name, {'out': out, 'dh': hg.grad, 'dw': wg.grad, 'db': bg.grad}, ' (autograd)')
    ht = h.transpose(1, 2).contiguous().transpose(1, 2)          # the same values, channel not fastest
    assert not ht.is_contiguous() or m * hh * ww == 1 or c == 1
    h2 = ht.detach().requires_grad_(True)
    out2 = V.dwconv_gelu(h2, w, b, hh, ww)
    out2.backward(dout.transpose(1, 2).contiguous().transpose(1, 2))
    assert torch.equal(out2, out) and torch.equal(h2.grad, hg.grad)
    with CallSpy(_lib.get(), ('cffm_dwconv_gelu_fwd', 'cffm_dwconv_gelu_bwd_workspace_bytes', 'cffm_dwconv_gelu_bwd')) as spy:
        with torch.no_grad():
            out3 = V.dwconv_gelu(hg, wg, bg, hh, ww)
    assert spy.calls == {'cffm_dwconv_gelu_fwd': 1, 'cffm_dwconv_gelu_bwd_workspace_bytes': 0, 'cffm_dwconv_gelu_bwd': 0}
    assert out3.grad_fn is None and not out3.requires_grad and torch.equal(out3, out)


# ---------------------------------------------------------------------------------------------- emulator
def test_symbols_and_export():
    assert callable(V.dwconv_gelu)
    lib = emu.lib()
    for n in ('cffm_dwconv_gelu_fwd', 'cffm_dwconv_gelu_bwd_workspace_bytes', 'cffm_dwconv_gelu_bwd'):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.cffm_abi_version() == 13


@pytest.mark.parametrize('name', NAMES)
def test_shapes_against_the_op_sequence(name):
    with emu.active():
        run_shape(torch.device('cpu'), name)


def test_nothing_leaks_across_images():
    with emu.active():
        run_no_leak(torch.device('cpu'))


def test_poisoned_workspace_and_determinism():
    with emu.active():
        run_poison_and_determinism(torch.device('cpu'))
        run_poison_and_determinism(torch.device('cpu'), 'wide')


def test_errors_leave_the_outputs_untouched():
    with emu.active():
        run_errors(torch.device('cpu'))


def test_autograd_and_no_grad():
    with emu.active():
        run_autograd(torch.device('cpu'))


def test_no_cpu_fallback():
    """a CPU tensor without the emulator raises, GPU present or not (the model: tests/test_predict.py::test_no_cpu_fallback)"""
    with pytest.raises(_lib.CffmError):
        V.dwconv_gelu(torch.zeros(1, 4, 8), torch.zeros(8, 1, 3, 3), torch.zeros(8), 2, 2)
