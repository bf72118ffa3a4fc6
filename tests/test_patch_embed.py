"""MiT's overlapping patch embedding as a kernel (cffm_patch_embed_fwd, csrc/pembed_kernels.h) and n consecutive stages per library call
(cffm_mit_infer, MixVisionTransformer.embed_impl = 'hip' on top of stage_impl = 'hip'), on the CPU through the fiber emulator.  The GPU
half is tests/test_patch_embed_gpu.py and shares the run_*(device) bodies below.

Gate: the yardstick of tests/test_mit_stage.py, extended to the convolution.  Reference: the 'torch' path in fp64.  Yardstick: the same path
in fp64 with every patch_embed*.proj replaced by conv(x_hi, w_hi) + conv(x_hi, w_lo) + conv(x_lo, w_hi) + bias of bf16-split operands (only
those convolutions: the depthwise and `sr` kernels are exact) and, at stage and model level, F.linear replaced by split_linear.  The gate
per tensor is 4 x dist(yardstick, fp64) + 2^-23 x max|fp64|.  Every test prints error / gate per tensor.

Largest error / gate measured (the same figures are in DESIGN.md section 3t):
    through the emulator (CPU):  the kernel alone 0.262 (k3_2x64x12x9_160+30);  one stage per call 0.280 (d320s2);  mit_b0 96x72 0.279 (out3)
    on the MI355X:               the kernel alone 0.258 (k3_2x64x12x9_160+30);  one stage per call 0.261 (d160s2);  mit_b0 96x72 0.271 (out0);
                                 mit_b1 on [2,3,96,128] against fp64 on the CPU 0.288 (out3)
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import vss_cffm_amd as V
from oracle import recipe as R
from tests import emu
from tests import test_backbone as TB
from tests import test_mit_stage as TS
from tests.test_mit_stage import STAGES, dist, make_stage, report, split_linears
from tests.test_mixffn import CallSpy
from vss_cffm_amd import _lib, ops
from vss_cffm_amd import backbone as B

CPU = torch.device('cpu')
MARGIN = 4.0
ULP = 2.0 ** -23
# (k, stride), input (B, Cin, H, W), Cout, what is added to the convolution's bias
KERNEL_CASES = {
    'k7_1x3x32x32_32': ((7, 4), (1, 3, 32, 32), 32, 0.0),
    'k7_2x3x68x76_64': ((7, 4), (2, 3, 68, 76), 64, 0.0),            # 17 x 19 map
    'k7_1x3x30x27_32': ((7, 4), (1, 3, 30, 27), 32, 0.0),            # sizes that are no multiple of the stride
    'k3_2x64x18x22_128': ((3, 2), (2, 64, 18, 22), 128, 0.0),
    'k3_2x64x12x9_160': ((3, 2), (2, 64, 12, 9), 160, 0.0),          # odd W, 40-lane rows
    'k3_2x128x10x14_320': ((3, 2), (2, 128, 10, 14), 320, 0.0),
    'k3_2x320x5x6_512': ((3, 2), (2, 320, 5, 6), 512, 0.0),          # K = 2880, 3 x 3 map
    'k3_1x32x1x1_64': ((3, 2), (1, 32, 1, 1), 64, 0.0),              # one pixel, eight taps in the padding
    'k3_1x256x7x7_16': ((3, 2), (1, 256, 7, 7), 16, 0.0),            # narrowest row
    'k3_2x64x12x9_160+30': ((3, 2), (2, 64, 12, 9), 160, 30.0),      # rows with |mean| >> std: the case E[z^2] - mean^2 fails
}
SPY = ('cffm_mit_infer', 'cffm_mit_stage_infer', 'cffm_patch_embed_fwd')


@contextlib.contextmanager
def impls(stage, embed):
    prev = B.MixVisionTransformer.stage_impl, B.MixVisionTransformer.embed_impl
    B.MixVisionTransformer.stage_impl, B.MixVisionTransformer.embed_impl = stage, embed
    try:
        yield
    finally:
        B.MixVisionTransformer.stage_impl, B.MixVisionTransformer.embed_impl = prev


# ---------------------------------------------------------------------------------------------- the yardstick
def split_conv(conv, x):
    xh, xl = TS._split(x)
    wh, wl = TS._split(conv.weight)
    kw = dict(stride=conv.stride, padding=conv.padding, dilation=conv.dilation, groups=conv.groups)
    y = F.conv2d(xh, wh, **kw) + F.conv2d(xh, wl, **kw) + F.conv2d(xl, wh, **kw)
    return y if conv.bias is None else y + conv.bias.view(1, -1, 1, 1)


@contextlib.contextmanager
def split_convs(convs):
    """the forward of these Conv2d modules -> the three products of their bf16-split operands"""
    convs = list(convs)
    for c in convs:
        c.forward = functools.partial(split_conv, c)
    try:
        yield
    finally:
        for c in convs:
            del c.forward


def embed_convs(m):
    return [getattr(m, 'patch_embed%d' % i).proj for i in range(1, 5)]


def gate_of(yard, want):
    return MARGIN * dist(yard, want) + ULP * float(want.detach().abs().max())


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
def make_embed(name, dtype=torch.float32):
    (k, s), shape, cout, shift = KERNEL_CASES[name]
    m = B.OverlapPatchEmbed(img_size=64, patch_size=k, stride=s, in_chans=shape[1], embed_dim=cout)
    m.load_state_dict(R.synth_state(m, seed=60), strict=True)
    with torch.no_grad():
        m.proj.bias += shift
        m.norm.weight.mul_(4.0).add_(1.0)          # gamma = 1 + 0.2 N(0, 1)
    return m.to(dtype).eval()


@functools.lru_cache(maxsize=None)
def kernel_case(name):
    """input, fp64 rows of the module's own forward, (Ho, Wo) and the yardstick gate"""
    x = R.synth_input('pembed_x', KERNEL_CASES[name][1], seed=61, scale=1.0)
    m = make_embed(name, torch.float64)
    with torch.no_grad():
        want, ho, wo = m(x.double())
        with split_convs([m.proj]):
            yard = m(x.double())[0]
    return x, want, (ho, wo), gate_of(yard, want)


def run_kernel(device, name):
    x, want, hw, gate = kernel_case(name)
    m = make_embed(name).to(device)
    xd = x.to(device)
    got = []
    with torch.no_grad():
        def call(out):
            res, ho, wo = V.patch_embed(xd, m.proj, m.norm, out=out)
            got.append((ho, wo))
            return res
        out = TS._twice(call, want.shape, device)
    assert got == [hw, hw]
    print('patch_embed %s: yardstick gate %.3e = %.2e of max|fp64|' % (name, gate, gate / float(want.abs().max())))
    return report('patch_embed', [(name, dist(out, want), gate)])


# ---------------------------------------------------------------------------------------------- 2. refusals
def run_refusals(device):
    lib = _lib.get()
    name = 'k3_2x64x12x9_160'
    m = make_embed(name).to(device)
    x = kernel_case(name)[0].to(device)
    out = torch.full((4 * 2 * 6 * 5 * 160,), float('nan'), device=device)
    big = torch.zeros(528 * 64 * 9, device=device)              # room for every weight / vector the bad sizes name
    p, st = ops._ptr, ops._stream(x)
    w, b, g, be = m.proj.weight, m.proj.bias, m.norm.weight, m.norm.bias
    good = [p(x), p(w), p(b), p(g), p(be), p(out), 2, 64, 12, 9, 160, 3, 2, 1e-5]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[dict(x=0, w=1, b=2, g=3, be=4, out=5, B=6, Cin=7, H=8, W=9, Cout=10, k=11, stride=12, eps=13)[k]] = v
        return a
    cases = dict(cout24=bad(Cout=24, w=p(big), b=p(big), g=p(big), be=p(big)), cout528=bad(Cout=528, w=p(big), b=p(big), g=p(big), be=p(big)),
                 k5s2=bad(k=5, stride=2, w=p(big)), cin6=bad(Cin=6, w=p(big)), eps=bad(eps=-1.0), null=bad(g=None),
                 odd=bad(x=C.c_void_p(x.data_ptr() + 4)), oddout=bad(out=C.c_void_p(out.data_ptr() + 4)), b0=bad(B=0), k7cin64=bad(k=7, stride=4),
                 k3s4=bad(stride=4))
    for tag, a in cases.items():
        assert lib.cffm_patch_embed_fwd(*a, st) != 0 and lib.cffm_last_error(), tag
    assert bool(torch.isnan(out).all())
    with torch.enable_grad(), pytest.raises(_lib.CffmError):
        V.patch_embed(x, m.proj, m.norm)                         # trainable parameters under grad mode: inference only
    with torch.no_grad(), pytest.raises(_lib.CffmError):
        V.patch_embed(x, nn.Conv2d(64, 160, 3, 2, 0).to(device), m.norm)          # padding != k // 2
    assert bool(torch.isnan(out).all())
    assert lib.cffm_patch_embed_fwd(*good, st) == 0 and not bool(torch.isnan(out[:2 * 6 * 5 * 160]).any())
    assert bool(torch.isnan(out[2 * 6 * 5 * 160:]).all())


# ---------------------------------------------------------------------------------------------- 3. cffm_mit_infer, n = 1
@functools.lru_cache(maxsize=None)
def stage_case(name):
    """input, fp64 result of the 'torch' path and the yardstick gate (Linear layers AND the embedding's convolution split)"""
    x = R.synth_input('stage_x', STAGES[name][4], seed=51, scale=1.0)
    m = make_stage(name, torch.float64)
    with torch.no_grad(), TB.impl('torch'):
        want = m(x.double())
        with split_linears(), split_convs([m.patch_embed.proj]):
            yard = m(x.double())
    return x, want, gate_of(yard, want)


def run_stage(device, name):
    x, want, gate = stage_case(name)
    lib = _lib.get()
    m = make_stage(name).to(device)
    xd = x.to(device)
    stages = [(m.patch_embed, m.block, m.norm)]
    arr, keep, shapes = ops.mit_stages(xd.shape, stages)
    need = lib.cffm_mit_infer_ws_floats(arr, 1)
    assert need > 0 and need == lib.cffm_mit_stage_infer_ws_floats(C.byref(ops.mit_stage_cfg(shapes[0], m.block, m.patch_embed.norm, m.norm)))
    outs = []
    with torch.no_grad():
        for fill in (float('nan'), 0.0):        # every byte of the workspace that is read is written by the same call
            ws = torch.full((need,), fill, dtype=torch.float32, device=device)
            out = torch.full(shapes[0], float('nan'), dtype=torch.float32, device=device)
            res = V.mit_infer(xd, stages, ws=ws, outs=[out])
            assert len(res) == 1 and res[0] is out and not bool(torch.isnan(out).any())
            outs.append(out)
    assert torch.equal(outs[0], outs[1]) and tuple(outs[0].shape) == tuple(want.shape) and outs[0].is_contiguous()
    print('mit_infer %s: yardstick gate %.3e = %.2e of max|fp64|' % (name, gate, gate / float(want.abs().max())))
    return report('mit_infer n=1', [(name, dist(outs[0], want), gate)])


def run_infer_refusals(device):
    """cffm_mit_infer refuses a cfg that is not the convolution's output shape, a broken chain, n outside 1..4 and aliased outputs"""
    lib = _lib.get()
    m = make_stage('d160s2').to(device)
    x = R.synth_input('stage_x', STAGES['d160s2'][4], seed=51, scale=1.0).to(device)
    stages = [(m.patch_embed, m.block, m.norm)]
    arr, keep, shapes = ops.mit_stages(x.shape, stages)
    need = lib.cffm_mit_infer_ws_floats(arr, 1)
    ws = torch.empty(need, device=device)
    out = torch.full(shapes[0], float('nan'), device=device)
    outs = (C.c_void_p * 1)(out.data_ptr())

    def call(a, n=1, o=outs, xin=x):
        return lib.cffm_mit_infer(a, n, ops._ptr(xin), o, ops._ptr(ws), ops._stream(x))

    def changed(**kw):
        a, _, _ = ops.mit_stages(x.shape, stages)
        for k, v in kw.items():
            if k in ('H', 'W', 'C', 'B'):
                setattr(a[0].cfg, k, v)
            else:
                setattr(a[0], k, v)
        return a
    for tag, a in dict(h=changed(H=shapes[0][2] + 1), w=changed(W=shapes[0][3] - 1), k=changed(k=7, stride=4), cin=changed(Cin=6),
                       nullw=changed(conv_w=None), oddb=changed(conv_b=m.patch_embed.proj.bias.data_ptr() + 4)).items():
        assert call(a) != 0 and lib.cffm_last_error(), tag
    for tag, a in dict(h=changed(H=shapes[0][2] + 1), k=changed(k=5)).items():
        assert lib.cffm_mit_infer_ws_floats(a, 1) < 0, tag
    assert call(arr, n=0) != 0 and call(arr, n=5) != 0 and lib.cffm_mit_infer_ws_floats(arr, 0) < 0
    assert call(arr, o=(C.c_void_p * 1)(None)) != 0 and call(arr, o=None) != 0
    assert call(arr, o=(C.c_void_p * 1)(x.data_ptr())) != 0
    two = (_lib.MitStage * 2)()
    C.memmove(two, arr, C.sizeof(_lib.MitStage))
    C.memmove(C.byref(two, C.sizeof(_lib.MitStage)), arr, C.sizeof(_lib.MitStage))      # stage 1 does not continue stage 0
    assert call(two, n=2, o=(C.c_void_p * 2)(out.data_ptr(), out.data_ptr())) != 0 and lib.cffm_last_error()
    assert bool(torch.isnan(out).all())
    with torch.enable_grad(), pytest.raises(_lib.CffmError):
        V.mit_infer(x, stages)
    assert call(arr) == 0 and not bool(torch.isnan(out).any())
    del keep


# ---------------------------------------------------------------------------------------------- 4. the whole backbone
@functools.lru_cache(maxsize=None)
def golden_gates():
    """per output: 4 x the yardstick's distance to mit_b0_96x72.npz (the reference's own fp64 outputs) + one fp32 ulp of its largest value"""
    gold = TB.golden('mit_b0_96x72.npz')
    with torch.no_grad(), TB.impl('torch'), impls('torch', 'torch'):
        m = TB.make(CPU, dtype=torch.float64).eval()
        with split_linears(), split_convs(embed_convs(m)):
            yard = m(R.synth_input('img', (1, 3, 96, 72), seed=41, scale=1.0).double())
    return [gate_of(y, torch.from_numpy(gold['out%d' % i])) for i, y in enumerate(yard)]


def stage_ws_floats(m, shape):
    """cffm_mit_stage_infer_ws_floats of each stage of backbone m on an input of `shape`"""
    lib, figs = _lib.get(), []
    for i in range(1, 5):
        pe = getattr(m, 'patch_embed%d' % i)
        ho, wo = ops.patch_embed_out_hw(pe.proj, shape[2], shape[3])
        shape = (shape[0], pe.proj.out_channels, ho, wo)
        figs.append(lib.cffm_mit_stage_infer_ws_floats(C.byref(ops.mit_stage_cfg(shape, getattr(m, 'block%d' % i), pe.norm, getattr(m, 'norm%d' % i)))))
    return figs


def run_golden_eval(device):
    gold, gates = TB.golden('mit_b0_96x72.npz'), golden_gates()
    shape = (1, 3, 96, 72)
    with impls('hip', 'hip'), CallSpy(_lib.get(), SPY) as spy, torch.no_grad():
        m = TB.make(device, 'mit_b0').eval()
        img = R.synth_input('img', shape, seed=41, scale=1.0).to(device)
        outs = m(img)
        again = m(img)
    assert spy.calls == {SPY[0]: 2, SPY[1]: 0, SPY[2]: 0}, spy.calls          # one call per forward
    assert [tuple(o.shape[2:]) for o in outs] == [(24, 18), (12, 9), (6, 5), (3, 3)]
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(outs, again))
    figs = stage_ws_floats(m, shape)
    assert len(m._run_workspaces) == 1 and [w.numel() for w in m._run_workspaces.values()] == [max(figs)] and min(figs) > 0
    assert not any('_run' in k for k in m.state_dict())
    for i, g in enumerate(gates):
        print('mit_b0 96x72 out%d: gate %.2e of max|golden|' % (i, g / float(np.abs(gold['out%d' % i]).max())))
    return report('mit_b0 96x72', [('out%d' % i, dist(o, torch.from_numpy(gold['out%d' % i])), gates[i]) for i, o in enumerate(outs)])


def run_segmentor(device):
    with impls('hip', 'hip'), CallSpy(_lib.get(), SPY) as spy:
        TB.run_segmentor_eval(device)              # head logits within 1e-3 of seg_mit_b0_64.npz; simple_test: int64 (1, 60, 67)
    assert spy.calls[SPY[0]] >= 1 and spy.calls[SPY[1]] == 0, spy.calls


# ---------------------------------------------------------------------------------------------- 5. dispatch
SMALL = TS.SMALL


def run_dispatch_off(device):
    """embed_impl = 'hip' alone calls nothing new; both 'torch' is the parent's path, bit for bit on the CPU, with no new call"""
    lib = _lib.get()
    with impls('torch', 'hip'), CallSpy(lib, SPY) as spy:
        a = TS.run_backbone(device, 'mit_b0', SMALL)
    assert spy.calls == {n: 0 for n in SPY}, spy.calls
    with impls('torch', 'torch'), CallSpy(lib, SPY) as spy:
        b = TS.run_backbone(device, 'mit_b0', SMALL)
    assert spy.calls == {n: 0 for n in SPY}, spy.calls
    with impls('hip', 'torch'), CallSpy(lib, SPY) as spy:
        c = TS.run_backbone(device, 'mit_b0', SMALL)
    assert spy.calls == {SPY[0]: 0, SPY[1]: 4, SPY[2]: 0}, spy.calls
    if device.type == 'cpu':          # (two calls of the stock Conv2d need not return the same bits on the GPU)
        with torch.no_grad():
            m = TB.make(device).eval()
            x = TS.small_img(device)
            want = []
            for i in range(1, 5):     # the parent's forward_features, written out
                x, H, W = getattr(m, 'patch_embed%d' % i)(x)
                for blk in getattr(m, 'block%d' % i):
                    x = blk(x, H, W)
                x = getattr(m, 'norm%d' % i)(x).reshape(1, H, W, -1).permute(0, 3, 1, 2).contiguous()
                want.append(x)
        assert all(torch.equal(p, q) for p, q in zip(a, want)) and all(torch.equal(p, q) for p, q in zip(b, want))
    for p, q in zip(c, b):
        assert dist(p, q) <= 1e-4 * float(q.abs().max())


def run_dispatch_calls(device):
    lib = _lib.get()
    with impls('hip', 'hip'), CallSpy(lib, SPY + TS.SPY[1:]) as spy:
        hip = TS.run_backbone(device, 'mit_b0', SMALL)
    assert spy.calls == dict({n: 0 for n in SPY + TS.SPY[1:]}, cffm_mit_infer=1), spy.calls
    with impls('torch', 'torch'):
        ref = TS.run_backbone(device, 'mit_b0', SMALL)
    for a, b in zip(hip, ref):
        assert dist(a, b) <= 1e-4 * float(b.abs().max())


def run_dispatch_grad(device):
    """grad enabled and trainable parameters: today's path, with gradients"""
    lib, img = _lib.get(), TS.small_img(device)
    with impls('hip', 'hip'), CallSpy(lib, SPY) as spy:
        m = TB.make(device).eval()
        outs = m(img)
        sum(o.sum() for o in outs).backward()
    assert spy.calls == {n: 0 for n in SPY}, spy.calls
    g = m.patch_embed1.proj.weight.grad
    assert all(o.requires_grad for o in outs) and g is not None and float(g.abs().max()) > 0


def run_dispatch_tensors(device):
    """an fp64 module and, outside the emulator, a CPU module take today's path"""
    lib = _lib.get()
    with impls('hip', 'hip'), CallSpy(lib, SPY) as spy:
        TS.run_backbone(device, 'mit_b0', SMALL, torch.float64)
        assert spy.calls == {n: 0 for n in SPY}, spy.calls
        prev, _lib._override = _lib._override, None
        try:
            TS.run_backbone(CPU, 'mit_b0', SMALL)
        finally:
            _lib._override = prev
        assert spy.calls == {n: 0 for n in SPY}, spy.calls


def small_heads_model(device):
    m = B.MixVisionTransformer(patch_size=4, embed_dims=[32, 64, 160, 256], num_heads=[2, 2, 5, 8], depths=[1, 1, 1, 1], qkv_bias=True)
    m.load_state_dict(R.synth_state(m, seed=40), strict=True)
    return m.to(device).eval()


def run_dispatch_limits(device):
    """stage 1 outside the stage call's limits (head size 16): one torch stage, then ONE call with n = 3"""
    lib, img = _lib.get(), TS.small_img(device)
    seen = []
    with impls('hip', 'hip'), CallSpy(lib, SPY + TS.SPY[1:2]) as spy, torch.no_grad():
        m = small_heads_model(device)
        real = lib.cffm_mit_infer
        lib.cffm_mit_infer = lambda a, n, *r: (seen.append(n), real(a, n, *r))[1]
        try:
            a = m(img)
        finally:
            lib.cffm_mit_infer = real
    assert seen == [3] and spy.calls[SPY[1]] == 0 and spy.calls[TS.SPY[1]] == 1, (seen, spy.calls)
    with impls('torch', 'torch'), torch.no_grad():
        b = m(img)
    for x, y in zip(a, b):
        assert dist(x, y) <= 1e-4 * float(y.abs().max())
    assert len(m._run_workspaces) == 1 and '_stage_workspaces' not in m.__dict__


def run_dispatch_split(device):
    """a patch_embed2.proj outside the kernel's limits (padding 0) splits the run: two calls, stage 2 on today's path alone (stock Conv2d +
    the stage call).  On a 64 x 64 image: at 32 x 32 the unpadded convolution leaves a 3 x 3 map, smaller than stage 2's 4 x 4 `sr` kernel,
    which no path accepts."""
    lib, img = _lib.get(), R.synth_input('img', (1, 3, 64, 64), seed=41, scale=1.0).to(device)
    seen = []
    with impls('hip', 'hip'), CallSpy(lib, SPY) as spy, torch.no_grad():
        m = TB.make(device).eval()
        old = m.patch_embed2.proj
        new = nn.Conv2d(old.in_channels, old.out_channels, 3, 2, 0).to(device)
        new.weight.copy_(old.weight)
        new.bias.copy_(old.bias)
        m.patch_embed2.proj = new
        real = lib.cffm_mit_infer
        lib.cffm_mit_infer = lambda a, n, *r: (seen.append(n), real(a, n, *r))[1]
        try:
            a = m(img)
        finally:
            lib.cffm_mit_infer = real
    assert seen == [1, 2] and spy.calls[SPY[1]] == 1 and spy.calls[SPY[2]] == 0, (seen, spy.calls)
    with impls('torch', 'torch'), torch.no_grad():
        b = m(img)
    for x, y in zip(a, b):
        assert x.shape == y.shape and dist(x, y) <= 1e-4 * float(y.abs().max())


# ---------------------------------------------------------------------------------------------- CPU (emulator)
@pytest.mark.parametrize('name', list(KERNEL_CASES))
def test_kernel(name):
    with emu.active():
        run_kernel(CPU, name)


def test_refusals_enqueue_nothing():
    with emu.active():
        run_refusals(CPU)


@pytest.mark.parametrize('name', list(STAGES))
def test_mit_infer_one_stage(name):
    with emu.active():
        run_stage(CPU, name)


def test_mit_infer_refusals():
    with emu.active():
        run_infer_refusals(CPU)


def test_golden_eval_96x72_is_one_call():
    with emu.active():
        run_golden_eval(CPU)


def test_segmentor_with_both_impls_hip():
    with emu.active():
        run_segmentor(CPU)


@pytest.mark.parametrize('what', ['off', 'calls', 'grad', 'tensors', 'limits', 'split'])
def test_dispatch(what):
    with emu.active():
        globals()['run_dispatch_' + what](CPU)
