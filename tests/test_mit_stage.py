"""One MiT stage per library call (cffm_mit_stage_infer, MixVisionTransformer.stage_impl = 'hip') and the three LayerNorm kernels behind it
(csrc/mitln_kernels.h), on the CPU through the fiber emulator.  The GPU half is tests/test_mit_stage_gpu.py and shares the run_*(device)
bodies below.

Gates.  LayerNorm kernels: 4 x max|F.layer_norm in fp32 - the same in fp64| + 2^-23 x max|out| (one fp32 ulp of the largest element: the
fp32 yardstick can be exact by luck on tiny inputs).  Stage path: its Linear layers are the library's three-pass bf16-split GEMMs, so the
yardstick is the 'torch' path of the same module in fp64 with F.linear replaced by a function that splits both operands into bf16 hi + bf16
lo and returns hi.hi + hi.lo + lo.hi (+ bias); the gate per output tensor is 4 x that yardstick's max-abs distance to the plain fp64
result (the margin covers fp32 accumulation, the rounding mode of the library's split and the order of the LayerNorm sums).  Every test
prints error / gate per tensor.

Largest error / gate measured (the same figures are in DESIGN.md section 3p):
    through the emulator (CPU):  LayerNorm kernels 0.263 (ln_rows 7x512);  single stages 0.269 (d64s8nobias);  mit_b0 96x72 0.274 (out0)
    on the MI355X:               LayerNorm kernels 0.235 (2x160x6x5);      single stages 0.278 (d160s2);       mit_b0 96x72 0.271 (out0);
                                 mit_b1 on [2,3,96,128] against fp64 on the CPU 0.267 (out0, out3)
The patch-embedding convolution is called once per comparison: on the MI355X two calls of the stock Conv2d on the same input need not
return the same bits.
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
from tests.test_mixffn import CallSpy
from vss_cffm_amd import _lib, ops
from vss_cffm_amd import backbone as B

CPU = torch.device('cpu')
MARGIN = 4.0
LN_SHAPES = [(1, 16), (9, 32), (30, 160), (432, 32), (131, 320), (7, 512), (65, 64)]
LN_NAMES = ['%dx%d' % s for s in LN_SHAPES] + ['30x160+mean']
MAP_SHAPES = [(1, 32, 24, 18), (2, 160, 6, 5), (2, 512, 3, 3), (1, 64, 17, 19), (1, 320, 1, 1)]
MAP_NAMES = ['%dx%dx%dx%d' % s for s in MAP_SHAPES]
# in-chans, dim, heads, sr, input shape, qkv_bias
STAGES = {
    'd64s8': (3, 64, 1, 8, (2, 3, 68, 76), True),          # map 17 x 19, sr with a remainder, head size 64
    'd32s8': (3, 32, 1, 8, (1, 3, 96, 72), True),
    'd128s4': (64, 128, 2, 4, (2, 64, 18, 22), True),
    'd160s2': (64, 160, 5, 2, (2, 64, 12, 9), True),        # head size 32, C / 4 = 40 lanes
    'd320s2': (128, 320, 5, 2, (2, 128, 10, 14), True),
    'd512s1': (320, 512, 8, 1, (2, 320, 5, 6), True),       # no sr, Nk = N = 9
    'd64s8nobias': (3, 64, 1, 8, (2, 3, 68, 76), False),
}
SPY = ('cffm_mit_stage_infer', 'cffm_dwconv_gelu_fwd', 'cffm_sra_attn_fwd', 'cffm_sr_ln_fwd')


@contextlib.contextmanager
def stage_impl(kind):
    prev = B.MixVisionTransformer.stage_impl
    B.MixVisionTransformer.stage_impl = kind
    try:
        yield
    finally:
        B.MixVisionTransformer.stage_impl = prev


# ---------------------------------------------------------------------------------------------- the yardstick
def _split(t):
    hi = t.float().bfloat16().double()
    lo = (t - hi).float().bfloat16().double()
    return hi, lo


def split_linear(x, w, b=None):
    xh, xl = _split(x)
    wh, wl = _split(w)
    y = xh @ wh.t() + xh @ wl.t() + xl @ wh.t()
    return y if b is None else y + b


@contextlib.contextmanager
def split_linears():
    prev = F.linear
    F.linear = split_linear
    try:
        yield
    finally:
        F.linear = prev


def report(tag, pairs):
    """pairs of (name, error, gate): print every ratio, then assert"""
    for name, err, gate in pairs:
        print('%s: %s err %.3e gate %.3e (%.3f of it)' % (tag, name, err, gate, err / gate))
    for name, err, gate in pairs:
        assert err <= gate, (tag, name, err, gate)
    return max(e / g for _, e, g in pairs)


def dist(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


# ---------------------------------------------------------------------------------------------- 1. the LayerNorm kernels
@functools.lru_cache(maxsize=None)
def ln_case(name):
    """x [M,C], gamma, beta, eps and (fp64 result, gate) of a rows case"""
    shifted = name.endswith('+mean')
    m, c = (int(v) for v in name.split('+')[0].split('x'))
    x = R.synth_input('ln_x', (m, c), seed=52, scale=1.0)
    if shifted:
        x = x + 30.0                                   # rows with mean ~ 30 x their standard deviation
    g = 1.0 + 0.2 * R.synth_input('ln_g', (c,), seed=52, scale=1.0)
    b = 0.1 * R.synth_input('ln_b', (c,), seed=52, scale=1.0)
    eps = 1e-6 if c % 32 else 1e-5
    want = F.layer_norm(x.double(), (c,), g.double(), b.double(), eps)
    gate = MARGIN * dist(F.layer_norm(x, (c,), g, b, eps), want) + 2.0 ** -23 * float(want.abs().max())
    return x, g, b, eps, want, gate


@functools.lru_cache(maxsize=None)
def map_case(name):
    """a map [B,C,H,W] with its LayerNorm over C as rows (fp64) and the gate"""
    shape = tuple(int(v) for v in name.split('x'))
    b_, c, h, w = shape
    x = R.synth_input('map_x', shape, seed=53, scale=1.0)
    g = 1.0 + 0.2 * R.synth_input('ln_g', (c,), seed=53, scale=1.0)
    b = 0.1 * R.synth_input('ln_b', (c,), seed=53, scale=1.0)
    eps = 1e-6
    rows = x.flatten(2).transpose(1, 2).contiguous()
    want = F.layer_norm(rows.double(), (c,), g.double(), b.double(), eps)
    gate = MARGIN * dist(F.layer_norm(rows, (c,), g, b, eps), want) + 2.0 ** -23 * float(want.abs().max())
    return x, rows, g, b, eps, want, gate


def _twice(fn, shape, device):
    """fn(out) on two NaN-poisoned outputs: both fully written, the same bits"""
    outs = []
    for _ in range(2):
        out = torch.full(shape, float('nan'), dtype=torch.float32, device=device)
        assert fn(out) is out
        assert not bool(torch.isnan(out).any())
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    return outs[0]


def run_ln_rows(device, name):
    x, g, b, eps, want, gate = ln_case(name)
    xd, gd, bd = (t.to(device) for t in (x, g, b))
    with torch.no_grad():
        out = _twice(lambda o: V.ln_rows(xd, gd, bd, eps, out=o), x.shape, device)
    return report('ln_rows', [(name, dist(out, want), gate)])


def run_nchw_ln_rows(device, name):
    x, rows, g, b, eps, want, gate = map_case(name)
    xd, gd, bd = (t.to(device) for t in (x, g, b))
    with torch.no_grad():
        out = _twice(lambda o: V.nchw_ln_rows(xd, gd, bd, eps, out=o), rows.shape, device)
    return report('nchw_ln_rows', [(name, dist(out, want), gate)])


def run_ln_rows_nchw(device, name):
    x, rows, g, b, eps, want, gate = map_case(name)
    b_, c, h, w = x.shape
    rd, gd, bd = (t.to(device) for t in (rows, g, b))
    with torch.no_grad():
        out = _twice(lambda o: V.ln_rows_nchw(rd, gd, bd, h, w, eps, out=o), x.shape, device)
    return report('ln_rows_nchw', [(name, dist(out, want.reshape(b_, h, w, c).permute(0, 3, 1, 2)), gate)])


def run_ln_refusals(device):
    x = torch.zeros(4, 16, device=device)
    g = torch.ones(16, device=device)
    for bad in (torch.zeros(4, 12, device=device), torch.zeros(4, 516, device=device), torch.zeros(4, 18, device=device)):
        with pytest.raises(_lib.CffmError):
            V.ln_rows(bad, torch.ones(bad.shape[1], device=device), torch.ones(bad.shape[1], device=device))
    with pytest.raises(_lib.CffmError):
        V.ln_rows(x, g.requires_grad_(True), torch.ones(16, device=device))        # inference only
    lib = _lib.get()
    out = torch.full((4, 16), float('nan'), device=device)
    g = torch.ones(16, device=device)
    p = ops._ptr
    for args in ((p(x), p(g), p(g), p(out), 4, 12, 1e-5), (p(x), p(g), p(g), p(out), 4, 16, -1.0), (p(x), None, p(g), p(out), 4, 16, 1e-5),
                 (p(x), p(g), p(g), C.c_void_p(out.data_ptr() + 4), 4, 16, 1e-5), (p(x), p(g), p(g), p(out), 0, 16, 1e-5)):
        assert lib.cffm_ln_rows(*args, ops._stream(x)) != 0 and lib.cffm_last_error()
    for fn in (lib.cffm_nchw_ln_rows, lib.cffm_ln_rows_nchw):
        assert fn(p(x), p(g), p(g), p(out), 1, 20, 0, 4, 1e-5, ops._stream(x)) != 0 and lib.cffm_last_error()
    assert bool(torch.isnan(out).all())


# ---------------------------------------------------------------------------------------------- 2. single stages
class Stage(nn.Module):
    """one stage of a MixVisionTransformer: OverlapPatchEmbed + two Blocks + LayerNorm"""

    def __init__(self, in_chans, dim, heads, sr, qkv_bias=True, first=False):
        super().__init__()
        self.patch_embed = B.OverlapPatchEmbed(img_size=64, patch_size=7 if first else 3, stride=4 if first else 2, in_chans=in_chans, embed_dim=dim)
        self.block = nn.ModuleList([B.Block(dim=dim, num_heads=heads, mlp_ratio=4, qkv_bias=qkv_bias, drop_path=0., sr_ratio=sr,
                                            norm_layer=functools.partial(nn.LayerNorm, eps=1e-6)) for _ in range(2)])
        self.norm = nn.LayerNorm(dim, eps=1e-6)

    def forward(self, x):
        """the 'torch' path (one iteration of forward_features)"""
        n = x.shape[0]
        x, H, W = self.patch_embed(x)
        for blk in self.block:
            x = blk(x, H, W)
        return self.norm(x).reshape(n, H, W, -1).permute(0, 3, 1, 2).contiguous()

    def hip(self, x, ws=None):
        return V.mit_stage_infer(self.patch_embed.proj(x), self.patch_embed.norm, self.block, self.norm, ws=ws)


def make_stage(name, dtype=torch.float32):
    cin, dim, heads, sr, _, qkv_bias = STAGES[name]
    m = Stage(cin, dim, heads, sr, qkv_bias, first=cin == 3)
    m.load_state_dict(R.synth_state(m, seed=50), strict=True)
    return m.to(dtype).eval()


@functools.lru_cache(maxsize=None)
def stage_case(name):
    """input, fp64 result of the 'torch' path and the yardstick gate"""
    x = R.synth_input('stage_x', STAGES[name][4], seed=51, scale=1.0)
    m = make_stage(name, torch.float64)
    with torch.no_grad(), TB.impl('torch'):
        want = m(x.double())
        with split_linears():
            yard = m(x.double())
    return x, want, MARGIN * dist(yard, want)


def run_stage(device, name):
    x, want, gate = stage_case(name)
    m = make_stage(name).to(device)
    xd = x.to(device)
    with torch.no_grad():
        y = m.patch_embed.proj(xd)
        need = _lib.get().cffm_mit_stage_infer_ws_floats(C.byref(ops.mit_stage_cfg(y.shape, m.block, m.patch_embed.norm, m.norm)))
        assert need > 0
        outs = []
        for fill in (float('nan'), 0.0):        # every byte of the workspace that is read is written by the same call
            ws = torch.full((need,), fill, dtype=torch.float32, device=device)
            outs.append(V.mit_stage_infer(y, m.patch_embed.norm, m.block, m.norm, ws=ws))      # (the same y: one convolution call)
    assert torch.equal(outs[0], outs[1]) and tuple(outs[0].shape) == tuple(want.shape) and outs[0].is_contiguous()
    rel = gate / float(want.abs().max())
    print('stage %s: yardstick gate %.3e = %.2e of max|fp64|' % (name, gate, rel))
    return report('stage', [(name, dist(outs[0], want), gate)])


# ---------------------------------------------------------------------------------------------- 3. the whole backbone
@functools.lru_cache(maxsize=None)
def golden_gates():
    """per output: 4 x the yardstick's distance to mit_b0_96x72.npz (the reference's own fp64 outputs)"""
    gold = TB.golden('mit_b0_96x72.npz')
    with torch.no_grad(), TB.impl('torch'), stage_impl('torch'), split_linears():
        m = TB.make(CPU, dtype=torch.float64).eval()
        yard = m(R.synth_input('img', (1, 3, 96, 72), seed=41, scale=1.0).double())
    return [MARGIN * dist(y, torch.from_numpy(gold['out%d' % i])) for i, y in enumerate(yard)]


def run_golden_eval(device):
    gold, gates = TB.golden('mit_b0_96x72.npz'), golden_gates()
    with stage_impl('hip'), CallSpy(_lib.get(), SPY[:1]) as spy:
        outs = run_backbone(device, 'mit_b0', (1, 3, 96, 72))
    assert spy.calls[SPY[0]] == 4
    assert [tuple(o.shape[2:]) for o in outs] == [(24, 18), (12, 9), (6, 5), (3, 3)]
    for i, g in enumerate(gates):
        print('mit_b0 96x72 out%d: gate %.2e of max|golden|' % (i, g / float(np.abs(gold['out%d' % i]).max())))
    return report('mit_b0 96x72', [('out%d' % i, dist(o, torch.from_numpy(gold['out%d' % i])), gates[i]) for i, o in enumerate(outs)])


def run_backbone(device, kind, shape, dtype=torch.float32):
    with torch.no_grad():
        m = TB.make(device, kind, dtype).eval()
        return m(R.synth_input('img', shape, seed=41, scale=1.0, dtype=dtype).to(device))


# ---------------------------------------------------------------------------------------------- 4. the segmentor
def run_segmentor(device):
    with stage_impl('hip'), CallSpy(_lib.get(), SPY[:1]) as spy:
        TB.run_segmentor_eval(device)              # head logits within 1e-3 of seg_mit_b0_64.npz; simple_test: int64 (1, 60, 67)
    assert spy.calls[SPY[0]] >= 4 and spy.calls[SPY[0]] % 4 == 0, spy.calls


# ---------------------------------------------------------------------------------------------- 5. dispatch
SMALL = (1, 3, 32, 32)          # maps 8 x 8 (sr 8), 4 x 4, 2 x 2, 1 x 1: the smallest image every stage of mit_b0 accepts


def small_img(device):
    return R.synth_input('img', SMALL, seed=41, scale=1.0).to(device)


def run_dispatch_calls(device):
    """'hip' under no_grad: four stage calls and nothing else from Python; 'torch': none"""
    lib = _lib.get()
    with stage_impl('hip'), CallSpy(lib, SPY) as spy:
        hip = run_backbone(device, 'mit_b0', SMALL)
    assert spy.calls == {SPY[0]: 4, SPY[1]: 0, SPY[2]: 0, SPY[3]: 0}, spy.calls
    with stage_impl('torch'), CallSpy(lib, SPY) as spy:
        ref = run_backbone(device, 'mit_b0', SMALL)
    assert spy.calls == {SPY[0]: 0, SPY[1]: 8, SPY[2]: 8, SPY[3]: 0}, spy.calls
    for a, b in zip(hip, ref):
        assert dist(a, b) <= 1e-4 * float(b.abs().max())


def run_dispatch_grad(device):
    """grad enabled and trainable parameters: today's path, bit for bit, with gradients"""
    lib, img, got = _lib.get(), small_img(device), {}
    for kind in ('hip', 'torch'):
        with stage_impl(kind), CallSpy(lib, SPY[:1]) as spy:
            m = TB.make(device).eval()
            outs = m(img)
            sum(o.sum() for o in outs).backward()
            got[kind] = (outs, m.block3[1].mlp.fc2.weight.grad, m.patch_embed1.proj.weight.grad)
        assert spy.calls[SPY[0]] == 0
    for a, b in zip(got['hip'][0], got['torch'][0]):
        assert a.requires_grad and torch.equal(a, b)
    for g in got['hip'][1:] + got['torch'][1:]:          # (the gradients of two runs of stock ops need not agree bit for bit on a GPU)
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


def run_dispatch_modes(device):
    lib, img = _lib.get(), small_img(device)
    with stage_impl('hip'), CallSpy(lib, SPY[:1]) as spy, torch.no_grad():
        m = V.build_backbone(dict(type='mit_b0', style='pytorch')).to(device)
        m.train()(img)                               # train mode, drop-path rate 0.1 (the constructor's): today's path
        assert spy.calls[SPY[0]] == 0
        m.reset_drop_path(0.)
        m(img)                                       # train mode with every rate and dropout 0: nothing is random, the stage path
        assert spy.calls[SPY[0]] == 4
        m.requires_grad_(False)
        with torch.enable_grad():
            m.eval()(img)                            # grad mode on, nothing requires grad
        assert spy.calls[SPY[0]] == 8
        with torch.enable_grad():
            m(img.clone().requires_grad_(True))      # the input requires grad
        assert spy.calls[SPY[0]] == 8


def run_dispatch_tensors(device):
    """an fp64 module and, outside the emulator, a CPU module take today's path"""
    lib = _lib.get()
    with stage_impl('hip'), CallSpy(lib, SPY[:1]) as spy:
        run_backbone(device, 'mit_b0', SMALL, torch.float64)
        assert spy.calls[SPY[0]] == 0
        prev, _lib._override = _lib._override, None
        try:
            run_backbone(CPU, 'mit_b0', SMALL)         # a CPU module outside the emulator
        finally:
            _lib._override = prev
        assert spy.calls[SPY[0]] == 0


def run_dispatch_limits(device):
    """a stage outside the limits (head size 16) falls back alone"""
    lib, img = _lib.get(), small_img(device)
    with stage_impl('hip'), CallSpy(lib, SPY) as spy, torch.no_grad():
        m = B.MixVisionTransformer(patch_size=4, embed_dims=[32, 64, 160, 256], num_heads=[2, 2, 5, 8], depths=[1, 1, 1, 1], qkv_bias=True)
        m.load_state_dict(R.synth_state(m, seed=40), strict=True)
        m = m.to(device).eval()
        a = m(img)
    assert spy.calls == {SPY[0]: 3, SPY[1]: 1, SPY[2]: 0, SPY[3]: 0}, spy.calls
    with stage_impl('torch'), torch.no_grad():
        b = m(img)
    for x, y in zip(a, b):
        assert dist(x, y) <= 1e-4 * float(y.abs().max())
    # the workspace is kept on the module, one per stage, outside the state dict
    assert len(m._stage_workspaces) == 3 and not any('_stage' in k for k in m.state_dict())
    with stage_impl('hip'), torch.no_grad():
        ws = dict(m._stage_workspaces)
        m(img)
        assert all(m._stage_workspaces[k] is v for k, v in ws.items()) and len(m._stage_workspaces) == 3


# ---------------------------------------------------------------------------------------------- 6. argument checks
def run_refusals(device):
    lib = _lib.get()
    m = make_stage('d160s2').to(device)
    x = R.synth_input('stage_x', STAGES['d160s2'][4], seed=51, scale=1.0).to(device)
    with torch.no_grad():
        y = m.patch_embed.proj(x)
    tensors = ops.mit_stage_tensors(m.block, m.patch_embed.norm, m.norm)
    n = len(ops._MIT_FIELDS)

    def call(cfg, out, ws, swap=None, conv=None):
        structs = (_lib.MitBlockPtrs * 2)()
        for i in range(2):
            for f, t in zip(ops._MIT_FIELDS, tensors[i * n:(i + 1) * n]):
                setattr(structs[i], f, t.data_ptr() if t is not None else None)
        ends = [ops._ptr(t) for t in tensors[-4:]]
        if swap:
            swap(structs, ends)
        return lib.cffm_mit_stage_infer(C.byref(cfg), structs, *ends, conv or ops._ptr(y), ops._ptr(out), ops._ptr(ws), ops._stream(y))

    def cfg(**kw):
        c = ops.mit_stage_cfg(y.shape, m.block, m.patch_embed.norm, m.norm)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    good = cfg()
    need = lib.cffm_mit_stage_infer_ws_floats(C.byref(good))
    assert need > 0 and ops.mit_stage_supported(good)
    ws = torch.empty(4 * need + 64, dtype=torch.float32, device=device)
    out = torch.full((4 * y.numel(),), float('nan'), dtype=torch.float32, device=device)
    bad_cfgs = dict(c24=cfg(C=24, heads=1), hd48=cfg(C=48, heads=1), sr3=cfg(sr_ratio=3), small=cfg(H=1, sr_ratio=2), hidden=cfg(hidden=642),
                    c528=cfg(C=528, heads=8), scale=cfg(scale=0.0), eps=cfg(eps_block=-1.0), depth=cfg(depth=0), bheads=cfg(B=20000), huge=cfg(B=2, H=2000, W=2000))
    for name, c in bad_cfgs.items():
        assert lib.cffm_mit_stage_infer_ws_floats(C.byref(c)) < 0, name
        assert not ops.mit_stage_supported(c), name
        assert call(c, out, ws) != 0 and lib.cffm_last_error(), name
    def null_out_g(structs, ends):
        ends[2] = None
    def null_fc1(structs, ends):
        structs[1].fc1_w = None
    def null_sr(structs, ends):
        structs[0].sr_w = None
    def odd_proj(structs, ends):
        structs[0].proj_b = structs[0].proj_b + 4
    for swap in (null_out_g, null_fc1, null_sr, odd_proj):
        assert call(good, out, ws, swap=swap) != 0 and lib.cffm_last_error(), swap.__name__
    assert call(good, out, ws, conv=C.c_void_p(y.data_ptr() + 4)) != 0 and b'aligned' in lib.cffm_last_error()
    assert call(good, out, ws[1:]) != 0 and call(good, out[1:], ws) != 0
    assert lib.cffm_mit_stage_infer(C.byref(good), None, *[ops._ptr(t) for t in tensors[-4:]], ops._ptr(y), ops._ptr(out), ops._ptr(ws), ops._stream(y)) != 0
    assert call(cfg(sr_ratio=1), out, ws) != 0 and b'sr_ratio == 1' in lib.cffm_last_error()      # sr tensors given at sr_ratio 1
    assert bool(torch.isnan(out).all())
    with torch.enable_grad(), pytest.raises(_lib.CffmError):
        m.hip(x)                                     # trainable parameters under grad mode: the operator is inference only
    assert call(good, out, ws) == 0 and not bool(torch.isnan(out[:y.numel()]).any())


# ---------------------------------------------------------------------------------------------- CPU (emulator)
@pytest.mark.parametrize('name', LN_NAMES)
def test_ln_rows(name):
    with emu.active():
        run_ln_rows(CPU, name)


@pytest.mark.parametrize('name', MAP_NAMES)
def test_nchw_ln_rows(name):
    with emu.active():
        run_nchw_ln_rows(CPU, name)


@pytest.mark.parametrize('name', MAP_NAMES)
def test_ln_rows_nchw(name):
    with emu.active():
        run_ln_rows_nchw(CPU, name)


def test_ln_refusals():
    with emu.active():
        run_ln_refusals(CPU)


@pytest.mark.parametrize('name', list(STAGES))
def test_stage(name):
    with emu.active():
        run_stage(CPU, name)


def test_golden_eval_96x72():
    with emu.active():
        run_golden_eval(CPU)


def test_segmentor_with_the_stage_path():
    with emu.active():
        run_segmentor(CPU)


@pytest.mark.parametrize('what', ['calls', 'grad', 'modes', 'tensors', 'limits'])
def test_dispatch(what):
    with emu.active():
        globals()['run_dispatch_' + what](CPU)


def test_refusals_enqueue_nothing():
    with emu.active():
        run_refusals(CPU)
