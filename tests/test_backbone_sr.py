"""The MiT backbone with the fused spatial reduction (Attention.sr_impl = 'hip': ops.sr_reduce -> cffm_sr_ln_fwd / _bwd in place of the
`sr` Conv2d and its LayerNorm) on the CPU through the fiber emulator.  The GPU half is tests/test_backbone_sr_gpu.py and shares the
run_*(device) bodies below.  Goldens, gates and the model builder are those of tests/test_backbone.py; its run_golden_* bodies are
called with sr_impl forced to 'hip' (the 96 x 72 evaluation input has a real tail: stage 1 is 24 x 18 with s = 8).

Measured (largest error / gate over the tensors of a kind) with sr_impl = 'hip', Mlp.dwconv_impl = 'hip', attn_impl = 'hip':
    emulator: outputs 64x64 0.024, outputs 96x72 0.025, input gradient 0.069, parameter gradients 0.891 (block1.1.attn.q.bias)
    MI355X:   outputs 64x64 0.031, outputs 96x72 0.037, input gradient 0.104, parameter gradients 0.843 (block1.1.attn.q.bias; the
              same tensor is at 0.732 of its gate with sr_impl = 'hip' and Mlp.dwconv_impl = 'torch')
"""
import contextlib
import json
import os

import torch

import vss_cffm_amd as V
from oracle import recipe as R
from tests import emu
from tests import test_backbone as T
from tests.test_mixffn import CallSpy
from vss_cffm_amd import _lib
from vss_cffm_amd import backbone as B

NAMES_ABI = ('cffm_sr_ln_fwd', 'cffm_sr_ln_bwd')


@contextlib.contextmanager
def sr_impl(kind):
    prev = B.Attention.sr_impl
    B.Attention.sr_impl = kind
    try:
        yield
    finally:
        B.Attention.sr_impl = prev


def run_golden_train(device):
    with sr_impl('hip'):
        T.run_golden_train(device, 'hip')


def run_golden_eval(device):
    with sr_impl('hip'), CallSpy(_lib.get(), NAMES_ABI) as spy:
        T.run_golden_eval(device, 'hip')
    assert spy.calls == {NAMES_ABI[0]: 6, NAMES_ABI[1]: 0}


def run_call_counts(device):
    """one training pass: two blocks in each of stages 1-3 reduce through the library with 'hip', none with 'torch'"""
    for kind, n in (('hip', 6), ('torch', 0)):
        with sr_impl(kind), CallSpy(_lib.get(), NAMES_ABI) as spy:
            m = T.make(device)
            T.train_pass(m, device)
        assert spy.calls == {NAMES_ABI[0]: n, NAMES_ABI[1]: n}, (kind, spy.calls)


def run_other_inputs_take_the_torch_lines(device):
    """fp64 tensors never reach the library and equal sr_impl = 'torch' bit for bit"""
    outs = {}
    for kind in ('hip', 'torch'):
        with sr_impl(kind), CallSpy(_lib.get(), NAMES_ABI) as spy:
            m = T.make(device, dtype=torch.float64)
            outs[kind] = T.train_pass(m, device, torch.float64)
        assert spy.calls == {n: 0 for n in NAMES_ABI}
    for a, b in zip(outs['hip'][0], outs['torch'][0]):
        assert torch.equal(a, b)
    assert torch.equal(outs['hip'][1], outs['torch'][1])
    assert all(torch.equal(outs['hip'][2][k], outs['torch'][2][k]) for k in outs['torch'][2])


# ---------------------------------------------------------------------------------------------- emulator / CPU
def test_attribute_and_state_dict():
    assert B.Attention.sr_impl in ('hip', 'torch')
    want = json.load(open(os.path.join(T.GOLDEN, 'mit_state_dict_keys.json')))
    with sr_impl('hip'):
        for kind in ('mit_b0', 'mit_b1'):
            m = V.build_backbone(dict(type=kind, style='pytorch'))
            assert [[k, list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()] == want[kind]
            assert m.block1[0].attn.norm.eps == 1e-5


def test_golden_train_64():
    with emu.active():
        run_golden_train(torch.device('cpu'))


def test_golden_eval_96x72():
    with emu.active():
        run_golden_eval(torch.device('cpu'))


def test_call_counts():
    with emu.active():
        run_call_counts(torch.device('cpu'))


def test_fp64_takes_the_torch_lines():
    with emu.active():
        run_other_inputs_take_the_torch_lines(torch.device('cpu'))


def test_cpu_tensors_outside_the_emulator_take_the_torch_lines():
    img = R.synth_input('img', (1, 3, 96, 72), seed=41, scale=1.0)
    outs = {}
    for kind in ('hip', 'torch'):
        with sr_impl(kind), torch.no_grad():
            outs[kind] = T.make(torch.device('cpu')).eval()(img)
    for a, b in zip(outs['hip'], outs['torch']):
        assert torch.equal(a, b)


def test_out_of_limit_shapes_take_the_torch_lines():
    """a reduction ratio outside 2 / 4 / 8 (here 3, with C = 48) never reaches the library and equals sr_impl = 'torch' bit for bit"""
    with emu.active(), sr_impl('hip'), CallSpy(_lib.get(), NAMES_ABI) as spy:
        a = B.Attention(48, num_heads=1, sr_ratio=3)
        x = torch.randn(1, 36, 48, generator=torch.Generator().manual_seed(0))
        with torch.no_grad():
            got = a(x, 6, 6)
            with sr_impl('torch'):
                want = a(x, 6, 6)
    assert spy.calls == {n: 0 for n in NAMES_ABI} and torch.equal(got, want)
