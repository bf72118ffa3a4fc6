"""The MiT backbones with the fused attention core (Attention.attn_impl = 'hip': vss_cffm_amd.sra_attention) on the CPU through the fiber
emulator.  The GPU half is tests/test_backbone_sra_gpu.py and shares the run_*(device) bodies below.  The goldens, the gates and the
helper bodies are those of tests/test_backbone.py, whose impl(kind) switches the Mix-FFN only; attn(kind) here switches the attention, and
every test selects both explicitly.

Measured (largest error / gate over the tensors of a kind), attention 'hip' with the Mix-FFN 'hip' | 'torch':
    through the emulator: outputs 64x64 0.028 | 0.022, outputs 96x72 0.025 | 0.025, input gradient 0.078 | 0.087,
    parameter gradients 0.336 (block4.1.attn.q.bias) | 0.641 (block3.1.attn.kv.weight)
    on the MI355X: outputs 0.027 | 0.031 (64x64), 0.029 | 0.029 (96x72); input gradient 0.087 | 0.104; parameter gradients 0.53-0.75
    (block1.1.attn.q.bias) in three runs (stock PyTorch attention on the same GPU: 0.65-0.76)
"""
import contextlib
import json
import os

import pytest
import torch

import vss_cffm_amd as V
from oracle import recipe as R
from tests import emu
from tests import test_backbone as T
from tests.test_mixffn import CallSpy
from vss_cffm_amd import _lib
from vss_cffm_amd import backbone as B

ATTN = ('cffm_sra_attn_fwd', 'cffm_sra_attn_bwd')


@contextlib.contextmanager
def attn(kind):
    """Attention.attn_impl for the block; 'hip' on CPU tensors runs through the emulator"""
    prev = B.Attention.attn_impl
    B.Attention.attn_impl = kind
    try:
        yield
    finally:
        B.Attention.attn_impl = prev


def run_goldens(device, dwconv):
    """attention 'hip': the 64 x 64 training goldens (outputs, input gradient, 176 parameter gradients) and the 96 x 72 eval outputs"""
    with attn('hip'), CallSpy(_lib.get(), ATTN) as spy:
        T.run_golden_train(device, dwconv)
        assert spy.calls == {ATTN[0]: 8, ATTN[1]: 8}
        T.run_golden_eval(device, dwconv)
        assert spy.calls == {ATTN[0]: 16, ATTN[1]: 8}


def run_hip_vs_torch(device):
    with attn('hip'):
        a = T.run_golden_eval(device, 'hip')
    with attn('torch'):
        b = T.run_golden_eval(device, 'hip')
    for i, (x, y) in enumerate(zip(a, b)):
        assert float((x - y).abs().max()) <= T.OUT_GATE * float(y.abs().max()), i


def run_call_counts(device):
    """one training pass of mit_b0: 8 forward and 8 backward calls with 'hip', none with 'torch'"""
    for kind, n in (('hip', 8), ('torch', 0)):
        with attn(kind), T.impl('hip'), CallSpy(_lib.get(), ATTN) as spy:
            m = T.make(device)
            T.train_pass(m, device)
        assert spy.calls == {ATTN[0]: n, ATTN[1]: n}, (kind, spy.calls)


def run_fallback(device):
    """attention dropout, or a head size that is not 32 / 64: the torch sequence, bit for bit what attn_impl = 'torch' gives"""
    for kw in (dict(dim=64, num_heads=2, attn_drop=0.1, sr_ratio=2), dict(dim=96, num_heads=2, sr_ratio=1)):
        torch.manual_seed(0)
        m = B.Attention(qkv_bias=True, **kw).to(device).eval()
        x = R.synth_input('x', (2, 24, kw['dim']), seed=44, scale=1.0).to(device)
        with CallSpy(_lib.get(), ATTN) as spy:
            with attn('hip'):
                assert not m._fused(x)
                a = m(x, 4, 6)
            with attn('torch'):
                b = m(x, 4, 6)
        assert spy.calls == {ATTN[0]: 0, ATTN[1]: 0} and torch.equal(a, b) and bool(a.isfinite().all())
    torch.manual_seed(0)
    m = B.Attention(dim=64, num_heads=2, qkv_bias=True, sr_ratio=2).to(device)
    x = R.synth_input('x', (2, 24, 64), seed=44, scale=1.0).to(device)
    with attn('hip'):
        assert m._fused(x) and not m._fused(x.double())
    with attn('torch'):
        assert not m._fused(x)


# ---------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize('dwconv', ['hip', 'torch'])
def test_goldens_with_the_fused_attention(dwconv):
    with emu.active():
        run_goldens(torch.device('cpu'), dwconv)


def test_hip_against_torch():
    with emu.active():
        run_hip_vs_torch(torch.device('cpu'))


def test_call_counts():
    with emu.active():
        run_call_counts(torch.device('cpu'))


def test_torch_in_fp64_never_reaches_the_library():
    with emu.active(), attn('hip'), T.impl('hip'), CallSpy(_lib.get(), ATTN + ('cffm_dwconv_gelu_fwd',)) as spy:
        m = T.make(torch.device('cpu'), dtype=torch.float64)
        T.train_pass(m, torch.device('cpu'), torch.float64)
    assert not any(spy.calls.values())


def test_fallback_is_the_torch_sequence():
    with emu.active():
        run_fallback(torch.device('cpu'))


def test_cpu_tensors_take_the_torch_sequence_outside_the_emulator():
    with attn('hip'), T.impl('hip'):
        m = T.make(torch.device('cpu')).eval()
        with torch.no_grad():
            outs = m(R.synth_input('img', (1, 3, 96, 72), seed=41, scale=1.0))
    T.check_outputs(outs, T.golden('mit_b0_96x72.npz'), "'hip' on CPU tensors without the emulator")


def test_state_dict_keys_are_unchanged():
    want = json.load(open(os.path.join(T.GOLDEN, 'mit_state_dict_keys.json')))
    for kind in ('mit_b0', 'mit_b1'):
        with attn('hip'):
            m = V.build_backbone(dict(type=kind, style='pytorch'))
        assert [[k, list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()] == want[kind]
    assert B.Attention.attn_impl in ('hip', 'torch')
