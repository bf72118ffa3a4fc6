"""One MiT stage per library call and the LayerNorm kernels behind it on a real MI355X: the shared run_*(device) bodies of
tests/test_mit_stage.py (what is checked and why is written there) at the same shapes, plus a mit_b1 forward against the fp64 'torch'
path run on the CPU and one stage call captured into a HIP graph.
"""
import ctypes as C

import pytest
import torch

from oracle import recipe as R
from tests import test_backbone as TB
from tests import test_mit_stage as T
from vss_cffm_amd import _lib, ops

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', T.LN_NAMES)
def test_ln_rows(name):
    T.run_ln_rows(dev(), name)


@pytest.mark.parametrize('name', T.MAP_NAMES)
def test_nchw_ln_rows(name):
    T.run_nchw_ln_rows(dev(), name)


@pytest.mark.parametrize('name', T.MAP_NAMES)
def test_ln_rows_nchw(name):
    T.run_ln_rows_nchw(dev(), name)


def test_ln_refusals():
    T.run_ln_refusals(dev())


@pytest.mark.parametrize('name', list(T.STAGES))
def test_stage(name):
    T.run_stage(dev(), name)


def test_golden_eval_96x72():
    T.run_golden_eval(dev())


def test_segmentor_with_the_stage_path():
    T.run_segmentor(dev())


@pytest.mark.parametrize('what', ['calls', 'grad', 'modes', 'tensors', 'limits'])
def test_dispatch(what):
    getattr(T, 'run_dispatch_' + what)(dev())


def test_refusals_enqueue_nothing():
    T.run_refusals(dev())


def test_mit_b1_against_the_fp64_torch_path():
    """mit_b1 on [2,3,96,128] with 'hip' against the fp64 'torch' path on the CPU, under the yardstick gate of the same run"""
    shape = (2, 3, 96, 128)
    with torch.no_grad(), TB.impl('torch'), T.stage_impl('torch'):
        m = TB.make(T.CPU, 'mit_b1', torch.float64).eval()
        img = R.synth_input('img', shape, seed=41, scale=1.0).double()
        want = m(img)
        with T.split_linears():
            yard = m(img)
    with T.stage_impl('hip'):
        outs = T.run_backbone(dev(), 'mit_b1', shape)
    T.report('mit_b1 96x128', [('out%d' % i, T.dist(o, w), T.MARGIN * T.dist(y, w)) for i, (o, w, y) in enumerate(zip(outs, want, yard))])


def test_captured_stage_call_replays_bit_for_bit():
    """one stage call on a single stream, captured with torch.cuda.graph and replayed twice, gives the bits of the eager call (a single
    chain: no side streams, no allocation, no host round trip inside the library)"""
    name = 'd128s4'
    m = T.make_stage(name).to(dev())
    x = R.synth_input('stage_x', T.STAGES[name][4], seed=51, scale=1.0).to(dev())
    with torch.no_grad():
        y = m.patch_embed.proj(x)
        need = _lib.get().cffm_mit_stage_infer_ws_floats(C.byref(ops.mit_stage_cfg(y.shape, m.block, m.patch_embed.norm, m.norm)))
        ws = torch.zeros(need, dtype=torch.float32, device=dev())
        out = torch.empty_like(y)
        first = ops.mit_stage_infer(y, m.patch_embed.norm, m.block, m.norm, ws=ws).clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ops.mit_stage_infer(y, m.patch_embed.norm, m.block, m.norm, ws=ws, out=out)
        for _ in range(2):
            out.fill_(float('nan'))
            ws.fill_(float('nan'))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, first)
