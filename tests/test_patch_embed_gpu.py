"""The patch-embedding kernel and cffm_mit_infer on a real MI355X: the shared run_*(device) bodies of tests/test_patch_embed.py (what is
checked and why is written there) at the same shapes, plus a mit_b1 forward against the fp64 'torch' path run on the CPU and one whole
backbone call captured into a HIP graph.
"""
import pytest
import torch

from oracle import recipe as R
from tests import test_backbone as TB
from tests import test_mit_stage as TS
from tests import test_patch_embed as T
from vss_cffm_amd import _lib, ops

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', list(T.KERNEL_CASES))
def test_kernel(name):
    T.run_kernel(dev(), name)


def test_refusals_enqueue_nothing():
    T.run_refusals(dev())


@pytest.mark.parametrize('name', list(T.STAGES))
def test_mit_infer_one_stage(name):
    T.run_stage(dev(), name)


def test_mit_infer_refusals():
    T.run_infer_refusals(dev())


def test_golden_eval_96x72_is_one_call():
    T.run_golden_eval(dev())


def test_segmentor_with_both_impls_hip():
    T.run_segmentor(dev())


@pytest.mark.parametrize('what', ['off', 'calls', 'grad', 'tensors', 'limits', 'split'])
def test_dispatch(what):
    getattr(T, 'run_dispatch_' + what)(dev())


def test_mit_b1_against_the_fp64_torch_path():
    """mit_b1 on [2,3,96,128] with both impls 'hip' (one call) against the fp64 'torch' path on the CPU, under the yardstick gate of the
    same run"""
    shape = (2, 3, 96, 128)
    with torch.no_grad(), TB.impl('torch'), T.impls('torch', 'torch'):
        m = TB.make(T.CPU, 'mit_b1', torch.float64).eval()
        img = R.synth_input('img', shape, seed=41, scale=1.0).double()
        want = m(img)
        with T.split_linears(), T.split_convs(T.embed_convs(m)):
            yard = m(img)
    with T.impls('hip', 'hip'), T.CallSpy(_lib.get(), T.SPY) as spy:
        outs = TS.run_backbone(dev(), 'mit_b1', shape)
    assert spy.calls == {T.SPY[0]: 1, T.SPY[1]: 0, T.SPY[2]: 0}, spy.calls
    T.report('mit_b1 96x128', [('out%d' % i, T.dist(o, w), T.gate_of(y, w)) for i, (o, w, y) in enumerate(zip(outs, want, yard))])


def test_captured_backbone_call_replays_bit_for_bit():
    """one cffm_mit_infer call (mit_b0, all four stages) on a single stream, captured with torch.cuda.graph and replayed twice with outputs
    and workspace NaN-filled before each replay, gives the bits of the eager call"""
    shape = (1, 3, 96, 72)
    m = TB.make(dev(), 'mit_b0').eval()
    x = R.synth_input('img', shape, seed=41, scale=1.0).to(dev())
    stages = [(getattr(m, 'patch_embed%d' % i), getattr(m, 'block%d' % i), getattr(m, 'norm%d' % i)) for i in range(1, 5)]
    with torch.no_grad():
        arr, keep, shapes = ops.mit_stages(x.shape, stages)
        need = _lib.get().cffm_mit_infer_ws_floats(arr, 4)
        assert need > 0
        ws = torch.zeros(need, dtype=torch.float32, device=dev())
        outs = [torch.empty(s, dtype=torch.float32, device=dev()) for s in shapes]
        first = [o.clone() for o in ops.mit_infer(x, stages, ws=ws)]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ops.mit_infer(x, stages, ws=ws, outs=outs)
        for _ in range(2):
            for o in outs:
                o.fill_(float('nan'))
            ws.fill_(float('nan'))
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(o, f) for o, f in zip(outs, first))
