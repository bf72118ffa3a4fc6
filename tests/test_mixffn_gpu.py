"""The fused Mix-FFN middle on a real MI355X through the C ABI: the shared run_*(device) bodies of tests/test_mixffn.py (what is checked
and why is written there) at the same shapes, plus forward and backward captured into a HIP graph."""
import pytest
import torch

import vss_cffm_amd as V
from tests import test_mixffn as T

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', T.NAMES)
def test_shapes_against_the_op_sequence(name):
    T.run_shape(dev(), name)


def test_nothing_leaks_across_images():
    T.run_no_leak(dev())


def test_poisoned_workspace_and_determinism():
    T.run_poison_and_determinism(dev())
    T.run_poison_and_determinism(dev(), 'wide')


def test_errors_leave_the_outputs_untouched():
    T.run_errors(dev())


def test_autograd_and_no_grad():
    T.run_autograd(dev())
    T.run_autograd(dev(), 'b0s1')


@pytest.mark.parametrize('name', ['odd', 'b0s1'])
def test_captured_calls_replay_bit_for_bit(name):
    """forward + backward captured with torch.cuda.graph (no allocation inside the library, no host round trip) and replayed twice equal
    the eager call; a replay after h changed equals the eager call on the new h (the model: tests/test_predict_gpu.py)"""
    m, hh, ww, c = T.SHAPES[name]
    h, w, b, dout = T.on(dev(), T.SHAPES[name])
    h = h.clone()

    def eager():
        hg, wg, bg = (t.detach().clone().requires_grad_(True) for t in (h, w, b))
        out = V.dwconv_gelu(hg, wg, bg, hh, ww)
        out.backward(dout)
        return out.detach(), hg.grad, wg.grad, bg.grad

    first = eager()
    hs, ws, bs = (t.detach().clone().requires_grad_(True) for t in (h, w, b))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hs.data.copy_(h)
        out = V.dwconv_gelu(hs, ws, bs, hh, ww)
        grads = torch.autograd.grad(out, (hs, ws, bs), dout)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((out.detach(),) + tuple(grads), first):
            assert torch.equal(got, want)
    h.copy_(h.flip(dims=(1,)) * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    second = eager()
    for got, want in zip((out.detach(),) + tuple(grads), second):
        assert torch.equal(got, want)
    assert not torch.equal(second[0], first[0])
