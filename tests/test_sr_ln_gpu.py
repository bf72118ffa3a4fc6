"""The fused spatial-reduction convolution + LayerNorm on a real MI355X through the C ABI: the shared run_*(device) bodies of
tests/test_sr_ln.py (what is checked and why, and the figures measured on the MI355X, are written there) at the same shapes, plus forward
and backward captured into a HIP graph.
"""
import pytest
import torch

import vss_cffm_amd as V
from tests import test_sr_ln as T

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', T.NAMES)
def test_shapes_against_the_op_sequence(name):
    T.run_shape(dev(), name)


@pytest.mark.parametrize('name', ('rows', 'b0s1'))
def test_backward_is_deterministic(name):
    T.run_determinism(dev(), name)


def test_autograd_matches_the_direct_call():
    T.run_autograd(dev())
    T.run_autograd(dev(), 'b0s1')


def test_call_counts():
    T.run_call_counts(dev())


def test_refusals_launch_nothing():
    T.run_refusals(dev())


@pytest.mark.parametrize('name', ['tail', 's4'])
def test_captured_calls_replay_bit_for_bit(name):
    """forward + backward captured with torch.cuda.graph (no allocation inside the library, no host round trip) and replayed twice equal
    the eager call; a replay after x changed equals the eager call on the new x (the model: tests/test_sra_attn_gpu.py)"""
    b, h, w, c, s = T.dims(T.SHAPES[name])
    ts = T.on(dev(), T.SHAPES[name])
    x, dout = ts[0].clone(), ts[5]

    def eager():
        leaves = [t.detach().clone().requires_grad_(True) for t in (x,) + ts[1:5]]
        out = V.sr_reduce(*leaves, h, w, s, T.EPS)
        out.backward(dout)
        return (out.detach(),) + tuple(t.grad for t in leaves)

    first = eager()
    leaves = [t.detach().clone().requires_grad_(True) for t in (x,) + ts[1:5]]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        leaves[0].data.copy_(x)
        out = V.sr_reduce(*leaves, h, w, s, T.EPS)
        grads = torch.autograd.grad(out, leaves, dout)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((out.detach(),) + tuple(grads), first):
            assert torch.equal(got, want)
    x.copy_(x.flip(dims=(1,)) * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    second = eager()
    for got, want in zip((out.detach(),) + tuple(grads), second):
        assert torch.equal(got, want)
    assert not torch.equal(second[0], first[0])
