"""The fused spatial-reduction attention core on a real MI355X through the C ABI: the shared run_*(device) bodies of
tests/test_sra_attn.py (what is checked and why is written there) at the same shapes, plus forward and backward captured into a HIP graph."""
import pytest
import torch

import vss_cffm_amd as V
from tests import test_sra_attn as T

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', T.NAMES)
def test_shapes_against_the_op_sequence(name):
    T.run_shape(dev(), name)


@pytest.mark.parametrize('name', ('n4100', 'k225'))
def test_backward_is_deterministic(name):
    T.run_determinism(dev(), name)


def test_autograd_matches_the_direct_call():
    T.run_autograd(dev())
    T.run_autograd(dev(), 'k405')


def test_call_counts():
    T.run_call_counts(dev())


def test_refusals_launch_nothing():
    T.run_refusals(dev())


@pytest.mark.parametrize('name', ['odd', 'k225'])
def test_captured_calls_replay_bit_for_bit(name):
    """forward + backward captured with torch.cuda.graph (no allocation inside the library, no host round trip) and replayed twice equal
    the eager call; a replay after q changed equals the eager call on the new q (the model: tests/test_mixffn_gpu.py)"""
    b, n, nk, heads, hd = T.dims(T.SHAPES[name])
    q, kv, dout = T.on(dev(), T.SHAPES[name])
    q = q.clone()

    def eager():
        qg, kvg = (t.detach().clone().requires_grad_(True) for t in (q, kv))
        out = V.sra_attention(qg, kvg, heads, hd ** -0.5)
        out.backward(dout)
        return out.detach(), qg.grad, kvg.grad

    first = eager()
    qs, kvs = (t.detach().clone().requires_grad_(True) for t in (q, kv))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        qs.data.copy_(q)
        out = V.sra_attention(qs, kvs, heads, hd ** -0.5)
        grads = torch.autograd.grad(out, (qs, kvs), dout)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((out.detach(),) + tuple(grads), first):
            assert torch.equal(got, want)
    q.copy_(q.flip(dims=(1,)) * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    second = eager()
    for got, want in zip((out.detach(),) + tuple(grads), second):
        assert torch.equal(got, want)
    assert not torch.equal(second[0], first[0])
