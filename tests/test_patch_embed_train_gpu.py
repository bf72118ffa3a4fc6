"""The patch embedding's training forward and backward and the backbone's ``conv_impl`` switch on a real MI355X: the shared run_*(device)
bodies of tests/test_patch_embed_train.py (what is checked and why is written there) at the same shapes, plus forward and backward captured
into a HIP graph."""
import pytest
import torch

import vss_cffm_amd as V
from tests import test_patch_embed_train as T

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', list(T.CASES))
def test_case_against_the_gate(name):
    T.run_case(dev(), name)


def test_without_dx_the_other_gradients_keep_their_bits():
    T.run_without_dx(dev())


@pytest.mark.parametrize('name', ['k7_1x3x30x27_32', 'k3_2x64x12x9_160+30'])
def test_forward_is_the_inference_call(name):
    T.run_forward(dev(), name)


@pytest.mark.parametrize('name', ['k7_2x3x68x76_64', 'k3_2x64x12x9_160', 'k3_2x320x5x6_512'])
def test_poisoned_workspace_and_determinism(name):
    T.run_poison_and_determinism(dev(), name)


def test_nothing_leaks_across_images():
    T.run_no_leak(dev())


def test_refusals_enqueue_nothing():
    T.run_refusals(dev())


def test_non_contiguous_inputs():
    T.run_non_contiguous(dev())


def test_backbone_conv_impl():
    T.run_backbone(dev())


def test_backbone_convolutions_outside_the_limits():
    T.run_backbone_outside_the_limits(dev())


@pytest.mark.parametrize('name', ['k3_2x64x12x9_160', 'k7_1x3x30x27_32'])
def test_captured_calls_replay_bit_for_bit(name):
    """forward + backward captured with torch.cuda.graph (no allocation inside the library, no host round trip) and replayed twice equal
    the eager call; a replay after x changed equals the eager call on the new x (the model: tests/test_ln_train_gpu.py)"""
    m, x, dout = T.on(dev(), name)
    x = x.clone()
    with_dx = T.CASES[name][0][0] == 3
    params = (m.proj.weight, m.proj.bias, m.norm.weight, m.norm.bias)

    def eager():
        g, _ = T.autograd_grads(m, x, dout, with_dx)
        return [g[n] for n in T.NAMES if g[n] is not None]

    first = eager()
    xs = x.detach().clone().requires_grad_(with_dx)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        xs.data.copy_(x)
        out = V.overlap_patch_embed(xs, m.proj, m.norm)[0]
        grads = torch.autograd.grad(out, ((xs,) if with_dx else ()) + params, dout)
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
