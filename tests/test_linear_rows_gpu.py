"""linear_rows and the backbone's ``linear_impl`` switch on a real MI355X: the shared run_*(device) bodies of tests/test_linear_rows.py (what
is checked and why is written there) at the same shapes, plus the shape that takes the 128 x 128 forward body, and forward + backward
captured into a HIP graph."""
import pytest
import torch

import vss_cffm_amd as V
from tests import test_linear_rows as T

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', list(T.ALL))
def test_cases_against_the_split_yardstick(name):
    T.run_case(dev(), name)


def test_needs_input_grad_and_no_grad():
    T.run_needs_input_grad(dev())


def test_errors_leave_the_outputs_untouched():
    T.run_errors(dev())


def test_backbone_dispatch():
    T.run_dispatch(dev())


def test_backbone_rng_and_dropped_samples():
    T.run_rng(dev())


def test_backbone_model_against_fp64():
    T.run_model(dev())


@pytest.mark.parametrize('name', ['2x35x160x160', '3x100x128x128'])
def test_captured_calls_replay_bit_for_bit(name):
    """forward + backward captured with torch.cuda.graph (no allocation inside the library, no host round trip) and replayed twice equal
    the eager call; a replay after x changed equals the eager call on the new x (the model: tests/test_ln_train_gpu.py)"""
    t = T.on(dev(), name)
    x = t['x'].clone()

    def eager():
        leaves = [v.detach().clone().requires_grad_(True) for v in (x, t['w'], t['b'], t['r'])]
        y = V.linear_rows(*leaves, t['s'])
        return (y.detach(),) + torch.autograd.grad(y, leaves, t['dy'])

    first = eager()
    xs, ws, bs, rs = (v.detach().clone().requires_grad_(True) for v in (x, t['w'], t['b'], t['r']))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        xs.data.copy_(x)
        y = V.linear_rows(xs, ws, bs, rs, t['s'])
        grads = torch.autograd.grad(y, (xs, ws, bs, rs), t['dy'])
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((y.detach(),) + tuple(grads), first):
            assert torch.equal(got, want)
    x.copy_(x.flip(dims=(1,)) * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    second = eager()
    for got, want in zip((y.detach(),) + tuple(grads), second):
        assert torch.equal(got, want)
    assert not torch.equal(second[2], first[2])
