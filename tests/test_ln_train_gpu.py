"""The LayerNorm backwards and the backbone's ``norm_impl`` switch on a real MI355X: the shared run_*(device) bodies of
tests/test_ln_train.py (what is checked and why is written there) at the same shapes, plus forward and backward of each form captured
into a HIP graph."""
import pytest
import torch

from tests import test_ln_train as T

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('form,shape', T.CASES, ids=T.IDS)
def test_shapes_against_the_stock_sequence(form, shape):
    T.run_shape(dev(), form, shape)


@pytest.mark.parametrize('form,shape', [('rows', (7, 36)), ('rows', (5, 260)), ('from_nchw', (2, 160, 6, 5)), ('to_nchw', (2, 160, 6, 5))])
def test_forward_is_the_inference_call(form, shape):
    T.run_forward(dev(), form, shape)


@pytest.mark.parametrize('form', T.FORMS)
def test_poisoned_workspace_and_determinism(form):
    for shape in ((70, 16), (5, 260)) if form == 'rows' else ((2, 64, 9, 9), (1, 260, 3, 3)):
        T.run_poison_and_determinism(dev(), form, shape)


@pytest.mark.parametrize('form', ('from_nchw', 'to_nchw'))
def test_nothing_leaks_across_images(form):
    T.run_no_leak(dev(), form)


def test_errors_leave_the_outputs_untouched():
    T.run_errors(dev())


@pytest.mark.parametrize('form,shape', [('rows', (33, 160)), ('from_nchw', (2, 64, 9, 9)), ('to_nchw', (2, 160, 6, 5))])
def test_non_contiguous_inputs(form, shape):
    T.run_non_contiguous(dev(), form, shape)


def test_backbone_norm_impl():
    T.run_backbone(dev())


def test_backbone_norms_outside_the_limits():
    T.run_backbone_outside_the_limits(dev())


@pytest.mark.parametrize('form,shape', [('rows', (70, 16)), ('from_nchw', (2, 64, 9, 9)), ('to_nchw', (1, 260, 3, 3))])
def test_captured_calls_replay_bit_for_bit(form, shape):
    """forward + backward captured with torch.cuda.graph (no allocation inside the library, no host round trip) and replayed twice equal
    the eager call; a replay after x changed equals the eager call on the new x (the model: tests/test_mixffn_gpu.py)"""
    fn, _, hw = T.fn_of(form, shape)
    x, gamma, beta, dout = T.on(dev(), form, shape)
    x = x.clone()

    def eager():
        out, g = T.autograd_grads(form, shape, x, gamma, beta, dout)
        return out, g['dx'], g['dgamma'], g['dbeta']

    first = eager()
    xs, gs, bs = (t.detach().clone().requires_grad_(True) for t in (x, gamma, beta))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        xs.data.copy_(x)
        out = fn(xs, gs, bs, *hw, eps=T.EPS)
        grads = torch.autograd.grad(out, (xs, gs, bs), dout)
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
    assert not torch.equal(second[1], first[1])
