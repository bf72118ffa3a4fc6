"""GPU half of tests/test_mit_blocks_train.py: the same bodies on the MI355X, plus the captured-graph replay of the stage call."""
import pytest
import torch

import vss_cffm_amd as V
from tests import test_mit_blocks_train as T

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('shape', T.LN_ROWS, ids=T.LN_IDS)
def test_ln_rows_bwd_add(shape):
    T.run_ln_add(dev(), shape)


def test_ln_rows_bwd_add_errors():
    T.run_ln_add_errors(dev())


@pytest.mark.parametrize('name', list(T.CASES))
def test_stage_against_the_composition(name):
    T.run_stage_case(dev(), name)


def test_stage_poisoned_buffers():
    T.run_stage_poison(dev())


def test_stage_dropped_sample():
    T.run_stage_dropped(dev())


def test_stage_needs_input_grad():
    T.run_stage_needs_grad(dev())


def test_stage_against_fp64():
    T.run_stage_anchor(dev())


def test_stage_errors():
    T.run_stage_errors(dev())


def test_backbone_block_impl():
    T.run_backbone(dev())


def test_backbone_dispatch():
    T.run_backbone_dispatch(dev())


def test_captured_calls_replay_bit_for_bit():
    """forward + backward of case a captured with torch.cuda.graph (no allocation inside the library, no host round trip) and replayed
    twice equal the eager call; a replay after x changed equals the eager call on the new x (the model: tests/test_linear_rows_gpu.py)"""
    blocks, x, dy, scales = T.stage_on(dev(), 'a')
    params = list(blocks.parameters())
    x = x.clone()

    def eager():
        xg = x.detach().clone().requires_grad_(True)
        y = V.mit_blocks_train(xg, blocks, 8, 8, scales)
        return (y.detach(),) + torch.autograd.grad(y, [xg] + params, dy)

    first = eager()
    xs = x.detach().clone().requires_grad_(True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        xs.data.copy_(x)
        y = V.mit_blocks_train(xs, blocks, 8, 8, scales)
        grads = torch.autograd.grad(y, [xs] + params, dy)
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
