"""Fused prediction on a real MI355X through the C ABI: the shared run_*(device) bodies of tests/test_predict.py (what is checked and why is
written there) at the same shapes, plus a captured call replayed from a HIP graph."""
import pytest
import torch

import vss_cffm_amd as V
from tests import test_predict as T

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('name,kind,which', [('vspw', 'normal', ('plain', 'rows')), ('vspw', 'smooth', ('rows',)), ('k19', 'normal', ('plain',)),
                                             ('k19', 'smooth', ('plain',)), ('r8', 'normal', ('plain', 'rows')), ('r8', 'smooth', ('plain',)),
                                             ('one', 'normal', ('plain', 'rows')), ('chunk', 'smooth', ('plain', 'rows'))])
def test_shapes_against_the_op_sequence(name, kind, which):
    T.run_shape(dev(), name, kind, which)


def test_identity_second_stage():
    T.run_identity(dev())


def test_smallest_and_largest_k():
    T.run_small_k(dev())


def test_errors_leave_the_outputs_untouched():
    T.run_errors(dev())


def test_clip_buffer_equals_per_map_calls():
    T.run_clip_buffer(dev())


def test_ties_go_to_the_lowest_class():
    T.run_ties(dev())


def test_flip():
    T.run_flip(dev())


def test_accumulation_over_augmentations():
    T.run_accumulate(dev())


def test_determinism_and_full_coverage():
    T.run_determinism(dev())


@pytest.mark.parametrize('name,flip', [('vspw', None), ('k19', 'horizontal')])
def test_captured_call_replays_bit_for_bit(name, flip):
    """predict captured with torch.cuda.graph (one launch, no workspace, no host round trip) and replayed twice equals the eager call; a
    replay after the logits changed equals the eager call on the new logits (the model: tests/test_kmeans_gpu.py)"""
    m, k, (h, w), mid, out = T.SHAPES[name]
    lg = T.layouts(T.make_logits(T.SHAPES[name], 'smooth'), dev())['rows']
    eager_probs = torch.empty((m, k) + tuple(out), device=dev())
    eager = V.predict(lg, mid, out, flip=flip, probs=eager_probs)
    probs = torch.full_like(eager_probs, float('nan'))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pred = V.predict(lg, mid, out, flip=flip)
        pred2 = V.predict(lg, mid, out, flip=flip, probs=probs)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pred, eager) and torch.equal(pred2, eager) and torch.equal(probs, eager_probs)
    lg.copy_(lg.flip(dims=(1,)) * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    new_probs = torch.empty_like(eager_probs)
    new = V.predict(lg, mid, out, flip=flip, probs=new_probs)
    assert torch.equal(pred, new) and torch.equal(pred2, new) and torch.equal(probs, new_probs)
    assert not torch.equal(new, eager)
