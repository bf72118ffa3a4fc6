"""The device-side k-means on a real MI355X at the sizes the prototype stage runs at (the emulator half and the shared run_*(device)
bodies, with what is checked and why, are in tests/test_kmeans.py): N = 14 400 (60 x 60 grid, T = 4) and 25 920 (60 x 108) at K = 100,
plus K = 8 and 128; the prototype-generating head at B1 480 x 480; a captured call replayed from a HIP graph."""
import pytest
import torch

import vss_cffm_amd as V
from tests import test_kmeans as T

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('kind,n,k', [('normal', 14400, 100), ('relu', 14400, 100), ('tight', 14400, 100), ('normal', 25920, 100),
                                      ('relu', 25920, 100), ('tight', 25920, 100), ('relu', 14400, 8), ('relu', 25920, 128),
                                      ('tight', 14400, 128), ('normal', 25920, 8)])
def test_one_step_against_the_definition(kind, n, k):
    T.run_step(dev(), kind, n, k)


@pytest.mark.parametrize('kind,n,k', [('relu', 25920, 100), ('tight', 14400, 100), ('normal', 14400, 100), ('relu', 14400, 8),
                                      ('tight', 25920, 128)])
def test_chained_steps_equal_one_call_bit_for_bit(kind, n, k):
    T.run_chain(dev(), kind, n, k)


def test_edges():
    T.run_edges(dev(), n=14400)


def test_edges_small():
    T.run_edges(dev(), n=500)


def test_head_takes_the_rows_path_b1_480():
    from tests.golden.make_golden_head import feature_maps
    from tests.golden import make_golden_head_b1 as G
    T.run_head(dev(), feature_maps(1, 4, G.SIZE, chans=G.B1, seed=71), 100, in_channels=G.B1, depths=2)


def test_head_takes_the_rows_path_b0_64():
    from tests.golden.make_golden_head import feature_maps
    T.run_head(dev(), feature_maps(1, 4, 64), 8)


@pytest.mark.parametrize('n,k', [(14400, 100), (25920, 8)])
def test_captured_call_replays_bit_for_bit(n, k):
    """kmeans with a given init captured with torch.cuda.graph (one chain on the caller's stream, no host round trip between the
    iterations) and replayed twice equals the eager call; a replay after the input changed equals the eager call on the new input"""
    x = T.make_points('relu', n, 40).to(dev())
    init = T.make_init(x, k, 41)
    eager = V.kmeans(x, k, iters=10, init=init)
    ws = V.kmeans_workspace(n, k, dev())
    ws.fill_(0xFF)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = V.kmeans(x, k, iters=10, init=init, ws=ws)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)
    x.mul_(0.5)
    init.mul_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, V.kmeans(x, k, iters=10, init=init)):
        assert torch.equal(a, b)
    assert not torch.equal(out[0], eager[0])
