"""Streaming video inference on a real MI355X: the shared run_*(device) bodies of tests/test_stream.py, and the two new library calls
captured into a HIP graph and replayed for consecutive frames with nothing but the slot table and the inputs changing."""
import ctypes as C

import pytest
import torch

from tests import test_infer as TI
from tests import test_stream as T
from vss_cffm_amd import _lib, ops

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', sorted(T.POOL_SHAPES))
def test_segfuse_pool_equals_the_two_pass_tail(name):
    T.run_segfuse_pool(name, dev())


def test_segfuse_pool_refusals():
    T.run_segfuse_pool_refusals(dev())


@pytest.mark.parametrize('name', sorted(T.LAYER_SHAPES))
def test_layer_on_the_ring_equals_the_layer_on_the_gathered_stack(name):
    T.run_layer_ring(name, dev())


def test_layer_ring_refusals():
    T.run_layer_ring_refusals(dev())


def test_stream_equals_the_composed_ops_and_the_clip_path():
    """(the per-frame lines this prints say whether the comparison with simple_test's N = 4 clip was exact on this machine)"""
    T.streamed(dev())


def test_stream_reset_and_torch_partner():
    T.run_reset_and_torch_partner(dev())


def test_stream_two_videos_at_once():
    T.run_stream(dev(), b=2, frames=5, clip_path=False)


def test_stream_cffmpp_head(tmp_path):
    T.run_stream_pp(dev(), tmp_path)


def test_stream_refusals():
    T.run_stream_refusals(dev())


def test_captured_frame_step_replays_for_consecutive_frames():
    """cffm_segfuse_pool_fwd (a 16 x 16 map -> 64 rows into the table's last slot) and cffm_layer_infer_rows_ring (the 8 x 8 layer on the
    table's four slots) captured ONCE with torch.cuda.graph -- each enqueues on the capturing stream alone -- and replayed for frames 3, 4
    and 5 of a video: between replays only the 16-byte slot table and the contents of the input map change, no pointer.  Every replay
    leaves the ring and the output the eager calls leave."""
    lib = _lib.get()
    c = T.PoolCase('n1_16x16', dev())
    h = w = 8
    depth, slots_in_ring, sf = 1, 5, c.rows * 256
    assert c.rows == h * w
    st, ring0 = T.layer_case('b1_8x8_d1')
    params = TI.flat_params(st, depth, dev())
    prepared = ops.layer_prepare(depth, params)
    need = lib.cffm_layer_infer_ws_floats(C.byref(ops.make_geom(lib, 1, h, w)))
    ring = ring0.clone().to(dev())                                       # [5,1,64,256]: frames 0..2 lie in slots 0..2
    ws = torch.full((need,), T.NAN, device=dev())
    buf, out = T.poisoned_out(1, h * w, dev())
    slots = T.table([0, 1, 2, 3], dev())
    g = torch.Generator().manual_seed(123)
    inputs = [torch.randn(c.y.shape, generator=g).to(dev()) for _ in range(3)]

    def step(ring_t, slots_t, ws_t, out_t):
        assert c.call(ring_t, sf, slots_in_ring, slots_t, 3) == 0, lib.cffm_last_error()
        ops.cffm_layer_rows_ring(ring_t, slots_t, h, w, depth, params, prepared, ws=ws_t, out=out_t)

    step(ring0.clone().to(dev()), slots, torch.empty_like(ws), torch.empty_like(out))     # warm-up: the cached device tables exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(ring, slots, ws, out)
    eager_ring = ring0.clone().to(dev())
    ring.copy_(eager_ring)                                               # (whatever the capture pass left is not part of the video)
    for k, frames in enumerate(([0, 1, 2, 3], [0, 2, 3, 4], [0, 2, 4, 5])):
        entries = [f % slots_in_ring for f in frames]
        c.y.copy_(inputs[k])
        slots.copy_(T.table(entries, dev()))
        ws.fill_(T.NAN)
        out.fill_(T.NAN)
        graph.replay()
        torch.cuda.synchronize()
        eager_out = torch.full_like(out, T.NAN)
        step(eager_ring, T.table(entries, dev()), torch.full_like(ws, T.NAN), eager_out)
        torch.cuda.synchronize()
        assert not torch.isnan(out).any() and T.same_bits(out, eager_out), 'frame %d' % frames[-1]
        assert T.same_bits(ring, eager_ring) and T.all_nan(buf[h * w:])
    assert not T.same_bits(ring, ring0.to(dev())), 'the replays wrote their frames into the ring'
