"""Segmenting a video in chunks on a real MI355X: the shared run_*(device) bodies of tests/test_stream_chunk.py, and the head's two chunk
calls captured into a HIP graph and replayed for consecutive chunks with nothing but the two tables and the input maps changing."""
import pytest
import torch

from tests import test_segmentor as TS
from tests import test_stream as T
from tests import test_stream_chunk as TC

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', sorted(TC.FRAME_SHAPES))
def test_segfuse_frames_equals_the_single_frame_calls(name):
    TC.run_segfuse_frames(name, dev())


def test_segfuse_frames_refusals():
    TC.run_segfuse_frames_refusals(dev())


@pytest.mark.parametrize('name', sorted(TC.LAYER_SHAPES))
def test_layer_tables_equals_the_ring_call_per_sample(name):
    TC.run_layer_tables(name, dev())


def test_layer_tables_refusals():
    TC.run_layer_tables_refusals(dev())


def test_whole_video_in_one_call_and_reset():
    """(the per-frame lines this prints say whether the comparison with frame-by-frame push was exact on this machine)"""
    TC.run_whole_video_and_reset(dev())


def test_uneven_chunks():
    TC.run_chunked(dev(), [('many', c) for c in (1, 4, 6, 8, 11)])


def test_push_and_push_many_mixed():
    TC.run_chunked(dev(), [('push', 1), ('many', 5), ('push', 1), ('many', TC.FRAMES - 7)])


def test_chunk_torch_partner():
    TC.run_torch_partner(dev())


def test_chunk_cffmpp_head(tmp_path):
    TC.run_chunk_pp(dev(), tmp_path)


def test_chunk_refusals():
    TC.run_chunk_refusals(dev())


def test_captured_chunk_step_replays_for_consecutive_chunks():
    """head.stream_rows_many (three 16 x 16 maps -> 64 rows each into the slots of the first table) and head.forward_stream_many (the 8 x 8
    layer on the three clip tables) captured ONCE with torch.cuda.graph and replayed for the chunks of frames 3..5, 6..8 and 9..11 of a
    video: between replays only the two tables and the contents of the four input maps change, no pointer.  Every replay leaves the ring
    and the logits the eager calls leave.  One chain on one stream apart from the library's own embedding branches."""
    from vss_cffm_amd import data
    m, r = 3, 12
    head = T.streaming_segmentor(dev()).decode_head
    g = torch.Generator().manual_seed(321)
    new_feats = lambda: [torch.randn(m, ch, 16 // s, 16 // s, generator=g).to(dev()) for ch, s in zip(TS.B0, (1, 2, 4, 8))]
    ring0 = torch.randn(r, 64, 256, generator=g).to(dev())               # frames 0..2 lie in slots 0..2; the others are overwritten first
    chunks = [new_feats() for _ in range(3)]
    feats = [torch.zeros_like(f) for f in chunks[0]]
    ring, slots, tables = ring0.clone(), T.table([3, 4, 5], dev()), T.table([[0, 1, 2, 3]] * m, dev())

    def step(feats_t, ring_t, slots_t, tables_t):
        head.stream_rows_many(feats_t, ring_t, slots_t)
        return head.forward_stream_many(ring_t, tables_t, 16, 16)

    with torch.no_grad():
        step(chunks[0], ring0.clone(), slots.clone(), tables.clone())     # warm-up: prepared data and cached device tables exist before the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step(feats, ring, slots, tables)
        eager_ring = ring0.clone()
        ring.copy_(eager_ring)                                            # (whatever the capture pass left is not part of the video)
        for k in range(3):
            first = 3 + m * k
            s_host = [(first + n) % r for n in range(m)]
            t_host = [[f % r for f in data.clip_indices_test(first + n, first + n + 1)] for n in range(m)]
            for dst, src in zip(feats, chunks[k]):
                dst.copy_(src)
            slots.copy_(T.table(s_host, dev()))
            tables.copy_(T.table(t_host, dev()))
            out.fill_(T.NAN)
            graph.replay()
            torch.cuda.synchronize()
            eager_out = step(chunks[k], eager_ring, T.table(s_host, dev()), T.table(t_host, dev()))
            torch.cuda.synchronize()
            assert out.shape == (m, 124, 16, 16) and not torch.isnan(out).any() and T.same_bits(out, eager_out), 'chunk %d' % k
            assert T.same_bits(ring, eager_ring)
    assert not T.same_bits(ring, ring0), 'the replays wrote their frames into the ring'
