"""``ClipStream`` -- streaming video inference around ``EncoderDecoder_clips``: push the frames of a video one at a time, get each frame's
label map.

The clip path (``simple_test``) segments target frame i from the clip ``data.clip_indices_test(i, n)``, normally [i-9, i-6, i-3, i], and
sends all four frames through the backbone and the SegFormer embedding: walking a video, every frame is encoded four times.  In eval mode
nothing in front of the CFFM layer depends on the clip -- the backbone, the four embeddings, ``linear_fuse`` (conv, BatchNorm with running
statistics, ReLU) and the 1/4 -> 1/8 resize act on each frame alone -- and all the layer needs of a frame is its [h/2*w/2, 256] stack rows.
So here a frame is encoded ONCE and its rows are kept in a ring on the device; the layer reads its four frames out of the ring where they
lie (``cffm_layer_infer_rows_ring``), addressed through a 16-byte table in device memory.

Contract: the result of ``push`` equals ``simple_test`` on the clip of the frames pushed so far IF the backbone's output for a frame does
not depend on the other frames of its batch.  That holds mathematically for every backbone here (no batch statistics in eval mode); bit for
bit it holds where the backbone's kernels pick the same tiles at N = 1 as at N = 4 -- the tests use a backbone that runs sample by sample,
and compare against the clip path under the arg-max rule of tests/test_predict.py otherwise.

Offline work has its frames at hand: ``push_many`` takes the next M frames of ONE video and runs the backbone once on the M frames, one
``cffm_segfuse_pool_fwd_frames`` (a slot per frame) and one ``cffm_layer_infer_rows_ring_tables`` (a clip table per target), in chunks of at
most ``max_chunk`` frames.  Frame j lives in slot j % R whichever call wrote it, so ``push`` and ``push_many`` may be mixed on one stream.

Not streamed: test-time flips and multi-scale testing (``aug_test``), sliding-window testing.
"""
import torch

from . import data
from .head import resize
from .ops import predict


class ClipStream:
    # 'hip': the frame's eval tail in one pass into the ring (head.stream_rows) and the layer on the ring (head.forward_stream) -- applies
    # when the head's rows path does (`_rows_path_ok`) and align_corners is false; 'torch' (and whatever 'hip' does not cover): the same
    # cache kept with stock ops -- per-frame resize(_fuse(...)) maps, then decoder_focal and _clip_logits.  The A/B partner in the tests.
    stream_impl = 'hip'

    def __init__(self, segmentor, dilation=data.DILATION, max_chunk=1):
        dilation = tuple(int(d) for d in dilation)
        if not dilation or max(dilation) >= 0:
            raise ValueError('ClipStream: the reference frames lie in the past (negative dilation), got %r' % (dilation,))
        head = segmentor.decode_head
        if len(dilation) + 1 != 4 or head.num_clips != 4:
            raise NotImplementedError('ClipStream: the CFFM layer takes 3 reference frames + the target (num_clips = 4)')
        if not getattr(head, 'can_stream', False):
            raise NotImplementedError('%s has no streaming forward' % type(head).__name__)
        max_chunk = int(max_chunk)
        if max_chunk < 1:
            raise ValueError('ClipStream: max_chunk >= 1 expected, got %r' % (max_chunk,))
        self.segmentor, self.dilation, self.max_chunk = segmentor, dilation, max_chunk
        # frame j lives in slot j % R until frame j + R replaces it; a chunk writes its max_chunk frames before the first of them reads
        # its clip, so the ring holds max_chunk - 1 frames more than a clip reaches back (max_chunk = 1: R = 1 - min(dilation) = 10)
        self.slots_in_ring = (1 - min(dilation)) - 1 + max_chunk
        self._ring = self._maps = self._slots = self._many = self.last_logits = None
        self.reset()

    def reset(self):
        """start a new video (the ring keeps its memory: every slot a clip reads has been rewritten by then)"""
        self.count = 0
        self._batch = None          # the B of the frames pushed since (push_many takes B = 1 streams only)

    # ---- the two caches -------------------------------------------------------------------------------------------------------------
    def _hip_ok(self, feats):
        head = self.segmentor.decode_head
        return self.stream_impl == 'hip' and head._rows_path_ok(feats) and not head.align_corners

    def _same_video(self, cache, shape, dev):
        """whether `cache` can take this frame; a frame of another size in the middle of a video is the caller's mistake"""
        if cache is not None and tuple(cache.shape) == tuple(shape) and cache.device == dev:
            return True
        if self.count:
            raise RuntimeError('ClipStream: frame %d has another size (or takes another stream_impl) than the frames before it; '
                               'call reset() between videos' % self.count)
        return False

    def _ring_for(self, b, h2, w2, dev):
        shape = (self.slots_in_ring, b, h2 * w2, 256)
        if not self._same_video(self._ring, shape, dev):
            self._ring = torch.zeros(shape, dtype=torch.float32, device=dev)
            self._slots = torch.zeros(4, dtype=torch.int32, device=dev)
            self._many = torch.zeros(5 * self.max_chunk, dtype=torch.int32, device=dev)      # a chunk's slots [m] | its clip tables [m,4]
        return self._ring

    def _table(self, frames, dev):
        """the slots of `frames` -> the device table, by a stream-ordered copy (the kernels enqueued behind it read the new entries)"""
        host = torch.tensor([f % self.slots_in_ring for f in frames], dtype=torch.int32)
        self._slots.copy_(host, non_blocking=True)
        return self._slots

    # ---- one frame ------------------------------------------------------------------------------------------------------------------
    def push(self, img, img_meta, rescale=True, to_numpy=True):
        """img [B,3,H,W]: the next frame of B videos; img_meta: its B meta dicts.  Returns what ``simple_test`` returns for the clip
        ``data.clip_indices_test(i, i + 1, dilation)`` of the frames pushed since ``reset()``, i counting them from 0."""
        seg = self.segmentor
        head = seg.decode_head
        assert img.dim() == 4, 'one frame batch [B,3,H,W] expected'
        assert not any(m.get('flip', False) for m in img_meta), 'ClipStream does not stream test-time flips (use aug_test)'
        if seg.training:
            raise RuntimeError('ClipStream is inference: call segmentor.eval() first')
        seg._test_mode()
        i = self.count
        frames = data.clip_indices_test(i, i + 1, list(self.dilation))
        size, ori, _ = seg._sizes(img, img_meta, rescale)
        b = img.shape[0]
        with torch.no_grad():
            feats = seg.extract_feat(img)
            picked = head._transform_inputs(feats)
            h, w = picked[0].shape[2:]
            dev = img.device
            full = len(frames) == head.num_clips
            if self._hip_ok(feats):
                ring = self._ring_for(b, h // 2, w // 2, dev)
                self._maps = None
                # one table per push: the clip's slots with the target last -- entry 3 is where this frame's rows go (a short clip: the
                # target alone, four times)
                slots = self._table(frames if full else [i] * 4, dev)
                head.stream_rows(feats, ring, slots, 3)
                if full:
                    logits = head.forward_stream(ring, slots, h, w, img_meta)
                else:
                    logits = head.forward_test(feats, img_meta, seg.test_cfg, b, 1)       # the head's short-circuit: the target alone
            else:
                small = resize(head._fuse(feats), size=(int(h / 2), int(w / 2)), mode='bilinear', align_corners=False)
                shape = (self.slots_in_ring,) + tuple(small.shape)
                if not self._same_video(self._maps, shape, dev):
                    self._maps = torch.zeros(shape, dtype=small.dtype, device=dev)
                self._ring = None
                self._maps[i % self.slots_in_ring] = small
                if full:
                    stack = torch.stack([self._maps[f % self.slots_in_ring] for f in frames], dim=1)
                    logits = head._stream_tail_torch(stack, (h, w), img_meta)
                else:
                    logits = head.forward_test(feats, img_meta, seg.test_cfg, b, 1)
            self.last_logits = logits        # [B,K,h,w], as the head left them (the tests compare them bit for bit)
            self.count, self._batch = i + 1, b
            if seg._fused(logits):
                return seg._maps(predict(logits, size, ori, None), to_numpy)
            return seg._maps(seg._probs_torch(logits, size, ori, None).argmax(dim=1), to_numpy)

    # ---- a chunk of frames ----------------------------------------------------------------------------------------------------------
    def _tables_many(self, first, m):
        """frames first .. first + m - 1 (all with full clips): their slots and clip tables -> the device, by ONE stream-ordered copy"""
        r, mc = self.slots_in_ring, self.max_chunk
        host = torch.zeros(5 * mc, dtype=torch.int32)
        for n in range(m):
            host[n] = (first + n) % r
            clip = data.clip_indices_test(first + n, first + n + 1, list(self.dilation))
            host[mc + 4 * n:mc + 4 * n + 4] = torch.tensor([f % r for f in clip], dtype=torch.int32)
        self._many.copy_(host, non_blocking=True)
        return self._many[:m], self._many[mc:mc + 4 * m].view(m, 4)

    def _push_chunk(self, imgs, meta, rescale):
        """m <= max_chunk frames whose clips are full: one backbone call, one stream_rows_many, one forward_stream_many, one predict"""
        seg = self.segmentor
        head = seg.decode_head
        i, m, r = self.count, imgs.shape[0], self.slots_in_ring
        size, ori, _ = seg._sizes(imgs, meta, rescale)
        clips = [data.clip_indices_test(i + n, i + n + 1, list(self.dilation)) for n in range(m)]
        assert all(len(c) == head.num_clips for c in clips)
        with torch.no_grad():
            feats = seg.extract_feat(imgs)
            picked = head._transform_inputs(feats)
            h, w = picked[0].shape[2:]
            dev = imgs.device
            if self._hip_ok(feats):
                ring = self._ring_for(1, h // 2, w // 2, dev)[:, 0]                    # [R, h2*w2, 256]: single frames
                self._maps = None
                slots, tables = self._tables_many(i, m)
                head.stream_rows_many(feats, ring, slots)
                logits = head.forward_stream_many(ring, tables, h, w, meta * m)
            else:
                small = resize(head._fuse(feats), size=(int(h / 2), int(w / 2)), mode='bilinear', align_corners=False)
                shape = (r, 1) + tuple(small.shape[1:])
                if not self._same_video(self._maps, shape, dev):
                    self._maps = torch.zeros(shape, dtype=small.dtype, device=dev)
                self._ring = None
                for n in range(m):
                    self._maps[(i + n) % r] = small[n:n + 1]
                stack = torch.stack([torch.cat([self._maps[f % r] for f in c], dim=0) for c in clips], dim=0)     # [m,4,256,h2,w2]
                logits = head._stream_tail_torch(stack, (h, w), meta * m)
            self.count, self._batch = i + m, 1
            if seg._fused(logits):
                return logits, predict(logits, size, ori, None)
            return logits, seg._probs_torch(logits, size, ori, None).argmax(dim=1)

    def push_many(self, imgs, img_metas, rescale=True, to_numpy=True):
        """imgs [M,3,H,W]: the next M frames of ONE video; img_metas: the video's meta dict (a list of one), or one per frame.  Returns what
        M successive ``push`` calls of the frames return: a list of M label maps, or with ``to_numpy=False`` an int64 [M,H,W] tensor;
        ``last_logits`` is [M,K,h,w].  Frames whose clips are short (the first three of a video) go through ``push`` one by one; the others
        in chunks of at most ``max_chunk`` frames -- per chunk one backbone call, one ``stream_rows_many``, one ``forward_stream_many``, one
        ``predict``.  May be mixed with ``push`` of single frames ([1,3,H,W]) on the same stream."""
        seg = self.segmentor
        head = seg.decode_head
        assert imgs.dim() == 4, 'the frames of one video [M,3,H,W] expected'
        m_all = imgs.shape[0]
        assert len(img_metas) in (1, m_all), 'one meta for the video, or one per frame'
        assert not any(m.get('flip', False) for m in img_metas), 'ClipStream does not stream test-time flips (use aug_test)'
        if seg.training:
            raise RuntimeError('ClipStream is inference: call segmentor.eval() first')
        if self.count and self._batch != 1:
            raise RuntimeError('ClipStream: push_many takes the frames of ONE video, this stream has been pushed with B = %d; '
                               'call reset() first' % self._batch)
        seg._test_mode()
        meta_of = lambda j: [img_metas[j if len(img_metas) == m_all else 0]]
        logits, preds, j = [], [], 0
        while j < m_all:
            if self.count < head.num_clips - 1:                     # a short clip: the head's short-circuit on the target alone
                preds.append(self.push(imgs[j:j + 1], meta_of(j), rescale, to_numpy=False))
                logits.append(self.last_logits)
                j += 1
                continue
            m = min(self.max_chunk, m_all - j)
            lg, pred = self._push_chunk(imgs[j:j + m], meta_of(j), rescale)
            logits.append(lg)
            preds.append(pred)
            j += m
        if not preds:
            raise ValueError('push_many: no frames')
        self.last_logits = torch.cat(logits, dim=0)                 # [M,K,h,w], as the head left them
        return seg._maps(torch.cat(preds, dim=0), to_numpy)
