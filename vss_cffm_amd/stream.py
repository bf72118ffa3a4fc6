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

    def __init__(self, segmentor, dilation=data.DILATION):
        dilation = tuple(int(d) for d in dilation)
        if not dilation or max(dilation) >= 0:
            raise ValueError('ClipStream: the reference frames lie in the past (negative dilation), got %r' % (dilation,))
        head = segmentor.decode_head
        if len(dilation) + 1 != 4 or head.num_clips != 4:
            raise NotImplementedError('ClipStream: the CFFM layer takes 3 reference frames + the target (num_clips = 4)')
        if not getattr(head, 'can_stream', False):
            raise NotImplementedError('%s has no streaming forward' % type(head).__name__)
        self.segmentor, self.dilation = segmentor, dilation
        self.slots_in_ring = 1 - min(dilation)          # frame j lives in slot j % R until frame j + R replaces it
        self._ring = self._maps = self._slots = self.last_logits = None
        self.reset()

    def reset(self):
        """start a new video (the ring keeps its memory: every slot a clip reads has been rewritten by then)"""
        self.count = 0

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
            self.count = i + 1
            if seg._fused(logits):
                return seg._maps(predict(logits, size, ori, None), to_numpy)
            return seg._maps(seg._probs_torch(logits, size, ori, None).argmax(dim=1), to_numpy)
