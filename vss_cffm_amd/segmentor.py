"""``EncoderDecoder_clips`` -- the reference's clip segmentor (mmseg/models/segmentors/encoder_decoder.py:295-591, base.py:76-149) under its
own registry name and constructor contract, around the MI355X head and the fused prediction kernel.

Training is plumbing: flatten the clip, run the backbone, hand the features to the head (``forward_train``).  Evaluation's tail is where
the work is: between ``decode_head.forward_test`` and the metrics the reference resizes the [B,K,h,w] logits to the input size, resizes
them again to ``ori_shape``, takes a softmax over K, flips and takes the arg-max -- three [B,K,H,W] fp32 tensors.  With
``predict_impl = 'hip'`` that tail is ONE library call (``ops.predict`` -> cffm_predict) on the head's logits where they lie: the resized
logits, the probabilities and the permute copy of the token-row logits never exist.  ``'torch'`` is the reference's op sequence in stock
PyTorch: the A/B partner in the tests and what CPU tensors get outside the emulator.

Refusals (NotImplementedError), like the heads' for non-CFFM hyper-parameters: ``test_cfg.mode == 'slide'``, a neck, an auxiliary head --
no CFFM config uses them.  The backbone is whatever ``BACKBONES`` builds: ``mit_b0`` .. ``mit_b5`` (backbone.py) as every CFFM config names them,
``init_weights(pretrained=path)`` handing the checkpoint path on to the backbone.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .head import resize
from .ops import predict
from .registry import SEGMENTORS, build_backbone, build_head


def add_prefix(inputs, prefix):
    """mmseg.core.add_prefix"""
    return {'%s.%s' % (prefix, k): v for k, v in inputs.items()}


def _cfg_get(cfg, key, default=None):
    if cfg is None:
        return default
    return cfg.get(key, default) if hasattr(cfg, 'get') else getattr(cfg, key, default)


@SEGMENTORS.register_module()
class EncoderDecoder_clips(nn.Module):
    # 'hip': resize + resize + softmax + flip + arg-max in one kernel of libcffm_hip.so for GPU tensors (it raises when the library is
    # missing or the sizes are outside the kernel's range); 'torch': the reference's op sequence (what CPU tensors and
    # align_corners=True heads get, and the A/B partner in the tests)
    predict_impl = 'hip'

    def __init__(self, backbone, decode_head, neck=None, auxiliary_head=None, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__()
        if neck is not None:
            raise NotImplementedError('EncoderDecoder_clips: no CFFM config has a neck')
        if auxiliary_head is not None:
            raise NotImplementedError('EncoderDecoder_clips: no CFFM config has an auxiliary head')
        self.backbone = build_backbone(backbone)
        self.decode_head = build_head(decode_head)
        self.align_corners = self.decode_head.align_corners
        self.num_classes = self.decode_head.num_classes
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self._test_mode()
        self.init_weights(pretrained=pretrained)

    def _test_mode(self):
        mode = _cfg_get(self.test_cfg, 'mode', 'whole')
        if mode == 'slide':
            raise NotImplementedError("EncoderDecoder_clips: test_cfg.mode='slide' is not implemented (every CFFM config tests in 'whole' mode)")
        if mode != 'whole':
            raise AssertionError("test_cfg.mode must be 'slide' or 'whole', got %r" % (mode,))
        return mode

    def init_weights(self, pretrained=None):
        if hasattr(self.backbone, 'init_weights'):
            self.backbone.init_weights(pretrained=pretrained)
        self.decode_head.init_weights()

    # ------------------------------------------------------------------------------------------ training
    def extract_feat(self, img):
        return self.backbone(img)

    def forward_train(self, img, img_metas, gt_semantic_seg):
        """img [B,T,3,H,W], gt_semantic_seg [B,T,1,H,W] -> {'decode.loss_seg', 'decode.acc_seg'} (encoder_decoder.py:420-454)"""
        assert img.dim() == 5, 'a clip batch [B,T,3,H,W] expected'
        batch_size, num_clips, _, h, w = img.size()
        x = self.extract_feat(img.reshape(batch_size * num_clips, -1, h, w))
        return add_prefix(self.decode_head.forward_train(x, img_metas, gt_semantic_seg, self.train_cfg, batch_size, num_clips), 'decode')

    # ------------------------------------------------------------------------------------------ evaluation
    def _head_logits(self, img, img_metas, batch_size, num_clips):
        """[B,K,h,w] logits of the clip's last frame, as the head leaves them (token rows viewed as [B,K,h,w] on the rows path)"""
        return self.decode_head.forward_test(self.extract_feat(img), img_metas, self.test_cfg, batch_size, num_clips)

    def _fused(self, logits):
        return (self.predict_impl == 'hip' and (logits.is_cuda or _lib._override is not None) and logits.dtype == torch.float32
                and not self.align_corners)

    def encode_decode(self, img, img_metas, batch_size, num_clips):
        """logits resized to the input size [B,K,H,W] (encoder_decoder.py:367-378)"""
        out = self._head_logits(img, img_metas, batch_size, num_clips)
        return resize(out, size=img.shape[2:], mode='bilinear', align_corners=self.align_corners)

    def whole_inference(self, img, img_meta, rescale, batch_size, num_clips):
        seg_logit = self.encode_decode(img, img_meta, batch_size, num_clips)
        if rescale:
            seg_logit = resize(seg_logit, size=img_meta[0]['ori_shape'][:2], mode='bilinear', align_corners=self.align_corners)
        return seg_logit

    @staticmethod
    def _sizes(img, img_meta, rescale):
        """(input size, ori_shape or None, flip direction or None) of one augmentation (encoder_decoder.py:535-550)"""
        ori_shape = img_meta[0]['ori_shape']
        assert all(m['ori_shape'] == ori_shape for m in img_meta)
        flip = None
        if img_meta[0].get('flip', False):
            flip = img_meta[0]['flip_direction']
            assert flip in ('horizontal', 'vertical')
        return tuple(img.shape[2:]), (tuple(ori_shape[:2]) if rescale else None), flip

    def _probs_torch(self, logits, size, ori, flip):
        """the reference's op sequence: resize, resize, softmax, flip"""
        seg_logit = resize(logits, size=size, mode='bilinear', align_corners=self.align_corners)
        if ori is not None:
            seg_logit = resize(seg_logit, size=ori, mode='bilinear', align_corners=self.align_corners)
        output = F.softmax(seg_logit, dim=1)
        if flip is not None:
            output = output.flip(dims=(3,) if flip == 'horizontal' else (2,))
        return output

    def inference(self, img, img_meta, rescale, batch_size, num_clips, out=None, accumulate=False):
        """softmax probabilities [B,K,H,W] at ori_shape, flipped back (encoder_decoder.py:518-552).  `out` / `accumulate`: write or add
        them into a caller's buffer (aug_test's in-place sum) -- on the 'hip' path inside the kernel."""
        self._test_mode()
        size, ori, flip = self._sizes(img, img_meta, rescale)
        logits = self._head_logits(img, img_meta, batch_size, num_clips)
        if self._fused(logits):
            shape = (logits.shape[0], logits.shape[1]) + (ori or size)
            if out is None:
                out, accumulate = torch.empty(shape, dtype=torch.float32, device=logits.device), False
            predict(logits, size, ori, flip, probs=out, accumulate=accumulate, want_pred=False)
            return out
        output = self._probs_torch(logits, size, ori, flip)
        if out is None:
            return output
        return out.add_(output) if accumulate else out.copy_(output)

    @staticmethod
    def _clip(img):
        """a list of T frame batches [B,3,H,W] (or a clip batch [B,T,3,H,W]) -> ([B*T,3,H,W], B, T)  (encoder_decoder.py:556-561)"""
        if not torch.is_tensor(img):
            img = torch.stack(list(img), dim=1)
        assert img.dim() == 5, 'a clip [B,T,3,H,W] expected'
        batch_size, num_clips, _, h, w = img.size()
        return img.reshape(batch_size * num_clips, -1, h, w), batch_size, num_clips

    @staticmethod
    def _maps(seg_pred, to_numpy):
        return list(seg_pred.cpu().numpy()) if to_numpy else seg_pred

    def simple_test(self, img, img_meta, rescale=True, to_numpy=True):
        """Label maps of the clip's last frame: the reference's list of [H,W] numpy maps, or with to_numpy=False the int64 [B,H,W] device
        tensor that evaluation.intersect_and_union / video_consistency take as it is (encoder_decoder.py:554-572).  'hip': head eval
        forward -> one ops.predict call."""
        self._test_mode()
        img, batch_size, num_clips = self._clip(img)
        size, ori, flip = self._sizes(img, img_meta, rescale)
        logits = self._head_logits(img, img_meta, batch_size, num_clips)
        if self._fused(logits):
            return self._maps(predict(logits, size, ori, flip), to_numpy)
        return self._maps(self._probs_torch(logits, size, ori, flip).argmax(dim=1), to_numpy)

    def aug_test(self, imgs, img_metas, rescale=True, to_numpy=True):
        """Test-time augmentation: the probabilities of every augmentation (its own scale / flip, all rescaled to ori_shape) summed in ONE
        buffer, then the arg-max (encoder_decoder.py:574-591; the mean the reference takes first does not change it)."""
        assert rescale, 'aug_test rescales every augmentation back to ori_shape'
        total = None
        for i, (img, meta) in enumerate(zip(imgs, img_metas)):
            img, batch_size, num_clips = self._clip(img)
            total = self.inference(img, meta, rescale, batch_size, num_clips, out=total, accumulate=i > 0)
        return self._maps(total.argmax(dim=1), to_numpy)

    def forward_test(self, imgs, img_metas, **kwargs):
        """imgs / img_metas: the outer list runs over the test-time augmentations (base.py:76-117)"""
        for var, name in ((imgs, 'imgs'), (img_metas, 'img_metas')):
            if not isinstance(var, list):
                raise TypeError('%s must be a list, but got %s' % (name, type(var)))
        if len(imgs) != len(img_metas):
            raise ValueError('num of augmentations (%d) != num of image meta (%d)' % (len(imgs), len(img_metas)))
        for img_meta in img_metas:
            for key in ('ori_shape', 'img_shape', 'pad_shape'):
                vals = [m[key] for m in img_meta if key in m]
                assert all(v == vals[0] for v in vals)
        if len(imgs) == 1:
            return self.simple_test(imgs[0], img_metas[0], **kwargs)
        return self.aug_test(imgs, img_metas, **kwargs)

    def forward(self, img, img_metas, return_loss=True, **kwargs):
        """return_loss=True: img / img_metas single-nested -> forward_train; False: double-nested -> forward_test (base.py:135-149)"""
        if return_loss:
            return self.forward_train(img, img_metas, **kwargs)
        return self.forward_test(img, img_metas, **kwargs)
