"""``EncoderDecoder_clips`` (vss_cffm_amd/segmentor.py) on one toy input through the emulator; the GPU twin is tests/test_segmentor_gpu.py and
shares the run_*(device) bodies below.  A toy backbone (four maps with MiT-B0's channel counts at strides 4 .. 32) registered in BACKBONES,
the B0 head of configs/cffm_b0_64.py, a [1,4,3,64,64] clip, ori_shape (60, 67).  'hip' (one cffm_predict call) is held against 'torch' (the
reference's op sequence on the same logits) under the arg-max rule of tests/test_predict.py."""
import contextlib
import io
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import vss_cffm_amd as V
from tests import emu
from tests import test_predict as TP
from tests.test_kmeans import CallSpy
from vss_cffm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORI = (60, 67)
B0 = (32, 64, 160, 256)


class ToyBackbone(nn.Module):
    """[N,3,H,W] -> four maps: average pooling to strides 4 / 8 / 16 / 32, then a seeded 1x1 convolution to MiT-B0's widths"""

    def __init__(self, chans=B0, strides=(4, 8, 16, 32), seed=5):
        super().__init__()
        self.strides = strides
        self.convs = nn.ModuleList([nn.Conv2d(3, c, 1) for c in chans])
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g))

    def init_weights(self, pretrained=None):
        pass

    def forward(self, x):
        return [conv(F.avg_pool2d(x, s)) for conv, s in zip(self.convs, self.strides)]


V.BACKBONES.register_module(name='ToyBackbone', force=True, module=ToyBackbone)


def make_clip(t=4, size=64, seed=9):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1, 3, size, size, generator=g) for _ in range(t)]


def meta(size=64, flip=None):
    return [dict(ori_shape=ORI + (3,), img_shape=(size, size, 3), pad_shape=(size, size, 3), flip=flip is not None, flip_direction=flip,
                 filename='data/vid0/origin/0001.jpg')]


def build(device, **over):
    from oracle import recipe as R
    from vss_cffm_amd import head as Hd
    model = V.Config.fromfile(os.path.join(ROOT, 'configs', 'cffm_b0_64.py')).model.copy()
    model['backbone'] = dict(type='ToyBackbone')          # (the config names no backbone: MiT is outside this package)
    model.update(over)
    seg = V.build_segmentor(model, test_cfg=model.pop('test_cfg', dict(mode='whole')))
    assert isinstance(seg, V.segmentor.EncoderDecoder_clips) and seg.num_classes == 124 and seg.align_corners is False
    assert not seg.decode_head.load_state_dict(R.synth_state(seg.decode_head, seed=30), strict=False).unexpected_keys
    if device.type == 'cpu':
        Hd.revert_sync_batchnorm(seg)                      # as tests/test_boundary.py::_my_head does
    return seg.to(device).eval()


def logits_of(seg, frames, metas):
    img, b, t = seg._clip(frames)
    return seg._head_logits(img, metas, b, t), tuple(img.shape[2:])


def run_simple_test(device, t=4):
    lib = _lib.get()
    seg = build(device)
    frames = [f.to(device) for f in make_clip(t)]
    head_forward, left = seg._head_logits, []
    seg._head_logits = lambda *a: left.append(head_forward(*a)) or left[-1]
    with torch.no_grad(), TP.ArgSpy(lib) as ptrs:
        seg.simple_test(frames, meta(), to_numpy=False)
    del seg._head_logits
    assert left[0].stride(1) == 1 and not left[0].is_contiguous(), 'the rows path leaves token rows viewed as [B,K,h,w]'
    assert ptrs.ptrs == [left[0].data_ptr()], "the head's logits reach the library where they lie (no copy)"
    with torch.no_grad(), CallSpy(lib, 'cffm_predict') as spy:
        pred = seg.simple_test(frames, meta(), to_numpy=False)
        assert spy.n['cffm_predict'] == 1, 'simple_test is the head forward + ONE prediction call'
        maps = seg.forward([frames], [meta()], return_loss=False)          # a single augmentation is simple_test
        assert spy.n['cffm_predict'] == 2
        seg.predict_impl = 'torch'
        want = seg.simple_test(frames, meta(), to_numpy=False)
        assert spy.n['cffm_predict'] == 2
        logits, size = logits_of(seg, frames, meta())
    assert pred.dtype == torch.int64 and pred.shape == (1,) + ORI and pred.device.type == device.type
    assert isinstance(maps, list) and len(maps) == 1 and maps[0].shape == ORI and (torch.from_numpy(maps[0]) == pred[0].cpu()).all()
    assert logits.shape[1:] == (124, 16, 16)
    values = TP.op_sequence(logits.contiguous(), size, ORI)[0].cpu()
    TP.check_argmax(pred, values, want.cpu(), float(logits.abs().max()), 'simple_test, %d frames' % t)
    return seg, pred


def run_feeds_the_metrics(device):
    seg, pred = run_simple_test(device)
    g = torch.Generator().manual_seed(4)
    label = torch.randint(0, 124, pred.shape, generator=g)
    label[torch.rand(pred.shape, generator=g) < 0.1] = 255
    inter, union, area_pred, area_label = V.evaluation.intersect_and_union(pred, label.to(device), 124, 255)
    keep = label != 255
    assert int(area_label.sum()) == int(keep.sum()) and int(area_pred.sum()) == int(keep.sum())
    assert int(inter.sum()) == int(((pred.cpu() == label) & keep).sum())
    assert torch.equal(area_pred.cpu(), torch.bincount(pred.cpu()[keep], minlength=124))


def run_aug_test(device):
    """two scales and a flip: 64 px, 48 px, 64 px flipped horizontally; every augmentation's probabilities land in one buffer"""
    lib = _lib.get()
    seg = build(device)
    clip = make_clip()
    augs = [[f.to(device) for f in clip],
            [F.interpolate(f, size=(48, 48), mode='bilinear', align_corners=False).to(device) for f in clip],
            [f.flip(dims=(3,)).to(device) for f in clip]]
    metas = [meta(64), meta(48), meta(64, 'horizontal')]
    with torch.no_grad(), CallSpy(lib, 'cffm_predict') as spy:
        pred = seg.forward(augs, metas, return_loss=False, to_numpy=False)
        assert spy.n['cffm_predict'] == 3
        seg.predict_impl = 'torch'
        total = sum(seg.inference(seg._clip(a)[0], m, True, 1, 4) for a, m in zip(augs, metas))
        assert spy.n['cffm_predict'] == 3
    want = total.argmax(dim=1)
    assert pred.shape == (1,) + ORI
    TP.check_argmax(pred, total.cpu(), want.cpu(), float(total.abs().max()), 'aug_test, two scales and a flip')


def run_forward_train(device):
    from tests.golden.make_golden_head import labels
    seg = build(device).train()
    img = torch.stack(make_clip(), dim=1).to(device)
    out = seg(img, meta(), gt_semantic_seg=labels(1, 4, 64).to(device))
    assert set(out) == {'decode.loss_seg', 'decode.acc_seg'}
    assert out['decode.loss_seg'].requires_grad and bool(torch.isfinite(out['decode.loss_seg']))
    x = seg.extract_feat(img.flatten(0, 1))
    head_out = seg.decode_head.forward_train(x, meta(), labels(1, 4, 64).to(device), None, 1, 4)
    assert set(head_out) == {'loss_seg', 'acc_seg'}


def run_refusals():
    with pytest.raises(NotImplementedError, match='slide'):
        build(torch.device('cpu'), test_cfg=dict(mode='slide', crop_size=(32, 32), stride=(16, 16)))
    with pytest.raises(NotImplementedError, match='neck'):
        build(torch.device('cpu'), neck=dict(type='FPN'))
    with pytest.raises(NotImplementedError, match='auxiliary'):
        build(torch.device('cpu'), auxiliary_head=dict(type='FCNHead'))
    seg = build(torch.device('cpu'))
    seg.test_cfg = dict(mode='slide')
    with pytest.raises(NotImplementedError, match='slide'):
        seg.simple_test(make_clip(), meta())
    with pytest.raises(TypeError):
        seg.forward_test(make_clip()[0], meta())


# ---------------------------------------------------------------------------------------------- emulator
def test_simple_test_is_one_prediction_call():
    with emu.active():
        run_feeds_the_metrics(torch.device('cpu'))


def test_short_clip_takes_the_short_circuit():
    with emu.active():
        run_simple_test(torch.device('cpu'), t=2)


def test_aug_test_accumulates_in_one_buffer():
    with emu.active():
        run_aug_test(torch.device('cpu'))


def test_forward_train_returns_the_head_losses():
    with emu.active():
        run_forward_train(torch.device('cpu'))


def test_refusals():
    with emu.active():
        run_refusals()


def test_cpu_tensors_take_the_torch_sequence_outside_the_emulator():
    """'torch' is also what CPU tensors get when no emulator is active; ops.predict itself has no CPU fallback (tests/test_predict.py)"""
    seg = build(torch.device('cpu'))
    seg.decode_head.rows_impl = seg.decode_head.fuse_impl = 'torch'
    seg.decode_head.loss_impl = 'torch'
    lib = emu.lib()
    with torch.no_grad(), CallSpy(lib, 'cffm_predict') as spy:
        img, b, t = seg._clip(make_clip(2))
        pred = seg.simple_test(make_clip(2), meta(), to_numpy=False)
        assert spy.n['cffm_predict'] == 0 and pred.shape == (1,) + ORI
        assert torch.equal(pred, seg.inference(img, meta(), True, b, t).argmax(dim=1))
        augs, metas = [make_clip(2), [f.flip(dims=(2,)) for f in make_clip(2)]], [meta(), meta(64, 'vertical')]
        total = sum(seg.inference(seg._clip(a)[0], m, True, 1, 2) for a, m in zip(augs, metas))
        assert torch.equal(seg.aug_test(augs, metas, to_numpy=False), total.argmax(dim=1)) and spy.n['cffm_predict'] == 0
        assert seg.whole_inference(img, meta(), True, b, t).shape == (1, 124) + ORI and seg.encode_decode(img, meta(), b, t).shape == (1, 124, 64, 64)


def test_against_the_reference_segmentor():
    """the reference's own EncoderDecoder_clips, built as it stands through oracle/ref_import.py with the toy backbone in ITS registry and the
    same weights: simple_test under the arg-max rule as it is, on the 4-frame toy clip (this head on the rows path) and on a 2-frame clip (the
    short-circuit: frame logits only)"""
    from oracle import ref_import as RI
    if not RI.available():
        pytest.skip('the reference tree is not on this machine')
    RI.import_mmseg_models()
    from mmseg.models import builder
    builder.BACKBONES.register_module(name='ToyBackbone', force=True, module=ToyBackbone)
    with contextlib.redirect_stdout(io.StringIO()):
        ref = builder.build_segmentor(dict(type='EncoderDecoder_clips', backbone=dict(type='ToyBackbone'), decode_head=RI.head_cfg(),
                                           test_cfg=V.config.ConfigDict(mode='whole')))
    with emu.active():
        seg = build(torch.device('cpu'))
        ref.decode_head.load_state_dict(seg.decode_head.state_dict())
        ref.eval()
        for t in (4, 2):
            frames = make_clip(t)
            with torch.no_grad():
                pred = seg.simple_test(frames, meta(), to_numpy=False)
                want = ref.simple_test(frames, meta())
                x = ref.extract_feat(torch.stack(frames, dim=1).flatten(0, 1))
                logits = ref.decode_head.forward_test(x, meta(), ref.test_cfg, 1, t)
            values = TP.op_sequence(logits, (64, 64), ORI)[0]
            assert len(want) == 1 and want[0].shape == ORI
            TP.check_argmax(pred, values, torch.from_numpy(want[0])[None], float(logits.abs().max()),
                            'simple_test against the reference segmentor, %d frames' % t)
