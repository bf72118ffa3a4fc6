"""The MiT backbones (vss_cffm_amd/backbone.py) on the CPU: 'torch' in stock PyTorch, 'hip' through the fiber emulator.  The GPU half is
tests/test_backbone_gpu.py and shares the run_*(device) bodies below.

Goldens (tests/golden/make_golden_mit.py): the reference's own mit_b0 in fp64, state from oracle/recipe.py seed 40, on [2,3,64,64] in
train mode (outputs, input gradient, parameter gradients) and on [1,3,96,72] in eval mode (outputs).  The reference was run with an
identity DropPath, so the module under test gets reset_drop_path(0).
Output gate: 1e-5 of max|golden| per tensor.  Gradient gate: stored with every gradient = 10 x the fp32-vs-fp64 difference of the
reference's own gradient, floored at 1e-6 of the tensor's largest element.

Measured on the CPU (largest error / gate over the tensors of a kind), 'torch' | 'hip' through the emulator:
    outputs 64x64    0.022 | 0.026        outputs 96x72    0.028 | 0.028
    input gradient   0.104 | 0.087        parameter gradients 0.119 (block1.0.mlp.fc2.bias) | 0.444 (block3.1.attn.kv.weight)
On the MI355X: outputs 0.031 | 0.029 (64x64), 0.031 | 0.031 (96x72); input gradient 0.087 | 0.104; parameter gradients 0.258
(block1.0.attn.proj.weight) | 0.330 (patch_embed4.proj.weight): the 'torch' path passes both gates there as they are.
The segmentor's head logits (mit_b0 + the B0 head through the emulator) are 1.2e-4 of max|golden| off seg_mit_b0_64.npz (gate 1e-3).
"""
import contextlib
import functools
import json
import os

import numpy as np
import pytest
import torch

import vss_cffm_amd as V
from oracle import recipe as R
from tests import emu
from vss_cffm_amd import backbone as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
VARIANTS = ('mit_b0', 'mit_b1', 'mit_b2', 'mit_b3', 'mit_b4', 'mit_b5')
OUT_GATE = 1e-5
FULL, HEAD = 16384, 4096       # parameter gradients: stored in full up to FULL elements, the first HEAD elements otherwise


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def golden_train():
    return dict(golden('mit_b0_64.npz'), **golden('mit_b0_64_grads34.npz'))


@contextlib.contextmanager
def impl(kind):
    """Mlp.dwconv_impl for the block; 'hip' on CPU tensors runs through the emulator"""
    prev = B.Mlp.dwconv_impl
    B.Mlp.dwconv_impl = kind
    try:
        yield
    finally:
        B.Mlp.dwconv_impl = prev


def make(device, kind='mit_b0', dtype=torch.float32):
    m = V.build_backbone(dict(type=kind, style='pytorch'))
    res = m.load_state_dict(R.synth_state(m, seed=40), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    m.reset_drop_path(0.)
    return m.to(device=device, dtype=dtype)


def train_pass(m, device, dtype=torch.float32):
    m.train()
    img = R.synth_input('img', (2, 3, 64, 64), seed=41, scale=1.0, dtype=dtype).to(device).requires_grad_(True)
    outs = m(img)
    sum((o * R.synth_input('w%d' % i, o.shape, seed=42, scale=1.0, dtype=dtype).to(device)).sum() for i, o in enumerate(outs)).backward()
    return outs, img.grad, {k: p.grad for k, p in m.named_parameters()}


def stored(t):
    t = t.detach().reshape(-1)
    return t if t.numel() <= FULL else t[:HEAD]


def worst(pairs):
    """pairs of (name, error, gate) -> the one with the largest error / gate"""
    name, err, gate = max(pairs, key=lambda p: p[1] / p[2])
    return name, err, gate


def check_outputs(outs, gold, tag):
    assert len(outs) == 4
    pairs = []
    for i, o in enumerate(outs):
        g = gold['out%d' % i]
        assert tuple(o.shape) == g.shape and o.is_contiguous()
        pairs.append(('out%d' % i, float((o.detach().cpu().double() - torch.from_numpy(g).double()).abs().max()), OUT_GATE * float(np.abs(g).max())))
    name, err, gate = worst(pairs)
    print('%s: outputs, worst %s err %.3e gate %.3e (%.3f of it)' % (tag, name, err, gate, err / gate))
    for name, err, gate in pairs:
        assert err <= gate, (tag, name, err, gate)


def run_golden_train(device, kind):
    gold = golden_train()
    with impl(kind):
        m = make(device)
        outs, dimg, grads = train_pass(m, device)
    check_outputs(outs, gold, '%s 64x64 train' % kind)
    e = float((dimg.cpu().double() - torch.from_numpy(gold['dimg']).double()).abs().max())
    print('%s: input gradient err %.3e gate %.3e (%.3f of it)' % (kind, e, float(gold['gate:dimg']), e / float(gold['gate:dimg'])))
    assert e <= float(gold['gate:dimg'])
    assert len(grads) == 176
    pairs = []
    for k, g in grads.items():
        want = torch.from_numpy(gold['grad:' + k]).double()
        got = stored(g).cpu().double()
        assert got.shape == want.shape, k
        pairs.append((k, float((got - want).abs().max()), float(gold['gate:' + k])))
    name, err, gate = worst(pairs)
    print('%s: parameter gradients, worst %s err %.3e gate %.3e (%.3f of it)' % (kind, name, err, gate, err / gate))
    for name, err, gate in pairs:
        assert err <= gate, (kind, name, err, gate)


def run_golden_eval(device, kind):
    with impl(kind), torch.no_grad():
        m = make(device).eval()
        outs = m(R.synth_input('img', (1, 3, 96, 72), seed=41, scale=1.0).to(device))
    assert [tuple(o.shape[2:]) for o in outs] == [(24, 18), (12, 9), (6, 5), (3, 3)]
    check_outputs(outs, golden('mit_b0_96x72.npz'), '%s 96x72 eval' % kind)
    return outs


def run_hip_vs_torch(device):
    a, b = run_golden_eval(device, 'hip'), run_golden_eval(device, 'torch')
    for i, (x, y) in enumerate(zip(a, b)):
        assert float((x - y).abs().max()) <= OUT_GATE * float(y.abs().max()), i


def run_hip_is_used(device):
    """'hip' goes through the library once per block and direction; 'torch' never does"""
    from tests.test_mixffn import CallSpy
    from vss_cffm_amd import _lib
    names = ('cffm_dwconv_gelu_fwd', 'cffm_dwconv_gelu_bwd')
    for kind, n in (('hip', 8), ('torch', 0)):
        with impl(kind), CallSpy(_lib.get(), names) as spy:
            m = make(device)
            train_pass(m, device)
        assert spy.calls == {names[0]: n, names[1]: n}, (kind, spy.calls)


SEG_HEAD = dict(type='CFFMHead_clips_resize1_8', in_channels=[32, 64, 160, 256], in_index=[0, 1, 2, 3], feature_strides=[4, 8, 16, 32],
                channels=128, dropout_ratio=0.1, num_classes=124, norm_cfg=dict(type='SyncBN', requires_grad=True), align_corners=False,
                decoder_params=dict(embed_dim=256, depths=1), loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                num_clips=4)


def build_segmentor(device):
    from vss_cffm_amd import head as Hd
    seg = V.build_segmentor(dict(type='EncoderDecoder_clips', backbone=dict(type='mit_b0', style='pytorch'), decode_head=dict(SEG_HEAD)),
                            test_cfg=dict(mode='whole'))
    assert type(seg.backbone).__name__ == 'mit_b0' and isinstance(seg.backbone, B.MixVisionTransformer)
    seg.backbone.load_state_dict(R.synth_state(seg.backbone, seed=40), strict=True)
    assert not seg.decode_head.load_state_dict(R.synth_state(seg.decode_head, seed=30), strict=False).unexpected_keys
    if device.type == 'cpu':
        Hd.revert_sync_batchnorm(seg)
    return seg.to(device)


SEG_META = [dict(ori_shape=(60, 67, 3), img_shape=(64, 64, 3), pad_shape=(64, 64, 3), flip=False, flip_direction=None,
                 filename='data/vid0/origin/0001.jpg')]


def seg_clip(device):
    return R.synth_input('clip', (1, 4, 3, 64, 64), seed=43, scale=1.0).to(device)


def run_segmentor_eval(device):
    seg = build_segmentor(device).eval()
    clip, meta = seg_clip(device), SEG_META
    want = torch.from_numpy(golden('seg_mit_b0_64.npz')['head_logits'])
    with torch.no_grad():
        logits = seg._head_logits(clip.flatten(0, 1), meta, 1, 4)
        pred = seg.simple_test([clip[:, i] for i in range(4)], meta, to_numpy=False)
    assert tuple(logits.shape) == (1, 124, 16, 16)
    rel = float((logits.cpu().double() - want.double()).abs().max() / want.double().abs().max())
    print('segmentor head logits: rel err %.3e (gate 1e-3)' % rel)
    assert rel <= 1e-3
    assert pred.dtype == torch.int64 and tuple(pred.shape) == (1, 60, 67)


def run_segmentor_train(device):
    from tests.golden.make_golden_head import labels
    seg = build_segmentor(device).train()
    clip, meta = seg_clip(device), SEG_META
    out = seg(clip, meta, gt_semantic_seg=labels(1, 4, 64).to(device))
    assert set(out) == {'decode.loss_seg', 'decode.acc_seg'}
    assert bool(torch.isfinite(out['decode.loss_seg'])) and bool(torch.isfinite(out['decode.acc_seg']).all())
    out['decode.loss_seg'].backward()
    g = seg.backbone.patch_embed1.proj.weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0


# ---------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize('kind', VARIANTS)
def test_registry_builds_every_variant_with_the_reference_keys(kind):
    want = json.load(open(os.path.join(GOLDEN, 'mit_state_dict_keys.json')))
    assert set(want) == set(VARIANTS) and kind in V.BACKBONES
    m = V.build_backbone(dict(type=kind, style='pytorch'))
    assert [[k, list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()] == want[kind]
    # load_state_dict(strict=True) from a recipe state (one tensor's storage broadcast to every shape: the keys and shapes are what
    # is checked here, the values are in the golden tests)
    flat = R.synth_tensor('flat', (max(v.numel() for v in m.state_dict().values()),), seed=40)
    res = m.load_state_dict({k: flat[:v.numel()].view(v.shape) for k, v in m.state_dict().items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_constructor_details():
    m = V.build_backbone(dict(type='mit_b1', style='pytorch', anything='ignored'))
    assert m.norm1.eps == m.block1[0].norm1.eps == m.block4[1].norm2.eps == 1e-6 and m.block1[0].attn.norm.eps == 1e-5
    assert isinstance(m.block1[0].drop_path, torch.nn.Identity) and abs(m.block4[1].drop_path.drop_prob - 0.1) < 1e-7
    rates = [getattr(m, 'block%d' % (i + 1))[j].drop_path for i in range(4) for j in range(2)][1:]
    assert all(abs(d.drop_prob - 0.1 * (k + 1) / 7) < 1e-7 for k, d in enumerate(rates))
    m.reset_drop_path(0.35)
    assert abs(m.block4[1].drop_path.drop_prob - 0.35) < 1e-7 and abs(m.block2[0].drop_path.drop_prob - 0.1) < 1e-7
    m.freeze_patch_emb()
    assert m.patch_embed1.requires_grad is False and m.patch_embed1.proj.weight.requires_grad
    # initialisation: Linear ~ truncated N(0, 0.02) (cut at +-2, as timm's default) with zero bias, LayerNorm 1 / 0, convolutions
    # N(0, sqrt(2 / fan_out)) with zero bias
    fc = m.block3[0].mlp.fc1
    assert float(fc.weight.detach().abs().max()) <= 2.0 and 0.019 < float(fc.weight.detach().std()) < 0.021 and not bool(fc.bias.any())
    assert bool((m.norm3.weight == 1).all()) and not bool(m.norm3.bias.any())
    for conv, fan_out in ((m.patch_embed2.proj, 9 * 128), (m.block1[0].attn.sr, 64 * 64), (m.block4[0].mlp.dwconv.dwconv, 9)):
        assert 0.8 < float(conv.weight.detach().std()) / (2.0 / fan_out) ** 0.5 < 1.2 and not bool(conv.bias.any())


def test_drop_path():
    d = B.DropPath(0.5)
    x = torch.ones(64, 3, 5)
    assert d.eval()(x) is x and B.DropPath(0.).train()(x) is x
    torch.manual_seed(0)
    y = d.train()(x)
    per = y.flatten(1)
    assert bool(((per == 0).all(dim=1) | (per == 2).all(dim=1)).all())
    kept = float((per[:, 0] == 2).float().mean())
    assert 0.25 < kept < 0.75


def test_against_the_live_reference_in_fp64():
    """'torch' in fp64 against the imported reference mit_b0 in fp64: outputs and all gradients within 1e-12 of each tensor's max"""
    from oracle import ref_import as RI
    if not RI.available():
        pytest.skip('the reference tree is not on this machine')
    M = RI.import_mmseg_models()
    ref = M.build_backbone(dict(type='mit_b0', style='pytorch'))
    ref.load_state_dict(R.synth_state(ref, seed=40), strict=True)
    with impl('torch'):
        mine = make(torch.device('cpu'), dtype=torch.float64)
        a = train_pass(mine, torch.device('cpu'), torch.float64)
    b = train_pass(ref.double(), torch.device('cpu'), torch.float64)
    pairs = [('out%d' % i, x, y) for i, (x, y) in enumerate(zip(a[0], b[0]))] + [('dimg', a[1], b[1])]
    assert list(a[2]) == list(b[2])
    pairs += [(k, a[2][k], b[2][k]) for k in a[2]]
    worst_rel = 0.0
    for k, x, y in pairs:
        rel = float((x.detach() - y.detach()).abs().max() / y.detach().abs().max())
        worst_rel = max(worst_rel, rel)
        assert rel <= 1e-12, (k, rel)
    print('fp64 against the live reference: worst %.2e of a tensor\'s max' % worst_rel)


@pytest.mark.parametrize('kind', ['torch', 'hip'])
def test_golden_train_64(kind):
    with emu.active():
        run_golden_train(torch.device('cpu'), kind)


@pytest.mark.parametrize('kind', ['torch', 'hip'])
def test_golden_eval_96x72(kind):
    with emu.active():
        run_golden_eval(torch.device('cpu'), kind)


def test_hip_against_torch():
    with emu.active():
        run_hip_vs_torch(torch.device('cpu'))


def test_hip_runs_the_library():
    with emu.active():
        run_hip_is_used(torch.device('cpu'))


def test_cpu_tensors_take_the_torch_sequence_outside_the_emulator():
    m = make(torch.device('cpu')).eval()
    with torch.no_grad():
        outs = m(R.synth_input('img', (1, 3, 96, 72), seed=41, scale=1.0))
    check_outputs(outs, golden('mit_b0_96x72.npz'), "'hip' on CPU tensors without the emulator")


def test_init_weights_from_a_bare_state_dict(tmp_path, capsys):
    src = make(torch.device('cpu'))
    sd = dict(src.state_dict(), **{'head.weight': torch.zeros(1000, 256), 'head.bias': torch.zeros(1000)})
    path = str(tmp_path / 'mit_b0.pth')
    torch.save(sd, path)
    m = V.build_backbone(dict(type='mit_b0'))
    assert m.init_weights() is None and m.init_weights(pretrained=None) is None
    missing, unexpected = m.init_weights(pretrained=path)
    assert missing == [] and sorted(unexpected) == ['head.bias', 'head.weight']
    assert 'head.weight' in capsys.readouterr().out
    for k, v in src.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k


def test_init_weights_from_a_model_checkpoint(tmp_path):
    src = make(torch.device('cpu'))
    sd = {'backbone.' + k: v for k, v in src.state_dict().items()}
    sd['decode_head.conv_seg.weight'] = torch.zeros(124, 128, 1, 1)
    sd['decode_head.patch_embed1.proj.weight'] = torch.full((32, 3, 7, 7), 7.0)       # a head key must not land in the backbone
    path = str(tmp_path / 'iter_160000.pth')
    torch.save({'meta': {'CLASSES': ['a', 'b']}, 'state_dict': sd}, path)
    seg = V.build_segmentor(dict(type='EncoderDecoder_clips', backbone=dict(type='mit_b0', style='pytorch'), decode_head=dict(SEG_HEAD),
                                 pretrained=path), test_cfg=dict(mode='whole'))          # EncoderDecoder_clips.init_weights passes it on
    for k, v in src.state_dict().items():
        assert torch.equal(seg.backbone.state_dict()[k], v), k
    m = V.build_backbone(dict(type='mit_b0'))
    assert m.init_weights(pretrained=path) == ([], [])


def test_segmentor_with_mit_b0_eval():
    with emu.active():
        run_segmentor_eval(torch.device('cpu'))


def test_segmentor_with_mit_b0_forward_train():
    with emu.active():
        run_segmentor_train(torch.device('cpu'))
