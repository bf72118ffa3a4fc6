"""Streaming video inference (vss_cffm_amd.ClipStream; include/cffm_hip.h: cffm_segfuse_pool_fwd, cffm_layer_infer_rows_ring) on the CPU
through the fiber emulator.  The GPU half is tests/test_stream_gpu.py and shares the run_*(device) bodies below.

A. cffm_segfuse_pool_fwd through the raw ABI: bit-equal to cffm_segfuse_fwd + cffm_bn_relu_pool_fwd's `stack` on a copy of y.
B. cffm_layer_infer_rows_ring: bit-equal to cffm_layer_infer_rows on the stack gathered with index_select.
C. The heads and ClipStream on the toy segmentor of tests/test_segmentor.py with a backbone that runs sample by sample (batch-invariant by
   construction), an 11-frame video: the three short clips, the six hand-picked clips (i = 3..8), the first regular one and the ring wrap.

Every input is seeded; every buffer a call writes is NaN-poisoned first and has guard rows behind it."""
import ctypes as C
import functools
import os

import pytest
import torch

import vss_cffm_amd as V
from oracle import recipe as R, ref_import as RI
from tests import emu
from tests import test_infer as TI
from tests import test_predict as TP
from tests import test_segmentor as TS
from tests.test_kmeans import CallSpy
from vss_cffm_amd import _lib, data, ops

NAN = float('nan')
GUARD = 8          # guard rows behind every output


def bits(t):
    """a float tensor as its bit patterns: equality that NaNs do not defeat"""
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def all_nan(t):
    return bool(torch.isnan(t).all())


def sync(device):
    if device.type == 'cuda':
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- A. cffm_segfuse_pool_fwd
# (N, H, W, maps): the issue's shapes -- a 2 x 3 patch grid, whole ratios at more than one workgroup, non-integer ratios, one patch per
# frame with one-cell maps, and a single map (cnt = 1)
POOL_SHAPES = {
    'n2_4x6': (2, 4, 6, ((2, 3), (1, 2), (1, 1))),
    'n1_16x16': (1, 16, 16, ((8, 8), (4, 4), (2, 2))),
    'n1_6x10_ragged': (1, 6, 10, ((3, 5), (2, 3), (1, 2))),
    'n3_2x2': (3, 2, 2, ((1, 1), (1, 1), (1, 1))),
    'n2_4x6_one_map': (2, 4, 6, ((2, 3),)),
}


class PoolCase:
    """seeded operands of one shape and the reference rows (segfuse_fwd + bn_relu_pool_fwd's stack on a copy of y), computed once"""

    def __init__(self, name, device):
        self.N, self.H, self.W, self.maps = POOL_SHAPES[name]
        N, H, W = self.N, self.H, self.W
        g = torch.Generator().manual_seed(1000 + sorted(POOL_SHAPES).index(name))
        rnd = lambda *s: torch.randn(*s, generator=g)
        self.y = rnd(N * H * W, 256).to(device)
        self.d = rnd(256).to(device)
        self.z = [rnd(N * h * w, 256).to(device) for h, w in self.maps]
        # about a third of the channels with a negative scale, so that the ReLU cuts on both sides of the sums
        sign = torch.where(torch.rand(256, generator=g) < 1.0 / 3.0, -1.0, 1.0)
        self.scale = ((0.5 + torch.rand(256, generator=g)) * sign).to(device)
        self.shift = (0.5 * rnd(256)).to(device)
        self.device = device
        k = len(self.maps)
        self.zp = (C.c_void_p * 3)(*([z.data_ptr() for z in self.z] + [None] * (3 - k)))
        self.hs = (C.c_int * 3)(*([h for h, _ in self.maps] + [1] * (3 - k)))
        self.ws = (C.c_int * 3)(*([w for _, w in self.maps] + [1] * (3 - k)))
        self.rows = N * (H // 2) * (W // 2)
        lib, st = _lib.get(), ops._stream(self.y)
        y2 = self.y.clone()
        _lib.check(lib.cffm_segfuse_fwd(ops._ptr(y2), ops._ptr(self.d), self.zp, self.hs, self.ws, k, N, H, W, st), lib)
        fused = torch.full_like(y2, NAN)
        self.want = torch.full((self.rows, 256), NAN, device=device)
        _lib.check(lib.cffm_bn_relu_pool_fwd(ops._ptr(y2), ops._ptr(self.scale), ops._ptr(self.shift), None, ops._ptr(fused), ops._ptr(self.want),
                                             N, H, W, st), lib)
        sync(device)
        assert not torch.isnan(self.want).any()
        assert bool((self.want == 0).any()) and bool((self.want > 0).any()), 'the ReLU cuts somewhere and passes somewhere'
        self.kept = [self.y.clone(), self.d.clone()] + [z.clone() for z in self.z]

    def call(self, ring, slot_floats, nslots, slots, which, y=None, H=None, W=None):
        lib = _lib.get()
        y = self.y if y is None else y
        return lib.cffm_segfuse_pool_fwd(ops._ptr(y), ops._ptr(self.d), self.zp, self.hs, self.ws, len(self.maps), ops._ptr(self.scale),
                                         ops._ptr(self.shift), ops._ptr(ring) if ring is not None else None, slot_floats, nslots,
                                         ops._ptr(slots) if slots is not None else None, which, self.N, H or self.H, W or self.W,
                                         ops._stream(self.y))

    def inputs_unchanged(self):
        return all(same_bits(a, b) for a, b in zip([self.y, self.d] + self.z, self.kept))


def table(entries, device):
    return torch.tensor(entries, dtype=torch.int32).to(device)


def run_segfuse_pool(name, device):
    c = PoolCase(name, device)
    sf = c.rows * 256
    new_ring = lambda: torch.full((3 * c.rows + GUARD, 256), NAN, device=device)
    slot = lambda ring, s: ring[s * c.rows:(s + 1) * c.rows]
    # slots[which] = 2 of a 3-slot ring: the rows land in slot 2 with the reference's bits, slots 0 / 1 and the guard keep their NaNs
    ring = new_ring()
    assert c.call(ring, sf, 3, table([0, 1, 0, 2], device), 3) == 0, _lib.get().cffm_last_error()
    sync(device)
    assert same_bits(slot(ring, 2), c.want)
    assert all_nan(ring[:2 * c.rows]) and all_nan(ring[3 * c.rows:])
    assert c.inputs_unchanged(), 'y, d and the maps are only read'
    # a table entry outside the ring is clamped on the device: 7 -> slot 2, -1 -> slot 0 (documented behaviour, no fault)
    for entry, lands in ((7, 2), (-1, 0)):
        ring = new_ring()
        assert c.call(ring, sf, 3, table([entry, 1, 1, 1], device), 0) == 0
        sync(device)
        assert same_bits(slot(ring, lands), c.want)
        others = [s for s in range(3) if s != lands]
        assert all(all_nan(slot(ring, s)) for s in others) and all_nan(ring[3 * c.rows:])
    # no table: slot 0
    ring = new_ring()
    assert c.call(ring, sf, 3, None, 0) == 0
    sync(device)
    assert same_bits(slot(ring, 0), c.want) and all_nan(ring[c.rows:])
    assert c.inputs_unchanged()


def run_segfuse_pool_refusals(device):
    """odd H, odd W, a null output, output == y: an error each, before anything is enqueued -- the poisoned output stays untouched"""
    c = PoolCase('n2_4x6', device)
    lib = _lib.get()
    sf = c.rows * 256
    ring = torch.full((3 * c.rows + GUARD, 256), NAN, device=device)
    slots = table([0, 0, 0, 1], device)
    big_y = torch.randn(2 * 5 * 7, 256).to(device)                     # room for the odd sizes
    kept = big_y.clone()
    assert c.call(ring, sf, 3, slots, 3, y=big_y, H=5, W=6) != 0 and b'even' in lib.cffm_last_error()
    assert c.call(ring, sf, 3, slots, 3, y=big_y, H=4, W=7) != 0 and b'even' in lib.cffm_last_error()
    assert c.call(None, sf, 3, slots, 3) != 0 and b'null' in lib.cffm_last_error()
    y_poison = torch.full((c.N * c.H * c.W, 256), NAN, device=device)
    assert c.call(y_poison, sf, 1, slots, 3, y=y_poison) != 0 and b'overlaps' in lib.cffm_last_error()
    assert c.call(c.z[0], c.z[0].numel(), 1, slots, 3) != 0 and b'overlaps' in lib.cffm_last_error()
    assert c.call(ring.view(-1)[1:], sf, 3, slots, 3) != 0 and b'aligned' in lib.cffm_last_error()
    sync(device)
    assert all_nan(ring) and all_nan(y_poison) and same_bits(big_y, kept) and c.inputs_unchanged()
    # the Python operator validates what the host can see
    head = streaming_segmentor(device).decode_head
    feats = [torch.randn(1, ch, 16 // s, 16 // s).to(device) for ch, s in zip(TS.B0, (1, 2, 4, 8))]
    lins = (head.linear_c1, head.linear_c2, head.linear_c3, head.linear_c4)
    args = lambda: (feats, [l.proj.weight for l in lins], [l.proj.bias for l in lins], head.linear_fuse.conv.weight, head.linear_fuse.bn)
    good = torch.full((3, 1, 64, 256), NAN, device=device)
    with torch.no_grad():
        for bad_ring, bad_slots, which in ((good[:, :, :63], slots, 3), (good.double(), slots, 3), (good, slots.long(), 3), (good, slots[:3], 3),
                                           (good, slots, 4), (good.transpose(0, 1), slots, 3)):
            with pytest.raises(_lib.CffmError):
                ops.segformer_fuse_pool(*args(), bad_ring, bad_slots, which)
    with pytest.raises(_lib.CffmError, match='inference only'):
        ops.segformer_fuse_pool(*args(), good, slots, 3)                 # the parameters require grad and grad mode is on
    assert all_nan(good)


# ---------------------------------------------------------------------------------------------- B. cffm_layer_infer_rows_ring
LAYER_SHAPES = {'b1_8x8_d1': (1, 8, 8, 1), 'b2_8x8_d2': (2, 8, 8, 2), 'b1_14x21_d2': (1, 14, 21, 2)}
TABLES = ([4, 0, 2, 1], [1, 1, 3, 2])          # five slots; the second repeats one


@functools.lru_cache(maxsize=None)
def layer_case(name):
    b, h, w, depth = LAYER_SHAPES[name]
    seed = 200 + sorted(LAYER_SHAPES).index(name)
    return R.layer_state(depth, seed=seed), R.synth_input('ring', (5, b, h * w, 256), seed=seed + 50)


def poisoned_out(b, hw, device):
    buf = torch.full((b * hw + GUARD, 256), NAN, device=device)
    return buf, buf[:b * hw].view(b, hw, 256)


def run_layer_ring(name, device):
    lib = _lib.get()
    b, h, w, depth = LAYER_SHAPES[name]
    st, ring0 = layer_case(name)
    params = TI.flat_params(st, depth, device)
    prepared = ops.layer_prepare(depth, params)
    need = lib.cffm_layer_infer_ws_floats(C.byref(ops.make_geom(lib, b, h, w)))
    for entries in TABLES:
        ring = ring0.clone().to(device)
        for s in set(range(5)) - set(entries):
            ring[s] = NAN                                             # a slot the table does not name is never read
        kept = ring.clone()
        slots = table(entries, device)
        gathered = ring.index_select(0, slots.long()).transpose(0, 1).contiguous()          # [B,4,HW,256]
        want = ops.cffm_layer_rows_infer(gathered, h, w, depth, params, prepared)
        assert not torch.isnan(want).any()
        buf, out = poisoned_out(b, h * w, device)
        ws = torch.full((need + GUARD,), NAN, device=device)
        got = ops.cffm_layer_rows_ring(ring, slots, h, w, depth, params, prepared, ws=ws, out=out)
        sync(device)
        assert got.data_ptr() == out.data_ptr() and same_bits(got, want), (name, entries)
        assert all_nan(buf[b * h * w:]) and all_nan(ws[need:]) and same_bits(ring, kept), 'guards intact, the ring only read'
    # the degenerate form that IS cffm_layer_infer_rows: ring = the stack, a slot = one frame, samples 4 frames apart
    x_rows = ring0[:4].transpose(0, 1).contiguous().to(device)                              # [B,4,HW,256]
    want = ops.cffm_layer_rows_infer(x_rows, h, w, depth, params, prepared)
    buf, out = poisoned_out(b, h * w, device)
    g, (key_src, q_dst, *_) = ops._layer_geom(lib, b, h, w, device)
    ws = torch.full((need,), NAN, device=device)
    img = h * w * 256
    identity = table([0, 1, 2, 3], device)
    call = lambda ring_t, y: lib.cffm_layer_infer_rows_ring(C.byref(g), depth, ops.block_structs(params, depth), ops._ptr(prepared), ops._ptr(ring_t),
                                                            img, 4, ops._ptr(identity), 4 * img, ops._ptr(y), ops._ptr(key_src),
                                                            ops._ptr(q_dst), ops._ptr(ws), ops._stream(ring_t))
    assert call(x_rows, out) == 0, lib.cffm_last_error()
    sync(device)
    assert same_bits(out, want) and all_nan(buf[b * h * w:])


def run_layer_ring_refusals(device):
    name = 'b1_8x8_d1'
    b, h, w, depth = LAYER_SHAPES[name]
    st, ring0 = layer_case(name)
    params = TI.flat_params(st, depth, device)
    prepared = ops.layer_prepare(depth, params)
    ring = ring0.clone().to(device)
    kept = ring.clone()
    slots = table([0, 1, 2, 3], device)
    with pytest.raises(_lib.CffmError, match='inside the ring'):
        ops.cffm_layer_rows_ring(ring, slots, h, w, depth, params, prepared, out=ring[4])
    for bad_ring, bad_slots in ((ring[:, :, :63], slots), (ring, slots.long()), (ring, slots[:2]), (ring.double(), slots)):
        with pytest.raises(_lib.CffmError):
            ops.cffm_layer_rows_ring(bad_ring, bad_slots, h, w, depth, params, prepared)
    sync(device)
    assert same_bits(ring, kept)


# ---------------------------------------------------------------------------------------------- C. head and stream
class SampledToyBackbone(TS.ToyBackbone):
    """the toy backbone run sample by sample: a frame's features cannot depend on the other frames of its batch"""
    calls = 0

    def forward(self, x):
        type(self).calls += 1
        per = [TS.ToyBackbone.forward(self, x[i:i + 1]) for i in range(x.shape[0])]
        return [torch.cat(level, dim=0) for level in zip(*per)]


V.BACKBONES.register_module(name='SampledToyBackbone', force=True, module=SampledToyBackbone)
FRAMES = 11


def streaming_segmentor(device, **over):
    return TS.build(device, backbone=dict(type='SampledToyBackbone'), **over)


def make_video(b=1, n=FRAMES, seed=77):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(b, 3, 64, 64, generator=g) for _ in range(n)]


def metas(b=1):
    return [dict(TS.meta()[0], filename='data/vid%d/origin/0001.jpg' % v) for v in range(b)]


class RowSpy:
    """counts calls of one entry point and keeps one integer argument of each (CallSpy's pattern)"""

    def __init__(self, lib, name, arg):
        self.lib, self.name, self.arg, self.real, self.seen = lib, name, arg, getattr(lib, name), []

    def __enter__(self):
        def counted(*a):
            self.seen.append(int(a[self.arg]))
            return self.real(*a)
        setattr(self.lib, self.name, counted)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.real)


def composed_logits(seg, video, rows, i, mt):
    """frame i's logits as the EXISTING ops compose them, every frame encoded on its own: segformer_fuse, bn_relu_pool, torch.stack,
    forward_rows, _rows_logits (a short clip: the head's forward on the target alone).  `rows`: the per-frame stack rows, built once."""
    head = seg.decode_head
    lins = (head.linear_c1, head.linear_c2, head.linear_c3, head.linear_c4)
    frames = data.clip_indices_test(i, i + 1)
    feats = seg.extract_feat(video[i])
    if i not in rows:
        c = head._transform_inputs(feats)
        y = ops.segformer_fuse(list(c), [l.proj.weight for l in lins], [l.proj.bias for l in lins], head.linear_fuse.conv.weight)
        rows[i] = ops.bn_relu_pool(y, head.linear_fuse.bn, want_stack=True)[1]                # [B, h2*w2, 256]
    if len(frames) != 4:
        return head.forward_test(feats, mt, seg.test_cfg, video[i].shape[0], 1)
    b, (h, w) = video[i].shape[0], (16, 16)
    x_rows = torch.stack([rows[f] for f in frames], dim=1)                                    # [B,4,h2*w2,256]
    mined = head.decoder_focal.forward_rows(x_rows, h // 2, w // 2)
    x2 = head._rows_logits(head.linear_pred2, torch.cat([x_rows[:, -1], mined], dim=-1).view(b, h // 2, w // 2, -1), head.dropout, (h, w))
    if not hasattr(head, 'decoder_swin'):
        return x2.squeeze(1)
    centers = head._load_centers(mt, x2.device)
    ctx = head.decoder_swin(x_rows[:, -1].contiguous(), h // 2, w // 2, centers)[0]
    x3 = head._rows_logits(head.linear_pred3, ctx.reshape(b, h // 2, w // 2, -1), head.dropout3, (h, w))
    return x2.squeeze(1) + 0.5 * x3.squeeze(1)


def run_stream(device, b=1, frames=FRAMES, clip_path=True, seg=None):
    """ClipStream against the composition of the existing ops (bit for bit, logits and label maps) and against simple_test on the 4-frame
    clip (N = 4 GEMM tiles) under the arg-max rule of tests/test_predict.py.

    Was the comparison with simple_test also exact?  On the emulator: yes, the logits are bit-equal at every one of the 11 frames.  On the
    MI355X: yes as well, at every frame, for the base head and the CFFM++ head (at these toy shapes the library's GEMMs sum a row in one
    order whether the batch holds one frame or four).  Nothing promises that at other shapes or with another backbone: the test prints the
    answer per frame, and the arg-max rule is what it asserts."""
    lib = _lib.get()
    seg = seg or streaming_segmentor(device)
    video = [f.to(device) for f in make_video(b, frames)]
    mt = metas(b)
    stream = V.ClipStream(seg)
    assert stream.slots_in_ring == 10 and stream.stream_impl == 'hip'
    rows, maps = {}, []
    with torch.no_grad():
        for i in range(frames):
            SampledToyBackbone.calls = 0
            with CallSpy(lib, 'cffm_predict', 'cffm_bn_relu_pool_fwd', 'cffm_segfuse_pool_fwd', 'cffm_layer_infer_rows_ring') as spy, \
                    RowSpy(lib, 'cffm_linear_bias_fwd', 4) as lin:
                pred = stream.push(video[i], mt, to_numpy=False)
            assert SampledToyBackbone.calls == 1 and spy.n['cffm_predict'] == 1 and spy.n['cffm_segfuse_pool_fwd'] == 1, (i, spy.n)
            if i >= 3:
                assert spy.n['cffm_bn_relu_pool_fwd'] == 0 and spy.n['cffm_layer_infer_rows_ring'] == 1, (i, spy.n)
                assert all(m < b * 16 * 16 for m in lin.seen) and lin.seen, 'no classifier runs on the 1/4-resolution rows'
            logits = stream.last_logits
            want = composed_logits(seg, video, rows, i, mt)
            assert logits.shape == (b, 124, 16, 16) and same_bits(logits, want), 'frame %d' % i
            assert torch.equal(pred, ops.predict(want, (64, 64), TS.ORI, None)), 'frame %d' % i
            maps.append(pred.cpu())
            if clip_path:
                clip = [video[f] for f in data.clip_indices_test(i, i + 1)]
                clip_logits, size = TS.logits_of(seg, clip, mt)
                values, probs = TP.op_sequence(clip_logits.contiguous().cpu(), size, TS.ORI)
                print('frame %2d: logits bit-equal to the clip path: %s' % (i, same_bits(logits, clip_logits)))
                TP.check_argmax(pred, values, probs.argmax(dim=1), float(clip_logits.abs().max()), 'ClipStream vs simple_test, frame %d' % i)
    return seg, stream, video, mt, maps


@functools.lru_cache(maxsize=None)
def streamed(device):
    """the 11-frame run, once per device: the tests below go on from its stream and maps"""
    return run_stream(device)


def run_reset_and_torch_partner(device):
    seg, stream, video, mt, maps = streamed(device)
    lib = _lib.get()
    with torch.no_grad():
        stream.reset()
        again = [stream.push(f, mt, to_numpy=False).cpu() for f in video]
        assert all(torch.equal(a, m) for a, m in zip(again, maps)), 'after reset() the same video gives the same maps'
        partner = V.ClipStream(seg)
        partner.stream_impl = 'torch'
        for i, f in enumerate(video):
            with CallSpy(lib, 'cffm_segfuse_pool_fwd', 'cffm_layer_infer_rows_ring') as spy:
                pred = partner.push(f, mt, to_numpy=False)
            assert spy.n == {'cffm_segfuse_pool_fwd': 0, 'cffm_layer_infer_rows_ring': 0}
            lg = partner.last_logits
            values, probs = TP.op_sequence(lg.contiguous().cpu(), (64, 64), TS.ORI)
            TP.check_argmax(maps[i], values, probs.argmax(dim=1), float(lg.abs().max()), "stream_impl 'hip' vs 'torch', frame %d" % i)
            assert pred.shape == maps[i].shape
    out = V.ClipStream(seg).push(video[0], mt)                               # the reference's list of numpy maps by default
    assert isinstance(out, list) and out[0].shape == TS.ORI


def run_stream_pp(device, tmp_path):
    """the CFFM++ head once: one centers.pt under tmp_path; frames 0..4 (two short clips would do, three are there, two full ones)"""
    os.makedirs(os.path.join(str(tmp_path), 'vid0'))
    torch.save(R.synth_input('centers', (1, 8, 256), seed=35, scale=1.0), os.path.join(str(tmp_path), 'vid0', 'centers.pt'))
    seg = streaming_segmentor(device, decode_head=RI.head_cfg(kind='CFFMHead_clips_resize1_8_finetune_w_prototype3'))
    seg.decode_head.save_path = str(tmp_path) + '/'
    run_stream(device, frames=5, clip_path=True, seg=seg)


def run_stream_refusals(device):
    seg = streaming_segmentor(device)
    video, mt = [f.to(device) for f in make_video(1, 1)], metas(1)
    with pytest.raises(AssertionError, match='flip'):
        V.ClipStream(seg).push(video[0], [dict(mt[0], flip=True, flip_direction='horizontal')])
    gene = streaming_segmentor(device, decode_head=RI.head_cfg(kind='CFFMHead_clips_resize1_8_gene_prototype'))
    with pytest.raises(NotImplementedError):
        V.ClipStream(gene)
    with pytest.raises(NotImplementedError):
        gene.decode_head.stream_rows(None, None, None, 3)
    with pytest.raises(NotImplementedError):
        gene.decode_head.forward_stream(None, None, 16, 16)
    walked = V.ClipStream(seg)
    with torch.no_grad():
        walked.push(video[0], mt)
        with pytest.raises(RuntimeError, match='reset'):
            walked.push(video[0][:, :, :48, :48].contiguous(), mt)           # another size in the middle of a video
        walked.reset()
        assert walked.push(video[0][:, :, :48, :48].contiguous(), mt)[0].shape == TS.ORI      # a new video may have one
    seg.decode_head.linear_fuse.bn.train()
    with pytest.raises(_lib.CffmError, match='eval'), torch.no_grad():
        V.ClipStream(seg).push(video[0], mt)
    seg.train()
    with pytest.raises(RuntimeError, match='eval'):
        V.ClipStream(seg).push(video[0], mt)


# ---------------------------------------------------------------------------------------------- emulator
@pytest.mark.parametrize('name', sorted(POOL_SHAPES))
def test_segfuse_pool_equals_the_two_pass_tail(name):
    with emu.active():
        run_segfuse_pool(name, torch.device('cpu'))


def test_segfuse_pool_refusals():
    with emu.active():
        run_segfuse_pool_refusals(torch.device('cpu'))


@pytest.mark.parametrize('name', sorted(LAYER_SHAPES))
def test_layer_on_the_ring_equals_the_layer_on_the_gathered_stack(name):
    with emu.active():
        run_layer_ring(name, torch.device('cpu'))


def test_layer_ring_refusals():
    with emu.active():
        run_layer_ring_refusals(torch.device('cpu'))


def test_stream_equals_the_composed_ops_and_the_clip_path():
    with emu.active():
        streamed(torch.device('cpu'))


def test_stream_reset_and_torch_partner():
    with emu.active():
        run_reset_and_torch_partner(torch.device('cpu'))


def test_stream_two_videos_at_once():
    with emu.active():
        run_stream(torch.device('cpu'), b=2, frames=5, clip_path=False)


def test_stream_cffmpp_head(tmp_path):
    with emu.active():
        run_stream_pp(torch.device('cpu'), tmp_path)


def test_stream_refusals():
    with emu.active():
        run_stream_refusals(torch.device('cpu'))
