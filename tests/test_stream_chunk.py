"""Segmenting a video in chunks (vss_cffm_amd.ClipStream.push_many; include/cffm_hip.h: cffm_segfuse_pool_fwd_frames,
cffm_layer_infer_rows_ring_tables) on the CPU through the fiber emulator.  The GPU half is tests/test_stream_chunk_gpu.py and shares the
run_*(device) bodies below.

A. cffm_segfuse_pool_fwd_frames through the raw ABI: every named slot bit-equal to cffm_segfuse_pool_fwd at N = 1 on that frame's slices.
B. cffm_layer_infer_rows_ring_tables: sample b bit-equal to cffm_layer_infer_rows_ring at B = 1 with that sample's table.
C. The heads and ClipStream on the toy segmentor with the sample-by-sample backbone of tests/test_stream.py, a 30-frame video, max_chunk = 4
   (R = 13: the ring wraps twice).

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
from tests import test_stream as T
from tests.test_kmeans import CallSpy
from vss_cffm_amd import _lib, data, ops

NAN, GUARD = T.NAN, T.GUARD
RING = 6           # slots of the rings of A and B


# ---------------------------------------------------------------------------------------------- A. cffm_segfuse_pool_fwd_frames
# the shapes of tests/test_stream.py with N >= 2, and three frames at 4 x 6; (slots, out-of-range table, where its entries land)
FRAME_SHAPES = {name: T.POOL_SHAPES[name] for name in T.POOL_SHAPES if T.POOL_SHAPES[name][0] >= 2}
FRAME_SHAPES['n3_4x6'] = (3, 4, 6, ((2, 3), (1, 2), (1, 1)))
SLOTS = {2: ([4, 0], [7, -1], [5, 0]), 3: ([4, 0, 2], [7, -1, 2], [5, 0, 2])}


class FramesCase:
    """seeded operands of one shape and the reference rows per frame (the existing cffm_segfuse_pool_fwd at N = 1 on the frame's slices of
    the same inputs), computed once"""

    def __init__(self, name, device):
        self.N, self.H, self.W, self.maps = FRAME_SHAPES[name]
        N, H, W = self.N, self.H, self.W
        g = torch.Generator().manual_seed(3000 + sorted(FRAME_SHAPES).index(name))
        rnd = lambda *s: torch.randn(*s, generator=g)
        self.y = rnd(N * H * W, 256).to(device)
        self.d = rnd(256).to(device)
        self.z = [rnd(N * h * w, 256).to(device) for h, w in self.maps]
        sign = torch.where(torch.rand(256, generator=g) < 1.0 / 3.0, -1.0, 1.0)       # the ReLU cuts on both sides of the sums
        self.scale = ((0.5 + torch.rand(256, generator=g)) * sign).to(device)
        self.shift = (0.5 * rnd(256)).to(device)
        self.device = device
        k = len(self.maps)
        self.hs = (C.c_int * 3)(*([h for h, _ in self.maps] + [1] * (3 - k)))
        self.ws = (C.c_int * 3)(*([w for _, w in self.maps] + [1] * (3 - k)))
        self.zp = self.map_ptrs(self.z)
        self.rows = (H // 2) * (W // 2)                                              # of ONE frame
        lib, st = _lib.get(), ops._stream(self.y)
        self.want = []
        for n in range(N):
            zn = [z[n * h * w:(n + 1) * h * w] for z, (h, w) in zip(self.z, self.maps)]
            out = torch.full((self.rows, 256), NAN, device=device)
            _lib.check(lib.cffm_segfuse_pool_fwd(ops._ptr(self.y[n * H * W:(n + 1) * H * W]), ops._ptr(self.d), self.map_ptrs(zn), self.hs, self.ws,
                                                 k, ops._ptr(self.scale), ops._ptr(self.shift), ops._ptr(out), self.rows * 256, 1, None, 0, 1, H, W,
                                                 st), lib)
            T.sync(device)
            assert not torch.isnan(out).any()
            self.want.append(out)
        allw = torch.cat(self.want)
        assert bool((allw == 0).any()) and bool((allw > 0).any()), 'the ReLU cuts somewhere and passes somewhere'
        self.kept = [self.y.clone(), self.d.clone()] + [z.clone() for z in self.z]

    def map_ptrs(self, zs):
        return (C.c_void_p * 3)(*([z.data_ptr() for z in zs] + [None] * (3 - len(zs))))

    def call(self, ring, slot_floats, nslots, slots, y=None, H=None, W=None):
        lib = _lib.get()
        y = self.y if y is None else y
        return lib.cffm_segfuse_pool_fwd_frames(ops._ptr(y), ops._ptr(self.d), self.zp, self.hs, self.ws, len(self.maps), ops._ptr(self.scale),
                                                ops._ptr(self.shift), ops._ptr(ring) if ring is not None else None, slot_floats, nslots,
                                                ops._ptr(slots) if slots is not None else None, self.N, H or self.H, W or self.W,
                                                ops._stream(self.y))

    def inputs_unchanged(self):
        return all(T.same_bits(a, b) for a, b in zip([self.y, self.d] + self.z, self.kept))


def run_segfuse_frames(name, device):
    c = FramesCase(name, device)
    sf = c.rows * 256
    slot = lambda ring, s: ring[s * c.rows:(s + 1) * c.rows]
    named, wild, lands = SLOTS[c.N]
    # a permutation with gaps, then entries outside the ring: clamped on the device to the last / first slot (documented, no fault)
    for entries, where in ((named, named), (wild, lands)):
        ring = torch.full((RING * c.rows + GUARD, 256), NAN, device=device)
        assert c.call(ring, sf, RING, T.table(entries, device)) == 0, _lib.get().cffm_last_error()
        T.sync(device)
        for n, s in enumerate(where):
            assert T.same_bits(slot(ring, s), c.want[n]), (name, entries, n)
        assert all(T.all_nan(slot(ring, s)) for s in range(RING) if s not in where) and T.all_nan(ring[RING * c.rows:])
        assert c.inputs_unchanged(), 'y, d and the maps are only read'
    # a slot longer than a frame: the rows lie at the head of each slot
    ring = torch.full((RING * (c.rows + 1) + GUARD, 256), NAN, device=device)
    assert c.call(ring, sf + 256, RING, T.table(named, device)) == 0
    T.sync(device)
    for n, s in enumerate(named):
        assert T.same_bits(ring[s * (c.rows + 1):s * (c.rows + 1) + c.rows], c.want[n])
    assert int(torch.isnan(ring).all(dim=1).sum()) == ring.shape[0] - c.N * c.rows


def run_segfuse_frames_refusals(device):
    """an error each, before anything is enqueued -- the poisoned ring stays untouched"""
    c = FramesCase('n2_4x6', device)
    lib = _lib.get()
    sf = c.rows * 256
    ring = torch.full((RING * c.rows + GUARD, 256), NAN, device=device)
    slots = T.table([4, 0], device)
    big_y = torch.randn(2 * 5 * 7, 256).to(device)                     # room for the odd sizes
    kept = big_y.clone()
    assert c.call(ring, sf, RING, slots, y=big_y, H=5, W=6) != 0 and b'even' in lib.cffm_last_error()
    assert c.call(ring, sf, RING, slots, y=big_y, H=4, W=7) != 0 and b'even' in lib.cffm_last_error()
    assert c.call(None, sf, RING, slots) != 0 and b'null' in lib.cffm_last_error()
    assert c.call(ring, sf, RING, None) != 0 and b'null' in lib.cffm_last_error()
    y_poison = torch.full((c.N * c.H * c.W, 256), NAN, device=device)
    assert c.call(y_poison, sf, 1, slots, y=y_poison) != 0 and b'overlaps' in lib.cffm_last_error()
    assert c.call(c.z[0], sf, 1, slots) != 0 and b'overlaps' in lib.cffm_last_error()
    assert c.call(ring.view(-1)[1:], sf, RING, slots) != 0 and b'aligned' in lib.cffm_last_error()
    assert c.call(ring, sf - 4, RING, slots) != 0 and b'slots of' in lib.cffm_last_error()          # below one frame
    T.sync(device)
    assert T.all_nan(ring) and T.all_nan(y_poison) and T.same_bits(big_y, kept) and c.inputs_unchanged()
    # the Python operator validates what the host can see
    head = T.streaming_segmentor(device).decode_head
    feats = [torch.randn(2, ch, 16 // s, 16 // s).to(device) for ch, s in zip(TS.B0, (1, 2, 4, 8))]
    lins = (head.linear_c1, head.linear_c2, head.linear_c3, head.linear_c4)
    args = lambda: (feats, [l.proj.weight for l in lins], [l.proj.bias for l in lins], head.linear_fuse.conv.weight, head.linear_fuse.bn)
    good = torch.full((RING, 64, 256), NAN, device=device)
    with torch.no_grad():
        for bad_ring, bad_slots in ((good[:, :63], slots), (good.double(), slots), (good, slots.long()), (good, T.table([4, 0, 2], device)),
                                    (good, slots.view(1, 2)), (good.unsqueeze(1), slots), (good.transpose(0, 1), slots)):
            with pytest.raises(_lib.CffmError):
                ops.segformer_fuse_pool_frames(*args(), bad_ring, bad_slots)
    with pytest.raises(_lib.CffmError, match='inference only'):
        ops.segformer_fuse_pool_frames(*args(), good, slots)            # the parameters require grad and grad mode is on
    head.linear_fuse.bn.train()
    with pytest.raises(_lib.CffmError, match='eval'), torch.no_grad():
        ops.segformer_fuse_pool_frames(*args(), good, slots)
    assert T.all_nan(good)


# ---------------------------------------------------------------------------------------------- B. cffm_layer_infer_rows_ring_tables
LAYER_SHAPES = {'b1_8x8_d1': (1, 8, 8, 1), 'b3_8x8_d2': (3, 8, 8, 2), 'b2_14x21_d2': (2, 14, 21, 2)}
TABLES = [[4, 0, 2, 1], [1, 1, 3, 2], [0, 2, 4, 5]]     # a clip each; the second repeats a slot; slots 1, 2, 4 ... are shared between samples


@functools.lru_cache(maxsize=None)
def layer_case(name):
    b, h, w, depth = LAYER_SHAPES[name]
    seed = 400 + sorted(LAYER_SHAPES).index(name)
    return R.layer_state(depth, seed=seed), R.synth_input('ring', (RING, h * w, 256), seed=seed + 50)


def tables_for(b):
    """B = 1 gets each of the first two clips in turn, B > 1 the first B together"""
    return [TABLES[:1], TABLES[1:2]] if b == 1 else [TABLES[:b]]


def run_layer_tables(name, device):
    lib = _lib.get()
    b, h, w, depth = LAYER_SHAPES[name]
    st, ring0 = layer_case(name)
    params = TI.flat_params(st, depth, device)
    prepared = ops.layer_prepare(depth, params)
    need = lib.cffm_layer_infer_ws_floats(C.byref(ops.make_geom(lib, b, h, w)))
    for entries in tables_for(b):
        ring = ring0.clone().to(device)
        for s in set(range(RING)) - set(sum(entries, [])):
            ring[s] = NAN                                             # a slot no table names is never read
        kept = ring.clone()
        tables = T.table(entries, device)
        # the yardstick: the EXISTING entry at B = 1 with each sample's four entries
        want = torch.cat([ops.cffm_layer_rows_ring(ring.unsqueeze(1), T.table(e, device), h, w, depth, params, prepared) for e in entries])
        assert not torch.isnan(want).any() and want.shape == (b, h * w, 256)
        buf, out = T.poisoned_out(b, h * w, device)
        ws = torch.full((need + GUARD,), NAN, device=device)
        got = ops.cffm_layer_rows_ring_tables(ring, tables, h, w, depth, params, prepared, ws=ws, out=out)
        T.sync(device)
        assert got.data_ptr() == out.data_ptr() and T.same_bits(got, want), (name, entries)
        assert T.all_nan(buf[b * h * w:]) and T.all_nan(ws[need:]) and T.same_bits(ring, kept), 'guards intact, the ring only read'
        if b > 1:
            assert not T.same_bits(got[0], got[1]), 'every sample has a clip of its own'


def run_layer_tables_refusals(device):
    lib = _lib.get()
    name = 'b3_8x8_d2'
    b, h, w, depth = LAYER_SHAPES[name]
    st, ring0 = layer_case(name)
    params = TI.flat_params(st, depth, device)
    prepared = ops.layer_prepare(depth, params)
    ring = ring0.clone().to(device)
    kept = ring.clone()
    tables = T.table(TABLES, device)
    g, (key_src, q_dst, *_) = ops._layer_geom(lib, b, h, w, device)
    need = lib.cffm_layer_infer_ws_floats(C.byref(g))
    ws = torch.full((need,), NAN, device=device)
    buf, out = T.poisoned_out(b, h * w, device)
    img = h * w * 256
    raw = lambda tab, y, ws_: lib.cffm_layer_infer_rows_ring_tables(C.byref(g), depth, ops.block_structs(params, depth), ops._ptr(prepared),
                                                                   ops._ptr(ring), img, RING, tab, ops._ptr(y), ops._ptr(key_src),
                                                                   ops._ptr(q_dst), ops._ptr(ws_), ops._stream(ring))
    assert raw(None, out, ws) != 0 and b'null or misaligned' in lib.cffm_last_error()
    assert raw(C.c_void_p(tables.data_ptr() + 2), out, ws) != 0 and b'null or misaligned' in lib.cffm_last_error()
    assert raw(ops._ptr(tables), ring[3:], ws) != 0 and b'inside the ring' in lib.cffm_last_error()
    assert raw(ops._ptr(tables), out, ring.view(-1)[img:]) != 0 and b'workspace lies inside the ring' in lib.cffm_last_error()
    with pytest.raises(_lib.CffmError, match='inside the ring'):
        ops.cffm_layer_rows_ring_tables(ring, tables, h, w, depth, params, prepared, out=ring[3:])
    for bad_ring, bad_tables in ((ring[:, :63], tables), (ring, tables.long()), (ring, tables[:, :3].contiguous()), (ring, tables.view(-1)),
                                 (ring, tables.t().contiguous().t()), (ring.double(), tables), (ring.unsqueeze(1), tables)):
        with pytest.raises(_lib.CffmError):
            ops.cffm_layer_rows_ring_tables(bad_ring, bad_tables, h, w, depth, params, prepared)
    T.sync(device)
    assert T.same_bits(ring, kept) and T.all_nan(buf) and T.all_nan(ws)


# ---------------------------------------------------------------------------------------------- C. heads and ClipStream
FRAMES, MAX_CHUNK, SEED = 30, 4, 77
SHORT = 3          # frames 0..2: clips shorter than num_clips, the head's short-circuit through push


@functools.lru_cache(maxsize=None)
def per_frame(device, frames=FRAMES, pp_dir=None):
    """the seeded video pushed frame by frame on a stream of its own (the parent's path), once per device: segmentor, frames, metas,
    per-frame logits and label maps -- the yardstick of C.3, left unchanged"""
    if pp_dir is None:
        seg = T.streaming_segmentor(device)
    else:
        seg = T.streaming_segmentor(device, decode_head=RI.head_cfg(kind='CFFMHead_clips_resize1_8_finetune_w_prototype3'))
        seg.decode_head.save_path = pp_dir + '/'
    video = [f.to(device) for f in T.make_video(1, frames, SEED)]
    mt = T.metas(1)
    stream = V.ClipStream(seg)
    assert stream.slots_in_ring == 10 and stream.max_chunk == 1
    logits, maps = [], []
    with torch.no_grad():
        for i, f in enumerate(video):
            maps.append(stream.push(f, mt, to_numpy=False).cpu())
            lg = stream.last_logits.contiguous().cpu()
            # the condition on the seeded video: the per-frame path alone stays inside the exempt cap at every frame
            values, probs = TP.op_sequence(lg, (64, 64), TS.ORI)
            TP.check_argmax(maps[-1], values, probs.argmax(dim=1), float(lg.abs().max()), 'per-frame push against its own logits, frame %d' % i)
            logits.append(lg)
    return seg, video, mt, logits, maps


def sub_chunks(count, c, max_chunk):
    """how push_many cuts c frames that follow `count` pushed ones: [(first, m, through_push)]"""
    out, j = [], count
    while j < count + c:
        if j < SHORT:
            out.append((j, 1, True))
            j += 1
        else:
            m = min(max_chunk, count + c - j)
            out.append((j, m, False))
            j += m
    return out


def composed_chunk(seg, video, rows, first, m, mt, slots_in_ring):
    """frames first .. first + m - 1 as the EXISTING ops compose them at batch size m: segformer_fuse + bn_relu_pool on the m frames, the
    stacks gathered per table with index_select, forward_rows at B = m, _rows_logits (and the CFFM++ additions).  `rows`: frame -> its
    [1, h2*w2, 256] stack rows, as tests/test_stream.py keeps them."""
    head = seg.decode_head
    lins = (head.linear_c1, head.linear_c2, head.linear_c3, head.linear_c4)
    dev = video[0].device
    feats = seg.extract_feat(torch.cat(video[first:first + m]))
    y = ops.segformer_fuse(list(head._transform_inputs(feats)), [l.proj.weight for l in lins], [l.proj.bias for l in lins],
                           head.linear_fuse.conv.weight)
    stack = ops.bn_relu_pool(y, head.linear_fuse.bn, want_stack=True)[1].view(m, 64, 256)
    for n in range(m):
        rows[first + n] = stack[n:n + 1]
    r, (h, w) = slots_in_ring, (16, 16)
    ring = torch.full((r, 64, 256), NAN, device=dev)
    for f in range(max(0, first + m - r), first + m):
        ring[f % r] = rows[f][0]
    tables = T.table([[f % r for f in data.clip_indices_test(first + n, first + n + 1)] for n in range(m)], dev)
    x_rows = ring.index_select(0, tables.view(-1).long()).view(m, 4, 64, 256)
    assert not torch.isnan(x_rows).any()
    mined = head.decoder_focal.forward_rows(x_rows, h // 2, w // 2)
    x2 = head._rows_logits(head.linear_pred2, torch.cat([x_rows[:, -1], mined], dim=-1).view(m, h // 2, w // 2, -1), head.dropout, (h, w))
    if not hasattr(head, 'decoder_swin'):
        return x2.squeeze(1)
    centers = head._load_centers(mt, dev).expand(m, -1, -1).contiguous()
    ctx = head.decoder_swin(x_rows[:, -1].contiguous(), h // 2, w // 2, centers)[0]
    x3 = head._rows_logits(head.linear_pred3, ctx.reshape(m, h // 2, w // 2, -1), head.dropout3, (h, w))
    return x2.squeeze(1) + 0.5 * x3.squeeze(1)


SPIED = ('cffm_predict', 'cffm_bn_relu_pool_fwd', 'cffm_segfuse_pool_fwd', 'cffm_segfuse_pool_fwd_frames', 'cffm_layer_infer_rows_ring',
         'cffm_layer_infer_rows_ring_tables')


def run_chunked(device, calls, base=None, max_chunk=MAX_CHUNK, stream=None):
    """`calls`: [('many', c) | ('push', 1)] covering the video.  C.1 - C.3 for every call; returns the stream and the label maps."""
    lib = _lib.get()
    seg, video, mt, frame_logits, frame_maps = base or per_frame(device)
    assert sum(c for _, c in calls) == len(video)
    stream = stream or V.ClipStream(seg, max_chunk=max_chunk)
    assert stream.slots_in_ring == 9 + max_chunk and stream.stream_impl == 'hip' and stream.count == 0
    rows, maps, j = {}, [], 0
    with torch.no_grad():
        for kind, c in calls:
            parts = sub_chunks(j, c, max_chunk) if kind == 'many' else [(j, 1, True)]
            T.SampledToyBackbone.calls = 0
            with CallSpy(lib, *SPIED) as spy:
                if kind == 'many':
                    pred = stream.push_many(torch.cat(video[j:j + c]), mt, to_numpy=False)
                else:
                    pred = stream.push(video[j], mt, to_numpy=False)
            singles, chunks = sum(1 for p in parts if p[2]), sum(1 for p in parts if not p[2])
            # 1. per chunk exactly one backbone call, one call of each of the two new entries and one predict; nothing of the clip path
            assert T.SampledToyBackbone.calls == singles + chunks and spy.n['cffm_predict'] == singles + chunks, (j, c, spy.n)
            assert spy.n['cffm_segfuse_pool_fwd_frames'] == chunks and spy.n['cffm_layer_infer_rows_ring_tables'] == chunks, (j, c, spy.n)
            assert spy.n['cffm_segfuse_pool_fwd'] == singles, (j, c, spy.n)
            assert spy.n['cffm_layer_infer_rows_ring'] == sum(1 for p in parts if p[2] and p[0] >= SHORT), (j, c, spy.n)
            if all(p[0] >= SHORT for p in parts):
                assert spy.n['cffm_bn_relu_pool_fwd'] == 0, (j, c, spy.n)
            logits = stream.last_logits
            assert pred.dtype == torch.int64 and pred.shape == (c,) + TS.ORI and logits.shape == (c, 124, 16, 16) and stream.count == j + c
            # 2. the logits bit-equal to the composition of the existing ops at the same batch size, the maps = ops.predict of that
            for first, m, single in parts:
                if single:
                    want = T.composed_logits(seg, video, rows, first, mt)
                else:
                    want = composed_chunk(seg, video, rows, first, m, mt, stream.slots_in_ring)
                assert T.same_bits(logits[first - j:first - j + m], want), 'frames %d..%d' % (first, first + m - 1)
                assert torch.equal(pred[first - j:first - j + m], ops.predict(want, (64, 64), TS.ORI, None)), 'frames %d..%d' % (first, first + m - 1)
            # 3. against frame-by-frame push on a stream of its own: the arg-max rule, measured on the per-frame logits
            for n in range(c):
                i = j + n
                print('frame %2d: logits bit-equal to the per-frame push: %s' % (i, T.same_bits(logits[n:n + 1], frame_logits[i])))
                values, probs = TP.op_sequence(frame_logits[i], (64, 64), TS.ORI)
                TP.check_argmax(pred[n:n + 1], values, probs.argmax(dim=1), float(frame_logits[i].abs().max()), 'push_many vs push, frame %d' % i)
            maps.extend(p.cpu() for p in pred.split(1))
            j += c
    return stream, maps


def run_whole_video_and_reset(device):
    """chunking [30]; 4. after reset() the same video gives the same maps (to_numpy: the reference's list of numpy maps)"""
    seg, video, mt, _, _ = per_frame(device)
    stream, maps = run_chunked(device, [('many', FRAMES)])
    with torch.no_grad():
        stream.reset()
        again = stream.push_many(torch.cat(video), mt)
    assert isinstance(again, list) and len(again) == FRAMES and again[0].shape == TS.ORI
    assert all(torch.equal(torch.from_numpy(a), m[0]) for a, m in zip(again, maps)), 'after reset() the same video gives the same maps'


def run_torch_partner(device):
    """stream_impl = 'torch': the same chunks with stock ops around the layer, none of the new entry points; the arg-max rule against it"""
    lib = _lib.get()
    seg, video, mt, _, frame_maps = per_frame(device)
    partner = V.ClipStream(seg, max_chunk=MAX_CHUNK)
    partner.stream_impl = 'torch'
    n = 12
    with torch.no_grad(), CallSpy(lib, *SPIED) as spy:
        pred = partner.push_many(torch.cat(video[:n]), mt, to_numpy=False)
    assert all(spy.n[k] == 0 for k in SPIED if k not in ('cffm_predict', 'cffm_bn_relu_pool_fwd')), spy.n
    lg = partner.last_logits.contiguous().cpu()
    for i in range(n):
        values, probs = TP.op_sequence(lg[i:i + 1], (64, 64), TS.ORI)
        TP.check_argmax(frame_maps[i], values, probs.argmax(dim=1), float(lg[i].abs().max()), "push 'hip' vs push_many 'torch', frame %d" % i)


def run_chunk_pp(device, tmp_path):
    """5. the CFFM++ head once: 8 frames as one push_many (three through push, five in one chunk), one centers.pt under tmp_path"""
    os.makedirs(os.path.join(str(tmp_path), 'vid0'))
    torch.save(R.synth_input('centers', (1, 8, 256), seed=35, scale=1.0), os.path.join(str(tmp_path), 'vid0', 'centers.pt'))
    base = per_frame(device, 8, str(tmp_path))
    run_chunked(device, [('many', 8)], base=base, max_chunk=8)


def run_chunk_refusals(device):
    seg, video, mt, _, _ = per_frame(device)
    chunk = torch.cat(video[:6])
    with pytest.raises(ValueError):
        V.ClipStream(seg, max_chunk=0)
    with torch.no_grad():
        two = V.ClipStream(seg, max_chunk=MAX_CHUNK)
        two.push(torch.cat(video[:2]), T.metas(2))                                  # two videos at once
        with pytest.raises(RuntimeError, match='ONE video'):
            two.push_many(chunk, mt)
        two.reset()
        assert len(two.push_many(chunk, mt)) == 6                                    # a new video may be one
        with pytest.raises(AssertionError, match='flip'):
            V.ClipStream(seg, max_chunk=MAX_CHUNK).push_many(chunk, [dict(mt[0], flip=True, flip_direction='horizontal')])
        walked = V.ClipStream(seg, max_chunk=MAX_CHUNK)
        walked.push_many(chunk, mt)
        with pytest.raises(RuntimeError, match='reset'):
            walked.push_many(chunk[:, :, :48, :48].contiguous(), mt)                 # another size in the middle of a video
        walked.reset()
        assert walked.push_many(chunk[:, :, :48, :48].contiguous(), mt)[5].shape == TS.ORI
    gene = T.streaming_segmentor(device, decode_head=RI.head_cfg(kind='CFFMHead_clips_resize1_8_gene_prototype'))
    with pytest.raises(NotImplementedError):
        V.ClipStream(gene, max_chunk=MAX_CHUNK)
    with pytest.raises(NotImplementedError):
        gene.decode_head.stream_rows_many(None, None, None)
    with pytest.raises(NotImplementedError):
        gene.decode_head.forward_stream_many(None, None, 16, 16)
    own = T.streaming_segmentor(device)                                              # (train() below must not reach the shared segmentor)
    own.train()
    with pytest.raises(RuntimeError, match='eval'):
        V.ClipStream(own, max_chunk=MAX_CHUNK).push_many(chunk, mt)
    with pytest.raises(RuntimeError, match='eval'):
        own.decode_head.stream_rows_many(None, None, None)
    with pytest.raises(RuntimeError, match='eval'):
        own.decode_head.forward_stream_many(None, T.table(TABLES, device), 16, 16)


# ---------------------------------------------------------------------------------------------- emulator
CPU = torch.device('cpu')


@pytest.mark.parametrize('name', sorted(FRAME_SHAPES))
def test_segfuse_frames_equals_the_single_frame_calls(name):
    with emu.active():
        run_segfuse_frames(name, CPU)


def test_segfuse_frames_refusals():
    with emu.active():
        run_segfuse_frames_refusals(CPU)


@pytest.mark.parametrize('name', sorted(LAYER_SHAPES))
def test_layer_tables_equals_the_ring_call_per_sample(name):
    with emu.active():
        run_layer_tables(name, CPU)


def test_layer_tables_refusals():
    with emu.active():
        run_layer_tables_refusals(CPU)


def test_whole_video_in_one_call_and_reset():
    with emu.active():
        run_whole_video_and_reset(CPU)


def test_uneven_chunks():
    with emu.active():
        run_chunked(CPU, [('many', c) for c in (1, 4, 6, 8, 11)])


def test_push_and_push_many_mixed():
    with emu.active():
        run_chunked(CPU, [('push', 1), ('many', 5), ('push', 1), ('many', FRAMES - 7)])


def test_chunk_torch_partner():
    with emu.active():
        run_torch_partner(CPU)


def test_chunk_cffmpp_head(tmp_path):
    with emu.active():
        run_chunk_pp(CPU, tmp_path)


def test_chunk_refusals():
    with emu.active():
        run_chunk_refusals(CPU)
