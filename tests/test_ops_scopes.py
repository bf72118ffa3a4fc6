"""The host-side ordering rules of ops.py's stream branches (ops._branches: cffm_branch_mark / _take / _join) and of the deferred branch
(ops._deferred: cffm_defer_begin / _join), and the buffer registry behind ops.cat_room.

The emulator runs every branch on the caller's stream, so a torch op enqueued between a mark and its join, an unjoined branch after a failed
stage call or a populated ops._DEFERRED after an aborted backward pass change no number there.  These tests therefore look at the CALL
SEQUENCE: a recording proxy around the emulator library (installed through _lib._override, as tests/emu.py does) logs the scope calls, a
TorchDispatchMode logs what torch dispatches in between, and the proxy can fail the n-th stage call of a region.  The emulator ignores
stream arguments, so the proxy may hand out a distinct handle from cffm_defer_begin to exercise the deferred bookkeeping."""
import contextlib
import gc
import weakref

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from tests import emu
from vss_cffm_amd import _lib, ops

SCOPE_CALLS = ('cffm_branch_mark', 'cffm_branch_take', 'cffm_branch_join', 'cffm_defer_begin', 'cffm_defer_join')
DEFER_HANDLE = 0xD0      # never dereferenced: the emulator ignores streams


class Recorder:
    """Forwards everything to the emulator library; logs the scope calls into `events`; `arm(opener, n)`: the n-th stage call (a call
    that returns a status) after the next `opener` returns non-zero instead of running."""

    def __init__(self, lib, events, defer_handle=None):
        self._lib, self.events, self._defer_handle = lib, events, defer_handle
        self._opener, self._n, self._countdown, self._failed = None, 0, 0, False

    def arm(self, opener, n):
        self._opener, self._n, self._countdown = opener, n, 0

    def names(self):
        return [e[1] for e in self.events if e[0] == 'lib']

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('cffm_'):
            return fn

        def call(*args):
            if name in SCOPE_CALLS:
                self.events.append(('lib', name))
                if name == self._opener:
                    self._opener, self._countdown = None, self._n
                res = fn(*args)
                return self._defer_handle if (name == 'cffm_defer_begin' and self._defer_handle) else res
            if name == 'cffm_last_error' and self._failed:
                self._failed = False
                return b'injected failure'
            if self._countdown and fn.restype is _lib.ci:
                self._countdown -= 1
                if self._countdown == 0:
                    self._failed = True
                    self.events.append(('lib', 'FAIL ' + name))
                    return 1
            return fn(*args)
        return call


@contextlib.contextmanager
def recording(defer_handle=None):
    events = []
    prev = _lib._override
    rec = Recorder(emu.lib(), events, defer_handle)
    _lib._override = rec
    try:
        yield rec
    finally:
        _lib._override = prev
        del ops._DEFERRED[:]


class AtenLog(TorchDispatchMode):
    def __init__(self, events):
        super().__init__()
        self.events = events

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.events.append(('aten', func))
        return func(*args, **(kwargs or {}))


def aten_inside_scopes(events):
    """the aten ops dispatched between a cffm_branch_mark and its cffm_branch_join that are no pure views"""
    bad, inside, scopes = [], False, 0
    for kind, what in events:
        if kind == 'lib' and what == 'cffm_branch_mark':
            assert not inside
            inside, scopes = True, scopes + 1
        elif kind == 'lib' and what == 'cffm_branch_join':
            assert inside
            inside = False
        elif kind == 'aten' and inside and not what.is_view:
            bad.append(str(what))
    assert not inside
    return scopes, bad


# ------------------------------------------------------------------------------------------------ the operators under test
def fuse_inputs(device='cpu', layout='channels_last'):
    """segformer_fuse at N=2, feature channels (8, 12, 16, 20), maps 16x24, 8x12, 4x6, 2x3"""
    gen = torch.Generator().manual_seed(11)
    n, chans, sizes = 2, (8, 12, 16, 20), ((16, 24), (8, 12), (4, 6), (2, 3))
    feats = []
    for c, (h, w) in zip(chans, sizes):
        f = torch.randn(n, c, h, w, generator=gen).to(device)
        if layout == 'channels_last':
            f = f.contiguous(memory_format=torch.channels_last)
        elif layout == 'permuted':
            f = f.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)           # a permuted view of an NHWC tensor
        else:
            f = f.contiguous()
        feats.append(f.requires_grad_(True))
    lin_w = [(torch.randn(256, c, generator=gen) * 0.1).to(device).requires_grad_(True) for c in chans]
    lin_b = [torch.randn(256, generator=gen).to(device).requires_grad_(True) for _ in chans]
    fuse_w = (torch.randn(256, 4 * 256, 1, 1, generator=gen) * 0.05).to(device).requires_grad_(True)
    gy = torch.randn(n, 256, *sizes[0], generator=gen).to(device)
    return feats, lin_w, lin_b, fuse_w, gy


def run_fuse(inp, between=None):
    """-> [output, 4 feature gradients, 9 parameter gradients]"""
    feats, lin_w, lin_b, fuse_w, gy = inp
    leaves = list(feats) + list(lin_w) + list(lin_b) + [fuse_w]
    for v in leaves:
        v.grad = None
    y = ops.segformer_fuse(feats, lin_w, lin_b, fuse_w)
    if between is not None:
        between()
    (y * gy).sum().backward()
    return [y.detach().clone()] + [v.grad.clone() for v in leaves]


def conv_inputs(device='cpu'):
    """conv1x1 of x [6,16,5,6] (plain NCHW) with weight [12,16,1,1]"""
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(6, 16, 5, 6, generator=gen).to(device).requires_grad_(True)
    wt = torch.randn(12, 16, 1, 1, generator=gen).to(device).requires_grad_(True)
    bs = torch.randn(12, generator=gen).to(device).requires_grad_(True)
    gy = torch.randn(6, 12, 5, 6, generator=gen).to(device)
    return x, wt, bs, gy


def run_conv(inp, clips, between=None):
    x, wt, bs, gy = inp
    for v in (x, wt, bs):
        v.grad = None
    y = ops.conv1x1(x, wt, bs, clips=clips)
    if between is not None:
        between()
    (y * gy.view(y.shape)).sum().backward()
    return [y.detach().clone(), x.grad.clone(), wt.grad.clone(), bs.grad.clone()]


def cat_inputs():
    """frame_logits_cat at B=2 clips of T=3 frames: fused [6,16,5,6] channels-last (as the rows path hands it), 12 classes"""
    gen = torch.Generator().manual_seed(13)
    b, t, c, o, h, w = 2, 3, 16, 12, 5, 6
    xc = torch.randn(b * t, h, w, c, generator=gen).permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.randn(o, c, 1, 1, generator=gen).requires_grad_(True)
    bs = torch.randn(o, generator=gen).requires_grad_(True)
    x2 = torch.randn(b, 1, h, w, o, generator=gen).permute(0, 1, 4, 2, 3).requires_grad_(True)
    gy = torch.randn(b, t + 1, o, h, w, generator=gen)
    return xc, wt, bs, x2, gy, b


def run_cat(inp, through=None, late=True):
    """late=False: the parameters not through ops.late_params (no race in the emulator) -- then nothing but the end-of-pass callback joins"""
    xc, wt, bs, x2, gy, b = inp
    for v in (xc, wt, bs, x2):
        v.grad = None
    lw, lb = ops.late_params(wt, bs) if late else (wt, bs)
    z = ops.frame_logits_cat(xc if through is None else through(xc), lw, lb, x2, b)
    (z * gy).sum().backward()
    return [z.detach().clone()] + [v.grad.clone() for v in (xc, wt, bs, x2)]


def all_equal(got, ref):
    return len(got) == len(ref) and all(torch.equal(a, b) for a, b in zip(got, ref))


# ------------------------------------------------------------------------------------------------ nothing but library calls in a scope
def test_no_torch_op_inside_a_branch_scope():
    """Between cffm_branch_mark and cffm_branch_join torch dispatches pure views at the most: a copy or a fill would be enqueued on the
    caller's stream BEHIND the mark (a branch waits for the mark only), an allocation could hand a branch's block to somebody else.
    Channels-last features make segformer_fuse copy them, a plain-NCHW input makes conv1x1's backward transpose its input gradient."""
    with recording() as rec:
        with AtenLog(rec.events):
            run_fuse(fuse_inputs())
        assert aten_inside_scopes(rec.events) == (2, [])                  # _SegFuseFn.forward, .backward
        for clips in (0, 2):
            del rec.events[:]
            with AtenLog(rec.events):
                run_conv(conv_inputs(), clips)
            assert aten_inside_scopes(rec.events) == (1, [])              # _Conv1x1Fn.backward
            assert sum(k == 'aten' for k, _ in rec.events) > 0


# ------------------------------------------------------------------------------------------------ a failing stage call
@pytest.mark.parametrize('region', ['fuse_forward', 'fuse_backward', 'conv_backward'])
@pytest.mark.parametrize('nth', [1, 3])
def test_branch_scope_joins_when_a_stage_call_fails(region, nth):
    with recording() as rec:
        if region == 'conv_backward':
            inp = conv_inputs()
            run = lambda between=None: run_conv(inp, 2, between)
        else:
            inp = fuse_inputs()
            run = lambda between=None: run_fuse(inp, between)
        ref = run()
        del rec.events[:]
        arm = lambda: rec.arm('cffm_branch_mark', nth)
        with pytest.raises(_lib.CffmError, match='injected failure'):
            if region == 'fuse_forward':
                arm()
                run()
            else:
                run(between=arm)
        names = rec.names()
        fail = [i for i, s in enumerate(names) if s.startswith('FAIL')]
        assert len(fail) == 1
        mark = max(i for i, s in enumerate(names[:fail[0]]) if s == 'cffm_branch_mark')
        assert 'cffm_branch_join' not in names[mark:fail[0]]              # the failure was inside the scope ...
        assert names[fail[0] + 1:].count('cffm_branch_join') == 1         # ... and the scope closed behind it, once
        assert not ops._DEFERRED
        assert all_equal(run(), ref)


@pytest.mark.parametrize('nth', [1, 4])
def test_deferred_scope_joins_when_a_stage_call_fails(nth):
    with recording(defer_handle=DEFER_HANDLE) as rec:
        inp = cat_inputs()
        ref = run_cat(inp)
        assert rec.names().count('cffm_defer_begin') == 1 and not ops._DEFERRED
        del rec.events[:]
        rec.arm('cffm_defer_begin', nth)
        with pytest.raises(_lib.CffmError, match='injected failure'):
            run_cat(inp)
        names = rec.names()
        fail = [i for i, s in enumerate(names) if s.startswith('FAIL')]
        assert len(fail) == 1 and names.index('cffm_defer_begin') < fail[0]
        assert names[fail[0] + 1:].count('cffm_defer_join') == 1
        assert not ops._DEFERRED
        assert all_equal(run_cat(inp), ref) and not ops._DEFERRED


# ------------------------------------------------------------------------------------------------ an aborted backward pass
class _Boom(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError('boom')


def test_aborted_pass_does_not_poison_the_next():
    """A backward pass that dies after frame_logits_cat deferred never runs its end-of-pass callback.  The next pass must still queue
    one: its gradients are right and it leaves ops._DEFERRED empty."""
    with recording(defer_handle=DEFER_HANDLE) as rec:
        inp = cat_inputs()
        ref = run_cat(inp)
        with pytest.raises(RuntimeError, match='boom'):
            run_cat(inp, through=_Boom.apply)
        assert ops._DEFERRED                                              # the aborted pass had deferred
        del rec.events[:]
        assert all_equal(run_cat(inp, late=False), ref)
        assert not ops._DEFERRED
        assert rec.names()[-1] == 'cffm_defer_join'                       # the end-of-pass callback: nothing else joins here
    with emu.active():                                                     # the plain emulator (no deferred stream): same numbers
        assert all_equal(run_cat(inp), ref)


# ------------------------------------------------------------------------------------------------ cat_room
def test_cat_room_goes_by_the_buffer():
    with emu.active():
        # a [:, :T] slice of an ordinary rows buffer has the strides of a front view and LIVE data at [:, T]
        lookalike = torch.empty(2, 4, 5, 6, 12)[:, :3].permute(0, 1, 4, 2, 3)
        assert not ops.cat_room(lookalike, 1)
        x, wt, bs, _ = conv_inputs()
        x2 = torch.randn(2, 1, 5, 6, 12).permute(0, 1, 4, 2, 3)
        y = ops.conv1x1(x, wt, bs, clips=2, extra=1)
        assert ops.cat_room(y, 1) and not ops.cat_room(y, 2) and not ops.cat_room(y, 0)
        assert ops.cat_room(y.detach(), 1)                                # an alias of the front view (the CFFM++ head detaches it): same room
        assert not ops.cat_room(y * 1, 1) and not ops.cat_room(y[:, :2], 1) and not ops.cat_room(y[:, 1:], 1)
        assert not ops.cat_room(ops.conv1x1(x, wt, bs, clips=2), 1)
        with pytest.raises(_lib.CffmError):
            ops.cat_into(lookalike, x2)                                   # not silently as_strided over whatever lies behind
        z = ops.cat_into(y.detach(), x2)
        assert z.shape == (2, 4, 12, 5, 6) and z.data_ptr() == y.data_ptr() and torch.equal(z[:, 3:], x2)
        assert not ops.cat_room(y, 1) and not ops.cat_room(y.detach(), 1)  # consumed, for every alias
        with pytest.raises(_lib.CffmError):
            ops.cat_into(y, x2)
        # the entry neither keeps the buffer alive nor outlives it
        del y, z
        gc.collect()
        assert len(ops._ROOMS) == 0
        y = ops.conv1x1(x, wt, bs, clips=2, extra=1)
        assert ops.cat_room(y, 1) and len(ops._ROOMS) == 1
        refs = [weakref.ref(y), weakref.ref(y.untyped_storage())]
        del y
        gc.collect()
        assert all(r() is None for r in refs) and len(ops._ROOMS) == 0


def test_cffmpp_head_concatenates_in_place(monkeypatch):
    """The CFFM++ head's rows path in training mode appends the prototype map behind the frame logits where they lie (ops.cat_into), although
    it DETACHES the frame logits between the classifier and the concatenation (cffm_head.py:514-518).  (The base head's training path is
    ops.frame_logits_cat.)"""
    import os, tempfile
    from oracle import recipe as R, ref_import as RI
    from tests.golden.make_golden_head import feature_maps
    from vss_cffm_amd import head as Hd
    from vss_cffm_amd.registry import build_head
    chans, made, cats = (32, 64, 160, 256), [], []
    monkeypatch.setattr(Hd, 'conv1x1', lambda *a: made.append(ops.conv1x1(*a)) or made[-1])
    monkeypatch.setattr(Hd, 'cat_into', lambda x, x2: cats.append((x.data_ptr(), ops.cat_into(x, x2))) or cats[-1][1])
    with emu.active(), tempfile.TemporaryDirectory() as tmp:
        feats = feature_maps(2, 4, 32, chans=chans, seed=72)
        metas = []
        for v in range(2):
            os.makedirs(os.path.join(tmp, 'vid%d' % v))
            torch.save(R.synth_input('centers%d' % v, (1, 8, 256), seed=74 + v, scale=1.0), os.path.join(tmp, 'vid%d' % v, 'centers.pt'))
            metas.append({'filename': tmp + '/data/vid%d/origin/0001.jpg' % v})
        head = build_head(RI.head_cfg(kind='CFFMHead_clips_resize1_8_finetune_w_prototype3', in_channels=chans, depths=1))
        head.load_state_dict(R.synth_state(head, seed=71), strict=False)
        Hd.revert_sync_batchnorm(head)
        head.save_path = tmp + '/'
        out = head.train()(feats, 2, 4, None, metas)
        frame = [y for y in made if y.dim() == 5]                         # the frame logits [B,T,K,h,w]: the classifier called with clips
        assert len(frame) == 1 and len(cats) == 1
        assert out.shape[1] == 5 and out.data_ptr() == frame[0].data_ptr() == cats[0][0]


# ------------------------------------------------------------------------------------------------ GPU: strided features
@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['channels_last', 'permuted'])
def test_segformer_fuse_strided_features_gpu(layout):
    """Features that segformer_fuse has to copy first give BIT-identical results (output, four feature and nine parameter gradients) to
    plain-NCHW copies of the same values: nothing here uses atomics (tests/test_headfuse.py::test_head_step_replayed_equals_eager_gpu
    rests on the same fact).  This pins the semantics for strided inputs; it is no race detector -- at this size the copy usually wins
    against the branches anyway.  The structural guarantee is test_no_torch_op_inside_a_branch_scope."""
    dev = torch.device('cuda')
    ref = run_fuse(fuse_inputs(dev, 'plain'))
    inp = fuse_inputs(dev, layout)
    assert not any(f.is_contiguous() for f in inp[0])
    got = run_fuse(inp)
    torch.cuda.synchronize()
    assert len(got) == 1 + 4 + 9
    for a, b in zip(got, ref):
        assert a.shape == b.shape and torch.equal(a, b)
