"""The NCHW forms of the fused Mlp kernels (csrc/panel_kernels.h): the layer's last block writes its output as the target
frame of the NCHW output (k_mlp_fwd<.., NCHW>) and reads the upstream gradient from the target frame of the NCHW gradient
(k_mlp_bwd<.., NCHW>), instead of going through token rows that only a transpose would write or read.  The arithmetic is that of the rows
forms, so everything is compared bit for bit, never with a tolerance:

  * forward stage: cffm_mlp_fwd_nchw against cffm_mlp_fwd followed by cffm_transpose on the same inputs -- the whole destination buffer
    (target frames, the three frames in front of each when the images are 4 frames apart, a guard region behind it: all sentinel-filled)
    and every other saved output;
  * backward stage: cffm_mlp_bwd_nchw against cffm_mlp_bwd on the rows of dy -- dh, dx1, dao, the dout rows the kernel emits, the five
    bias / norm gradients (the launch's record arrays, reduced in the same fixed order); NaN in every frame that is not a target frame,
    behind the gradient, and in the rows at and past NP of everything the kernel reads; sentinel rows behind every output;
  * layer: cffm_layer_forward_full + cffm_layer_backward_full against the sequence they replaced, expressed through the rows entry
    points and cffm_transpose (y, dx, every parameter gradient), depth 1 and 2; cffm_layer_infer_full against cffm_layer_infer_rows
    plus transposes.

What can go wrong is an index: rows at and past NP, a panel of 32 rows that holds the end of one image and the start of the next, four
pixels that are moved as one 16-byte unit although they cross an image or are not aligned (pixels per image not a multiple of 4).
Cases (images x pixels): 1 x 49 one ragged panel, odd pixel count; 2 x 56 a boundary inside panel 1, aligned quads; 3 x 50 boundaries at
50 and 100, quads that cross an image, ragged last panel; 2 x 112 whole panels with a boundary inside one (2 x 3600, the workload's own
shape, is 225 panels: far over a second on the emulator, where one panel costs about 0.1 s).  Each with the images one frame and four frames apart.

CPU: emulator build of the same sources; GPU: the product library."""
import ctypes as C
import functools

import pytest
import torch

from oracle import recipe as R
from tests import emu, helpers as H
from vss_cffm_amd import _lib, ops

SENTINEL = 7.0
GUARD = 4096                     # floats behind an NCHW buffer
PAD = 48                         # rows behind NP: more than a panel, so a panel that overruns NP lands in them
# (images, pixels per image)
CASES = [(1, 49), (2, 56), (3, 50), (2, 112)]
STRIDES = [1, 4]                 # images apart, in frames: the target frame alone, or frame 3 of a [B,4,256,HW] output


def P(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def stream_of(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == 'cuda' else None


def settle(device):
    if device.type == 'cuda':
        torch.cuda.synchronize(device)


def same(a, b):
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


@functools.lru_cache(maxsize=None)
def weights(device):
    """The block's Mlp parameters, the same for every case, on `device` with the fragment-ordered copies of both directions."""
    gen = torch.Generator().manual_seed(3000)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(device)
    t = dict(wp=rn(256, 256, scale=0.08), w1=rn(1024, 256, scale=0.08), w2=rn(256, 1024, scale=0.05), bp=rn(256, scale=0.1),
             b1=rn(1024, scale=0.1), b2=rn(256, scale=0.1), g2=1 + rn(256, scale=0.2), be2=rn(256, scale=0.1))
    lib, st = stage_lib(device), stream_of(device)
    for name in ('wp', 'w1', 'w2'):
        for form in (0, 1):
            t[name, form] = torch.empty(t[name].numel(), device=device)
            _lib.check(lib.cffm_panel_pack_weight(P(t[name]), t[name].shape[0], t[name].shape[1], form, P(t[name, form]), st), lib)
    settle(device)
    return t


def stage_lib(device):
    return _lib.get() if device.type == 'cuda' else emu.lib()


def fwd_outputs(device, NP):
    mk = lambda *s: torch.full(s, SENTINEL, device=device)
    return dict(x1=mk(NP, 256), z2s=mk(NP, 256), mean2=mk(NP), rstd2=mk(NP), hraw=mk(NP, 1024), acts=mk(NP, 1024))


def fwd_args(wt, t, pix, o):
    return [P(t['ao']), P(t['xt']), pix * 256, pix, P(wt['wp', 0]), P(wt['w1', 0]), P(wt['w2', 0]), P(wt['bp']), P(wt['b1']), P(wt['b2']),
            P(wt['g2']), P(wt['be2']), P(o['x1']), P(o['z2s']), P(o['mean2']), P(o['rstd2']), P(o['hraw']), P(o['acts'])]


def bwd_outputs(device, NP):
    mk = lambda *s: torch.full(s, SENTINEL, device=device)
    return dict(dhs=mk(NP + PAD, 1024), dx1=mk(NP + PAD, 256), dao=mk(NP + PAD, 256), dg2=mk(256), dbe2=mk(256), db1=mk(1024), db2=mk(256),
                dbp=mk(256))


def bwd_args(wt, sv, o, NP, st):
    return [P(sv['hraw']), P(wt['b1']), P(sv['x1']), P(sv['mean2']), P(sv['rstd2']), P(wt['g2']), P(wt['w2', 1]), P(wt['w1', 1]), P(wt['wp', 1]),
            P(o['dhs']), P(o['dx1']), P(o['dao']), P(o['dg2']), P(o['dbe2']), P(o['db1']), P(o['db2']), P(o['dbp']), NP, st]


@functools.lru_cache(maxsize=None)
def reference(device, nimg, pix):
    """One case on `device`: its inputs and what the ROWS forms give for them -- cffm_mlp_fwd (x2 as rows), cffm_mlp_bwd on the rows of
    dy.  Made once per case, shared by both strides and both directions, never modified."""
    lib, wt, st = stage_lib(device), weights(device), stream_of(device)
    NP = nimg * pix
    gen = torch.Generator().manual_seed(3000 + NP)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(device)
    t = dict(ao=rn(NP, 256), xt=rn(NP, 256, scale=1.5), dy=rn(nimg, 256, pix))
    fo = fwd_outputs(device, NP)
    x2 = torch.full((NP, 256), SENTINEL, device=device)
    _lib.check(lib.cffm_mlp_fwd(*fwd_args(wt, t, pix, fo), P(x2), NP, st), lib)
    # what a backward reads, and the rows of dy, each behind PAD rows of NaN: one row read at or past NP poisons the output
    nan_rows = lambda v: torch.cat([v, torch.full((PAD,) + tuple(v.shape[1:]), float('nan'), device=device)])
    settle(device)
    sv = {k: nan_rows(fo[k]) for k in ('hraw', 'x1', 'mean2', 'rstd2')}
    dout = nan_rows(t['dy'].permute(0, 2, 1).reshape(NP, 256).contiguous())
    bo = bwd_outputs(device, NP)
    _lib.check(lib.cffm_mlp_bwd(P(dout), *bwd_args(wt, sv, bo, NP, st)), lib)
    settle(device)
    bo['dout_rows'] = torch.cat([dout[:NP], torch.full((PAD, 256), SENTINEL, device=device)])
    return dict(t=t, fwd=fo, x2=x2, saved=sv, bwd=bo)


def run_fwd_stage(lib, device, nimg, pix, frames):
    wt, ref = weights(device), reference(device, nimg, pix)
    NP, img = nimg * pix, pix * 256
    st = stream_of(device)
    # the rows form's x2 through cffm_transpose into the target frames of a sentinel-filled destination
    want = torch.full((nimg * frames * img + GUARD,), SENTINEL, device=device)
    _lib.check(lib.cffm_transpose(P(ref['x2']), P(want, (frames - 1) * img), nimg, pix, 256, img, frames * img, st), lib)
    # the NCHW form
    o = fwd_outputs(device, NP)
    got = torch.full((nimg * frames * img + GUARD,), SENTINEL, device=device)
    _lib.check(lib.cffm_mlp_fwd_nchw(*fwd_args(wt, ref['t'], pix, o), P(got, (frames - 1) * img), frames * img, NP, st), lib)
    settle(device)
    body = got[:nimg * frames * img].view(nimg, frames, 256, pix)
    assert not torch.isnan(body[:, -1]).any() and not bool((body[:, -1] == SENTINEL).any()), 'target frame not fully written'
    assert bool((body[:, :-1] == SENTINEL).all()), 'a frame in front of a target frame was written'
    assert bool((got[nimg * frames * img:] == SENTINEL).all()), 'the guard region behind the destination was written'
    assert same(got, want), 'target frames differ from rows form + transpose (%d x %d, %d frames)' % (nimg, pix, frames)
    for k in o:
        assert same(o[k], ref['fwd'][k]), '%s differs from the rows form' % k


@pytest.mark.parametrize('frames', STRIDES)
@pytest.mark.parametrize('nimg,pix', CASES)
def test_mlp_fwd_nchw_emulated(nimg, pix, frames):
    run_fwd_stage(emu.lib(), torch.device('cpu'), nimg, pix, frames)


@pytest.mark.gpu
@pytest.mark.parametrize('frames', STRIDES)
@pytest.mark.parametrize('nimg,pix', CASES)
def test_mlp_fwd_nchw_gpu(nimg, pix, frames):
    run_fwd_stage(_lib.get(), torch.device('cuda:0'), nimg, pix, frames)


def run_bwd_stage(lib, device, nimg, pix, frames):
    """cffm_mlp_bwd_nchw on dy in NCHW (images `frames` frames apart, NaN in the other frames and behind the buffer) against cffm_mlp_bwd
    on the rows of dy: dh, dx1, dao, the emitted dout rows, and the five bias / norm gradients -- the record arrays of the launch, summed in
    the same fixed order by the same reduction.  The rows form's operand is made with torch here; that cffm_transpose gives these rows is
    checked on top."""
    wt, ref = weights(device), reference(device, nimg, pix)
    NP, img = nimg * pix, pix * 256
    st = stream_of(device)
    nan = float('nan')
    dy = torch.full((nimg, frames, 256, pix), nan, device=device)
    dy[:, -1] = ref['t']['dy']
    dy = torch.cat([dy.reshape(-1), torch.full((GUARD,), nan, device=device)])
    rows = torch.empty(NP, 256, device=device)
    _lib.check(lib.cffm_transpose(P(dy, (frames - 1) * img), P(rows), nimg, 256, pix, frames * img, img, st), lib)
    o = bwd_outputs(device, NP)
    o['dout_rows'] = torch.full((NP + PAD, 256), SENTINEL, device=device)
    _lib.check(lib.cffm_mlp_bwd_nchw(P(dy, (frames - 1) * img), frames * img, pix, P(o['dout_rows']), *bwd_args(wt, ref['saved'], o, NP, st)), lib)
    settle(device)
    assert same(rows, ref['bwd']['dout_rows'][:NP])
    for k in o:
        assert not torch.isnan(o[k]).any(), '%s: NaN (a read outside the target frames or past NP)' % k
        assert same(o[k], ref['bwd'][k]), '%s differs from the rows form fed the transposed gradient (%d x %d, %d frames)' % (k, nimg, pix, frames)


@pytest.mark.parametrize('frames', STRIDES)
@pytest.mark.parametrize('nimg,pix', CASES)
def test_mlp_bwd_nchw_emulated(nimg, pix, frames):
    run_bwd_stage(emu.lib(), torch.device('cpu'), nimg, pix, frames)


@pytest.mark.gpu
@pytest.mark.parametrize('frames', STRIDES)
@pytest.mark.parametrize('nimg,pix', CASES)
def test_mlp_bwd_nchw_gpu(nimg, pix, frames):
    run_bwd_stage(_lib.get(), torch.device('cuda:0'), nimg, pix, frames)


# ---------------------------------------------------------------------------------------------- layer level
def flat_params(st, depth, device):
    return [st['blocks.%d.%s' % (i, k)].clone().to(device) for i in range(depth) for k, _, _ in ops.BLOCK_PARAM_KEYS]


def transpose(lib, src, src_off, dst, dst_off, batch, rows, cols, src_bs, dst_bs, st):
    _lib.check(lib.cffm_transpose(P(src, src_off), P(dst, dst_off), batch, rows, cols, src_bs, dst_bs, st), lib)


def run_layer_training(lib, device, case):
    """y, dx and every parameter gradient of the NCHW entry points equal, bit for bit, those of: transpose to rows, the rows entry points,
    transposes back (+ the pass-through frames of y and of dy)."""
    b, h, w, depth, state, x, _ = H.layer_case_inputs(H.load_golden(case))
    hw, img = h * w, h * w * 256
    x = x.to(device).contiguous()
    dy = R.synth_input('g', (b, 4, 256, h, w), seed=2, scale=1.0).to(device).contiguous()
    params = flat_params(state, depth, device)
    st = stream_of(device)
    g = ops.make_geom(lib, b, h, w)
    ks, qd, ip, ii = ops.device_tables(h, w, device)
    ps = ops.block_structs(params, depth)

    def buffers():
        saved, scratch = ops._layer_buffers(lib, g, depth, device)
        grads = [torch.full_like(p, SENTINEL) for p in params]
        return saved.fill_(float('nan')), scratch.fill_(float('nan')), grads, ops.block_structs(grads, depth)

    # ---- the NCHW entry points
    saved, scratch, grads_a, gs = buffers()
    y_a, dx_a = torch.full_like(x, SENTINEL), torch.full_like(x, SENTINEL)
    _lib.check(lib.cffm_layer_forward_full(C.byref(g), depth, ps, P(x), P(y_a), P(ks), P(qd), P(saved), P(scratch), st), lib)
    _lib.check(lib.cffm_layer_backward_full(C.byref(g), depth, ps, gs, P(dy), P(dx_a), P(ks), P(qd), P(ip), P(ii), P(saved), P(scratch),
                                            depth - 1, 0, st), lib)
    settle(device)
    # ---- the same through token rows
    saved, scratch, grads_b, gs = buffers()
    x_rows, y_rows, dy_rows = torch.empty(b, 4, hw, 256, device=device), torch.empty(b, hw, 256, device=device), torch.empty(b, hw, 256, device=device)
    dx_rows, y_b, dx_b = torch.empty(b, 4, hw, 256, device=device), x.clone(), torch.empty_like(x)
    transpose(lib, x, 0, x_rows, 0, 4 * b, 256, hw, img, img, st)
    _lib.check(lib.cffm_layer_forward_rows(C.byref(g), depth, ps, P(x_rows), P(y_rows), P(ks), P(qd), P(saved), P(scratch), st), lib)
    transpose(lib, y_rows, 0, y_b, 3 * img, b, hw, 256, img, 4 * img, st)
    transpose(lib, dy, 3 * img, dy_rows, 0, b, 256, hw, 4 * img, img, st)
    _lib.check(lib.cffm_layer_backward_rows(C.byref(g), depth, ps, gs, P(x_rows), P(dy_rows), P(dx_rows), P(ks), P(qd), P(ip), P(ii), P(saved),
                                            P(scratch), st), lib)
    transpose(lib, dx_rows, 0, dx_b, 0, 4 * b, hw, 256, img, img, st)
    settle(device)
    dx_b[:, :3] += dy[:, :3]
    assert same(y_a, y_b), 'layer output differs'
    assert torch.isfinite(dx_a).all() and same(dx_a, dx_b), 'input gradient differs'
    for i, (ga, gb) in enumerate(zip(grads_a, grads_b)):
        assert torch.isfinite(ga).all() and same(ga, gb), 'gradient of parameter %d (%s) differs' % (i, ops.BLOCK_PARAM_KEYS[i % ops.NPB][0])


LAYER_TRAIN_CASES = ['layer_b1_8x8_d1', 'layer_b2_8x8_d2']        # the smallest grid of the goldens, depth 1 and depth 2


@pytest.mark.parametrize('case', LAYER_TRAIN_CASES)
def test_layer_full_equals_rows_plus_transposes_emulated(case):
    with emu.active():
        run_layer_training(emu.lib(), torch.device('cpu'), case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', LAYER_TRAIN_CASES)
def test_layer_full_equals_rows_plus_transposes_gpu(case):
    run_layer_training(_lib.get(), torch.device('cuda:0'), case)


def run_layer_infer(lib, device, b, h, w, depth):
    """cffm_layer_infer_full == transpose, cffm_layer_infer_rows, transpose; the pass-through frames are the input's."""
    hw, img = h * w, h * w * 256
    state = R.layer_state(depth, seed=71)
    x = R.synth_input('x', (b, 4, 256, h, w), seed=72).to(device).contiguous()
    params = flat_params(state, depth, device)
    prepared = ops.layer_prepare(depth, params)
    st = stream_of(device)
    g = ops.make_geom(lib, b, h, w)
    ks, qd = ops.device_tables(h, w, device)[:2]
    ps = ops.block_structs(params, depth)
    nan = float('nan')
    ws = torch.full((lib.cffm_layer_infer_ws_floats(C.byref(g)),), nan, device=device)
    y_a = torch.full_like(x, nan)
    _lib.check(lib.cffm_layer_infer_full(C.byref(g), depth, ps, P(prepared), P(x), P(y_a), P(ks), P(qd), P(ws), st), lib)
    settle(device)
    ws.fill_(nan)
    x_rows, y_rows, y_b = torch.empty(b, 4, hw, 256, device=device), torch.empty(b, hw, 256, device=device), x.clone()
    transpose(lib, x, 0, x_rows, 0, 4 * b, 256, hw, img, img, st)
    _lib.check(lib.cffm_layer_infer_rows(C.byref(g), depth, ps, P(prepared), P(x_rows), P(y_rows), P(ks), P(qd), P(ws), st), lib)
    transpose(lib, y_rows, 0, y_b, 3 * img, b, hw, 256, img, 4 * img, st)
    settle(device)
    assert torch.isfinite(y_a).all() and same(y_a, y_b)


# depth 1 (the residual rows are frame 3 of the stack that lives in the output: rows + transpose stay), depth 2 (NCHW form) on 2 x 8 x 8
# (an image boundary inside a panel) and on 1 x 33 x 34 = 1122 rows (the 16-row panels of the inference kernel, a ragged last one)
LAYER_INFER_CASES = [(1, 8, 8, 1), (2, 8, 8, 2), (1, 33, 34, 2)]


@pytest.mark.parametrize('b,h,w,depth', LAYER_INFER_CASES)
def test_layer_infer_full_equals_rows_plus_transposes_emulated(b, h, w, depth):
    with emu.active():
        run_layer_infer(emu.lib(), torch.device('cpu'), b, h, w, depth)


@pytest.mark.gpu
@pytest.mark.parametrize('b,h,w,depth', LAYER_INFER_CASES)
def test_layer_infer_full_equals_rows_plus_transposes_gpu(b, h, w, depth):
    run_layer_infer(_lib.get(), torch.device('cuda:0'), b, h, w, depth)
