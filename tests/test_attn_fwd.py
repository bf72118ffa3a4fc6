"""The attention forward on its own (cffm_attn_fwd: k_cfm_attn_fwd of csrc/cfm_attn_kernels.h) against an fp64 evaluation of the same
windowed cross-attention on the same f16 q|k|v rows and the same f16 bias: the attention output of every pixel and the log-sum-exp
of every (window, head, query).
Reference semantics: cffm_transformer.py:364-606; the key assembly comes from geometry.tables, which
tests/test_geometry.py pins against the oracle's roll / unfold maps.

1. parity (run_parity): `exact` is fp64 throughout; the `restatement` is the same fp64 evaluation with ONE step changed, the weights
   exp(s - max) rounded to f16 before the product with V and before the row sum -- what the kernel documents it does.  The kernel may be
   twice as far from `exact` as the restatement is (it also has fp32 logits and a hardware exp2), no more; neither gate is a number
   chosen in advance.  DESIGN.md ("The stage test of the attention forward") holds the measured columns.
2. selection probe (run_selection): q = 0 and a bias of +100 on one key slot per (head, query) make every logit exactly 0 or 100, every
   other weight underflows to 0 in f16: the output must BE the selected key's f16 V row and the log-sum-exp must BE 100.0 -- every
   gather address, validity flag, bias fragment, V^T read and destination pixel, bit for bit.
3. what is written and what is read (run_write_read).
4. the forward's own ao / lse handed to the backward (run_fwd_into_bwd), judged like tests/test_attn_bwd.py judges the reference's."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import emu
from tests.test_attn_bwd import P, bias_buffer, check, run_attn_bwd_stage, stage_inputs
from vss_cffm_amd import _lib, ops

GUARD = 4            # sentinel rows behind qkv / ao / lse
SENTINEL = -7.0
NAN = float('nan')
CPU = torch.device('cpu')


def make_inputs(b, h0, w0, qk_scale=0.7, v_scale=1.0, bias_scale=0.5):
    torch.manual_seed(b * 1000 + h0 * 31 + w0)
    nw = ((h0 + 6) // 7) * ((w0 + 6) // 7)
    x = torch.randn(b * 64 * nw, 768)
    x[:, :512] *= qk_scale
    x[:, 512:] *= v_scale
    bias = torch.randn(8, 64, 304) * bias_scale
    bias[:, 49:] = 0
    bias[:, :, 289:] = 0
    return x.half(), bias


def stream_of(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == 'cuda' else None


def call_fwd(lib, device, g, qkv, ks, qd, bias_h, ao, lse):
    """every argument is a tensor the CALLER holds by name across the call (a temporary's storage may be reused before the kernel ran)"""
    return lib.cffm_attn_fwd(C.byref(g), P(qkv), P(ks), P(qd), P(bias_h), P(ao), P(lse), stream_of(device))


def forward(lib, device, b, h0, w0, qkv, bias, on_device=False):
    """-> ao [b, HW, 256], lse [b, nW, 8, 64] (on the CPU unless on_device); the outputs are prefilled with NaN"""
    g = ops.make_geom(lib, b, h0, w0)
    ks_t, qd_t, _, _ = ops.device_tables(h0, w0, device)
    qkv_d, bias_d = qkv.contiguous().to(device), bias_buffer(bias).to(device)
    ao = torch.full((b * g.HW, 256), NAN, device=device)
    lse = torch.full((b * g.nW * 8, 64), NAN, device=device)
    _lib.check(call_fwd(lib, device, g, qkv_d, ks_t, qd_t, bias_d, ao, lse), lib)
    if on_device:
        return ao, lse.view(b, g.nW, 8, 64)
    return ao.cpu().view(b, g.HW, 256), lse.cpu().view(b, g.nW, 8, 64)


def tables(h0, w0):
    ks, qd, _, _ = ops.device_tables(h0, w0, CPU)
    nw, hw = ks.shape[0], h0 * w0
    # every pixel is the destination of exactly one query: the rows compared below are the whole of ao
    assert torch.equal(torch.sort(qd[qd >= 0].view(-1).long()).values, torch.arange(hw))
    return ks, qd, nw, hw


def reference(qkv, bias, ks, b, nw):
    """fp64, from the float values of the f16 rows and of bias.half().  -> (o, lse) exact, (o, lse) of the restatement with f16-rounded
    weights, the row maximum, max |s| per (clip, window, head, query) and max |v| per (clip, window, head) over the present keys"""
    x = qkv.double().view(b, 64 * nw, 768)
    q = x[:, :49 * nw, :256].reshape(b, nw, 49, 8, 32).permute(0, 1, 3, 2, 4)
    idx = ks[:, :289].long().clamp_min(0).view(-1)
    valid = (ks[:, :289] >= 0).view(1, nw, 1, 1, 289)
    gat = lambda t: t[:, idx].view(b, nw, 289, 8, 32).permute(0, 1, 3, 2, 4)
    k, v = gat(x[:, :, 256:512]), gat(x[:, :, 512:])
    s = q @ k.transpose(-1, -2) + bias.half().double()[None, None, :, :49, :289]
    smax = s.masked_fill(~valid, 0).abs().amax(-1)
    vmax = (v.abs().amax(-1) * valid.view(1, nw, 1, 289)).amax(-1)
    s = s.masked_fill(~valid, float('-inf'))
    m = s.amax(-1, keepdim=True)
    wgt = torch.exp(s - m)
    del s, k
    out = []
    for w_ in (wgt, wgt.float().half().double()):
        l = w_.sum(-1, keepdim=True)
        out += [(w_ @ v) / l, (m + torch.log(l)).squeeze(-1)]
    return out[0], out[1], out[2], out[3], m.squeeze(-1), smax, vmax


def dest_rows(ao, qd, b, nw):
    """ao [b, HW, 256] -> [b, nW, 8, 49, 32]: the row each query was scattered to (a query without a pixel shows pixel 0's: mask it)"""
    return ao.view(b, -1, 8, 32)[:, qd.view(-1).long().clamp_min(0)].view(b, nw, 49, 8, 32).permute(0, 1, 3, 2, 4)


def ulp32(x):
    """spacing of fp32 at |x| (fp64 magnitudes in, fp64 out)"""
    return torch.from_numpy(np.spacing(x.abs().float().numpy()).astype(np.float64))


def run_parity(lib, device, shape, qk_scale=0.7, v_scale=1.0, bias_scale=0.5):
    b, h0, w0 = shape
    ks, qd, nw, hw = tables(h0, w0)
    qkv, bias = make_inputs(b, h0, w0, qk_scale, v_scale, bias_scale)
    ao, lse = forward(lib, device, b, h0, w0, qkv, bias)
    o_ex, lse_ex, o_rs, lse_rs, m, smax, vmax = reference(qkv, bias, ks, b, nw)
    assert bool(torch.isfinite(ao).all()) and bool(torch.isfinite(lse).all())
    assert float(lse[..., 49:].abs().max()) == 0
    has_px = (qd >= 0).view(1, nw, 1, 49, 1)
    err_k = (dest_rows(ao.double(), qd, b, nw) - o_ex).abs() * has_px
    err_r = (o_rs - o_ex).abs() * has_px
    scale = float((o_ex.abs() * has_px).max())
    lerr_k = (lse[..., :49].double() - lse_ex).abs()
    lgate = 2 * float((lse_rs - lse_ex).abs().max()) + 4 * ulp32(smax)
    # |ao - exact| <= (2^-10 + 2^-18 max|s|) max|v|: numerator and denominator each carry the 2^-11 of an f16 weight, and a logit error of
    # 2^-19 |s| (32 fp32 products, a bias, the exponent's FMA) moves a weight by that fraction twice over
    cap = (2.0 ** -10 + 2.0 ** -18 * smax).unsqueeze(-1) * vmax.view(b, nw, 8, 1, 1)
    fig = {'ao_kernel': float(err_k.max()) / scale, 'ao_restated': float(err_r.max()) / scale, 'lse_kernel': float(lerr_k.max()),
           'lse_restated': float((lse_rs - lse_ex).abs().max()), 'lse_of_gate': float((lerr_k / lgate).max()),
           'cap_used': float((err_k / cap).max()), 'max_s': float(smax.max()), 'mean_top_weight': float(torch.exp(m - lse_ex).mean())}
    print('attn_fwd parity', shape, (qk_scale, v_scale, bias_scale), {k: '%.3g' % v for k, v in fig.items()})
    assert fig['ao_kernel'] <= 2 * fig['ao_restated'], fig
    assert bool((lerr_k <= lgate).all()), fig
    assert bool((err_k <= cap).all()), fig
    return fig


# (1, 1, 1): one valid query; (7, 7): one window that is its own neighbour; (8, 8): 2 x 2 windows, every direction wraps, 326 masked keys;
# (6, 15), (5, 20): ragged, one row of windows; (13, 30): ragged on both axes, two clips (the clip offset); (22, 23): 16 windows
SHAPES = [(1, 1, 1), (1, 7, 7), (1, 8, 8), (2, 6, 15), (1, 5, 20), (2, 13, 30), (1, 22, 23)]
# (q|k scale, v scale, bias scale): peaked softmaxes (mean largest weight ~0.95, |s| ~ 180); |s| ~ 1800; a uniform softmax over the present
# keys (the case most sensitive to a wrong mask); large V
CONDITIONS = {'peaked': (2.5, 1.0, 4.0), 'large_logits': (8.0, 1.0, 0.5), 'uniform': (0.01, 1.0, 0.0), 'large_v': (0.7, 30.0, 0.5)}
COND_CASES = [(s, c) for s in ((1, 8, 8), (2, 13, 30)) for c in CONDITIONS]


# --------------------------------------------------------------------------------------------------------------------------------
def selection_schedule(ks, qd):
    """passes of slots [8 heads, 49 queries] such that every (window, head, present slot) is chosen at least once by a query that has a
    pixel.  The bias is shared by the windows, so a pass chooses per (head, query); the window with the fewest pixels sets the number of
    passes (one pixel: 289).  Greedy for one head: each query takes the slot still missing in most of its windows; head h runs the same
    passes rotated by h, so no two heads carry the same bias in a call."""
    valid, dest = (ks[:, :289] >= 0).numpy(), (qd >= 0).numpy()
    need, base = valid.copy(), []
    while need.any():
        slots = np.zeros(49, dtype=np.int64)
        for q in range(49):
            wq = np.nonzero(dest[:, q])[0]
            score = need[wq].sum(0) if len(wq) else np.zeros(289, dtype=np.int64)
            slots[q] = int(np.argmax(score)) if score.max() > 0 else (q + 49 * len(base)) % 289
            need[wq, slots[q]] = False
        base.append(slots)
    n = len(base)
    return [np.stack([base[(p + h) % n] for h in range(8)]) for p in range(n)]


def run_selection(lib, device, shape, part=0, parts=1):
    """part / parts: this call runs every parts-th pass of the schedule (the emulator spends ~0.1 s on a launch: its cases are split so
    that each stays at a few seconds); the schedule's coverage is asserted whole in every part"""
    b, h0, w0 = shape
    ks, qd, nw, hw = tables(h0, w0)
    g = ops.make_geom(lib, b, h0, w0)
    ks_t, qd_t, _, _ = ops.device_tables(h0, w0, device)
    qkv, _ = make_inputs(b, h0, w0)
    qkv[:, :256] = 0
    qkv_d = qkv.to(device)
    valid, dest = ks[:, :289] >= 0, qd >= 0                                  # [nW, 289], [nW, 49]
    vrows = qkv.float().view(b, 64 * nw, 768)[:, :, 512:].reshape(b, 64 * nw, 8, 32)
    # an absent key selected: all present keys weigh the same
    v64 = vrows.double()[:, ks[:, :289].long().clamp_min(0).view(-1)].view(b, nw, 289, 8, 32) * valid.view(1, nw, 289, 1, 1)
    nvalid = valid.sum(1).double()                                            # [nW]
    vmean = (v64.sum(2) / nvalid.view(1, nw, 1, 1)).unsqueeze(3)              # [b, nW, 8, 1, 32]
    vmax = v64.abs().amax((2, 4)).view(b, nw, 8, 1, 1)
    lse_absent = torch.log(nvalid).view(1, nw, 1, 1)
    harange = torch.arange(8).view(1, 8, 1)
    covered = torch.zeros(nw, 8, 289, dtype=torch.bool)
    n_absent = n_absent_px = 0
    passes = selection_schedule(ks, qd)
    for i, slots in enumerate(passes):
        sl = torch.from_numpy(slots)                                         # [8, 49]
        for q in range(49):                                                  # slots chosen by queries that have a pixel
            covered[:, torch.arange(8), sl[:, q]] |= dest[:, q].view(nw, 1)
        if i % parts != part:
            continue
        bias = torch.zeros(8, 64, 304)
        bias[:, :49].scatter_(2, sl.unsqueeze(-1), 100.0)
        bias_d = bias_buffer(bias).to(device)
        ao = torch.full((b * hw, 256), NAN, device=device)
        lse = torch.full((b * nw * 8, 64), NAN, device=device)
        _lib.check(call_fwd(lib, device, g, qkv_d, ks_t, qd_t, bias_d, ao, lse), lib)
        got = dest_rows(ao.cpu().view(b, hw, 256), qd, b, nw)                # [b, nW, 8, 49, 32]
        lse = lse.cpu().view(b, nw, 8, 64)[..., :49]
        src = ks[:, sl]                                                      # [nW, 8, 49]: the row of the selected slot, -1 = absent
        present = (src >= 0).unsqueeze(0).expand(b, -1, -1, -1)
        want = vrows[:, src.long().clamp_min(0), harange]                    # [b, nW, 8, 49, 32]
        px = dest.view(1, nw, 1, 49).expand(b, -1, 8, -1)
        assert torch.equal(got[present & px], want[present & px])            # the selected key's f16 V slice, bit for bit
        assert bool((lse[present] == 100.0).all())
        absent = ~present
        if bool(absent.any()):
            # part 1's cap at max|s| = 0; lse = log(number of present keys), computed by logf and stored in fp32: 4 ulp of it (the
            # restatement is exact here, so part 1's gate leaves only its ulp term, taken at the stored value: every logit is 0)
            assert bool(((got.double() - vmean).abs() <= 2.0 ** -10 * vmax)[absent & px].all())
            assert bool(((lse.double() - lse_absent).abs() <= 4 * ulp32(lse_absent))[absent].all())
            n_absent, n_absent_px = n_absent + int(absent.sum()), n_absent_px + int((absent & px).sum())
    want_cov = valid.view(nw, 1, 289).expand(-1, 8, -1)
    assert bool((covered & want_cov).eq(want_cov).all()), 'coverage %d of %d' % (int((covered & want_cov).sum()), int(want_cov.sum()))
    print('attn_fwd selection', shape, 'part', part, 'of', parts, 'passes', len(passes), 'slots covered', int(want_cov.sum()) * b,
          'absent selections (with a pixel)', n_absent, n_absent_px)
    # the absent-key branch of the check ran: these grids all have pooled cells off the grid ((1, 1, 1): its one pixel's query takes
    # the present slots only, the 48 queries without a pixel show the absent ones through lse)
    assert n_absent > 0 and (n_absent_px > 0 or shape == (1, 1, 1))


# --------------------------------------------------------------------------------------------------------------------------------
def run_write_read(lib, device, shape):
    b, h0, w0 = shape
    ks, qd, nw, hw = tables(h0, w0)
    g = ops.make_geom(lib, b, h0, w0)
    ks_t, qd_t, _, _ = ops.device_tables(h0, w0, device)
    rc = 64 * nw
    qkv, bias = make_inputs(b, h0, w0)
    bias_d = bias_buffer(bias).to(device)

    def guarded(rows, cols, dtype, body):
        t = torch.full((rows + GUARD, cols), SENTINEL, dtype=dtype)
        t[:rows] = body
        return t.to(device)

    def run(qkv_rows, geom=g, nb=b):
        qkv_g = guarded(nb * rc, 768, torch.float16, qkv_rows)
        before = qkv_g.clone()
        ao = guarded(nb * hw, 256, torch.float32, NAN)
        lse = guarded(nb * nw * 8, 64, torch.float32, NAN)
        _lib.check(call_fwd(lib, device, geom, qkv_g, ks_t, qd_t, bias_d, ao, lse), lib)
        ao, lse, after = ao.cpu(), lse.cpu(), qkv_g.cpu()
        assert bool((ao[nb * hw:] == SENTINEL).all()) and bool((lse[nb * nw * 8:] == SENTINEL).all())
        assert torch.equal(after.view(torch.int16), before.cpu().view(torch.int16))           # the input rows and their guard
        ao, lse = ao[:nb * hw], lse[:nb * nw * 8]
        assert bool(torch.isfinite(ao).all())                                                # every row of ao is written
        assert bool(torch.isfinite(lse[:, :49]).all()) and bool((lse[:, 49:] == 0).all())    # (an exact 0, not NaN)
        return ao, lse

    ao, lse = run(qkv)
    ao2, lse2 = run(qkv)
    assert torch.equal(ao, ao2) and torch.equal(lse, lse2)                   # the same bits on a repeated call
    # the q third of the pooled rows (rows >= 49 nW of each clip) holds no query: never read
    poisoned = qkv.clone()
    poisoned.view(b, rc, 768)[:, 49 * nw:, :256] = NAN
    ao3, lse3 = run(poisoned)
    assert torch.equal(ao, ao3) and torch.equal(lse, lse3)
    # two clips in one call = the clips one by one
    q2, _ = make_inputs(2, h0, w0, qk_scale=0.9)
    g1, g2 = ops.make_geom(lib, 1, h0, w0), ops.make_geom(lib, 2, h0, w0)
    ao_b2, lse_b2 = run(q2, g2, 2)
    for i in range(2):
        ao_i, lse_i = run(q2[i * rc:(i + 1) * rc], g1, 1)
        assert torch.equal(ao_b2[i * hw:(i + 1) * hw], ao_i) and torch.equal(lse_b2[i * nw * 8:(i + 1) * nw * 8], lse_i)
    # a null argument: refused with a message, nothing launched (the outputs keep their NaN)
    qkv_d = qkv.to(device)
    ao_n, lse_n = torch.full((b * hw, 256), NAN, device=device), torch.full((b * nw * 8, 64), NAN, device=device)
    good = [C.byref(g), P(qkv_d), P(ks_t), P(qd_t), P(bias_d), P(ao_n), P(lse_n)]
    for i in range(len(good)):
        args = list(good)
        args[i] = None
        assert lib.cffm_attn_fwd(*args, stream_of(device)) != 0, i
        assert b'attn_fwd' in lib.cffm_last_error(), i
    assert bool(torch.isnan(ao_n.cpu()).all()) and bool(torch.isnan(lse_n.cpu()).all())


# --------------------------------------------------------------------------------------------------------------------------------
def run_fwd_into_bwd(lib, device, shape):
    """cffm_attn_bwd on the forward kernel's own ao and lse, against the autograd reference and the gates of tests/test_attn_bwd.py"""
    b, h0, w0 = shape
    qkv, bias, _ = stage_inputs(b, h0, w0)
    ao, lse = forward(lib, device, b, h0, w0, qkv, bias, on_device=True)
    errs = run_attn_bwd_stage(lib, device, b, h0, w0, ao=ao, lse=lse)
    print('attn_fwd -> attn_bwd', shape, {k: '%.2e' % v for k, v in errs.items() if '_' not in k})
    check(errs)


# ---- emulator -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES)
def test_attn_fwd_parity_emulated(shape):
    run_parity(emu.lib(), CPU, shape)


@pytest.mark.parametrize('shape,cond', COND_CASES)
def test_attn_fwd_parity_conditioning_emulated(shape, cond):
    run_parity(emu.lib(), CPU, shape, *CONDITIONS[cond])


# (1, 8, 8): the window with one pixel needs a pass per present slot, 214; (1, 1, 1): 191; (2, 13, 30): 19 passes of 160 workgroups
@pytest.mark.parametrize('shape,part,parts', [(s, i, n) for s, n in (((1, 8, 8), 8), ((2, 13, 30), 3), ((1, 1, 1), 3)) for i in range(n)])
def test_attn_fwd_selection_emulated(shape, part, parts):
    run_selection(emu.lib(), CPU, shape, part, parts)


@pytest.mark.parametrize('shape', [(1, 8, 8), (2, 13, 30)])
def test_attn_fwd_write_read_emulated(shape):
    run_write_read(emu.lib(), CPU, shape)


@pytest.mark.parametrize('shape', [(1, 8, 8), (2, 13, 30)])
def test_attn_fwd_feeds_bwd_emulated(shape):
    run_fwd_into_bwd(emu.lib(), CPU, shape)


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
# (2, 60, 60): 1296 workgroups, the only case that fills four workgroups per CU (the kernel's declared occupancy)
@pytest.mark.parametrize('shape', SHAPES + [(2, 60, 60)])
def test_attn_fwd_parity_gpu(shape):
    run_parity(_lib.get(), torch.device('cuda'), shape)


@pytest.mark.gpu
@pytest.mark.parametrize('shape,cond', COND_CASES)
def test_attn_fwd_parity_conditioning_gpu(shape, cond):
    run_parity(_lib.get(), torch.device('cuda'), shape, *CONDITIONS[cond])


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(1, 8, 8), (2, 13, 30), (1, 1, 1), (1, 42, 42)])
def test_attn_fwd_selection_gpu(shape):
    run_selection(_lib.get(), torch.device('cuda'), shape)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(1, 8, 8), (2, 13, 30)])
def test_attn_fwd_write_read_gpu(shape):
    run_write_read(_lib.get(), torch.device('cuda'), shape)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(1, 8, 8), (2, 13, 30), (1, 42, 42)])
def test_attn_fwd_feeds_bwd_gpu(shape):
    run_fwd_into_bwd(_lib.get(), torch.device('cuda'), shape)
