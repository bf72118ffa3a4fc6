"""The operand prefetches of the fused Mlp kernels (k_mlp_fwd / k_mlp_bwd, csrc/panel_kernels.h): the saved rows the
kernels read (the residual rows xt in the forward; hraw, x1, dout, mean2, rstd2 in the backward) are requested one phase ahead of
their use, for the NEXT hidden chunk while the current one is worked on.  What can go wrong is a row index: a request for rows at or
past NP, for a chunk past the last, from the wrong half of the double buffer, or across a clip boundary of the strided residual.  So
cffm_mlp_fwd / cffm_mlp_bwd are called through the C ABI at the row counts where the panels are ragged -- NP = 1 (a single partial
panel), 17 (a partial wave row), 32 (exactly one panel), 33 (one row into a second panel), 95 (a ragged last panel of three) -- and at
NP = 50 with 20 rows per clip (clip boundaries inside both panels, a partial last clip), with

  * every input followed by GUARD rows of NaN (and NaN in every unread slot of the strided residual): one row read from there
    poisons the output;
  * every output followed by GUARD rows of a sentinel, which must survive;
  * every output, saved intermediate and bias / norm gradient against fp64 torch autograd, tolerances of tests/test_panel.py
    (split-bf16 operands: 2e-5 of the result's norm; the LayerNorm statistics 1e-5);
  * a second call on the same inputs giving the same bits.

CPU: emulator build of the same sources; GPU: the product library."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import emu
from vss_cffm_amd import _lib

TOL, TOL_STAT = 2e-5, 1e-5       # tests/test_panel.py
GUARD = 48                       # rows behind NP: more than the largest panel (48 rows), so a panel that overruns NP lands in them
SENTINEL = 7.0
# (NP, rows per clip)
CASES = [(1, 1), (17, 17), (32, 32), (33, 33), (95, 95), (50, 20)]


def P(t):
    return C.c_void_p(t.data_ptr())


def rel(a, b):
    b = b.double()
    return float((a.double().cpu() - b.cpu()).norm() / b.norm().clamp_min(1e-30))


def unsplit4(t):
    """split-4 storage ({bf16 hi x4, bf16 lo x4} per 4 floats) -> float64 values."""
    raw = t.detach().cpu().contiguous().view(torch.int16).reshape(-1, 8).to(torch.int32)
    hi = (raw[:, :4] << 16).view(torch.float32).double()
    lo = (raw[:, 4:] << 16).view(torch.float32).double()
    return (hi + lo).reshape(t.shape)


@functools.lru_cache(maxsize=None)
def case(NP, rpb):
    """Inputs and the fp64 reference of one case (made once, shared by the emulator and the GPU test, never modified)."""
    gen = torch.Generator().manual_seed(1000 + NP)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=gen) * scale
    nb = (NP + rpb - 1) // rpb
    t = dict(wp=rn(256, 256, scale=0.08), w1=rn(1024, 256, scale=0.08), w2=rn(256, 1024, scale=0.05), bp=rn(256, scale=0.1),
             b1=rn(1024, scale=0.1), b2=rn(256, scale=0.1), g2=1 + rn(256, scale=0.2), be2=rn(256, scale=0.1), ao=rn(NP, 256),
             xt=rn(NP, 256, scale=1.5), dout=rn(NP, 256))
    d = {k: v.double().requires_grad_(True) for k, v in t.items() if k != 'dout'}
    x1 = d['xt'] + d['ao'] @ d['wp'].T + d['bp']
    z2 = F.layer_norm(x1, (256,), d['g2'], d['be2'], 1e-5)
    h = z2 @ d['w1'].T
    h.retain_grad(); x1.retain_grad()
    act = F.gelu(h + d['b1'])
    x2 = x1 + act @ d['w2'].T + d['b2']
    x2.backward(t['dout'].double())
    x1d = x1.detach()
    ref = dict(x1=x1d, z2=z2.detach(), hraw=h.detach(), act=act.detach(), x2=x2.detach(), mean2=x1d.mean(1),
               rstd2=1 / torch.sqrt(x1d.var(1, unbiased=False) + 1e-5), dh=h.grad, dx1=x1.grad, dao=d['ao'].grad, dg2=d['g2'].grad,
               dbe2=d['be2'].grad, db1=d['b1'].grad, db2=d['b2'].grad, dbp=d['bp'].grad)
    # the residual as the layer passes it: slot 3 of a [clips, 4, rows per clip, 256] stack; everything the kernel must not read is NaN
    rows = torch.full(((nb + 1) * rpb, 256), float('nan'))
    rows[:NP] = t['xt']
    stack = torch.full((nb + 1, 4, rpb, 256), float('nan'))
    stack[:, 3] = rows.view(nb + 1, rpb, 256)
    return t, ref, stack, nb


def guarded(rows, device):
    """Input rows followed by GUARD rows of NaN."""
    out = torch.full((rows.shape[0] + GUARD,) + tuple(rows.shape[1:]), float('nan'), device=device)
    out[:rows.shape[0]] = rows.to(device)
    return out


def run_case(lib, device, NP, rpb):
    t, ref, stack, nb = case(NP, rpb)
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == 'cuda' else None
    dev = lambda x: x.to(device).contiguous()
    frag = {}
    for name in ('wp', 'w1', 'w2'):
        for form in (0, 1):
            out = torch.empty(t[name].numel(), device=device)
            _lib.check(lib.cffm_panel_pack_weight(P(dev(t[name])), t[name].shape[0], t[name].shape[1], form, P(out), stream), lib)
            frag[name, form] = out
    pd = {k: dev(t[k]) for k in ('bp', 'b1', 'b2', 'g2', 'be2')}
    ao_d, dout_d, stack_d = guarded(t['ao'], device), guarded(t['dout'], device), dev(stack)
    xt_d = stack_d[:, 3]
    mk = lambda *s: torch.full(s, SENTINEL, device=device)
    NG = NP + GUARD

    def forward():
        o = dict(x1=mk(NG, 256), z2s=mk(NG, 256), mean2=mk(NG), rstd2=mk(NG), hraw=mk(NG, 1024), acts=mk(NG, 1024), x2=mk(NG, 256))
        _lib.check(lib.cffm_mlp_fwd(P(ao_d), P(xt_d), 4 * rpb * 256, rpb, P(frag['wp', 0]), P(frag['w1', 0]), P(frag['w2', 0]), P(pd['bp']),
                                    P(pd['b1']), P(pd['b2']), P(pd['g2']), P(pd['be2']), P(o['x1']), P(o['z2s']), P(o['mean2']), P(o['rstd2']),
                                    P(o['hraw']), P(o['acts']), P(o['x2']), NP, stream), lib)
        return o

    def backward(saved):
        o = dict(dhs=mk(NG, 1024), dx1=mk(NG, 256), dao=mk(NG, 256), dg2=mk(256), dbe2=mk(256), db1=mk(1024), db2=mk(256), dbp=mk(256))
        _lib.check(lib.cffm_mlp_bwd(P(dout_d), P(saved['hraw']), P(pd['b1']), P(saved['x1']), P(saved['mean2']), P(saved['rstd2']), P(pd['g2']),
                                    P(frag['w2', 1]), P(frag['w1', 1]), P(frag['wp', 1]), P(o['dhs']), P(o['dx1']), P(o['dao']), P(o['dg2']),
                                    P(o['dbe2']), P(o['db1']), P(o['db2']), P(o['dbp']), NP, stream), lib)
        return o

    def settle(o):
        if device.type == 'cuda':
            torch.cuda.synchronize(device)
        return {k: v.cpu() for k, v in o.items()}

    def check(o, rows, pairs, tag):
        for k, v in o.items():
            body = v[:NP] if k in rows else v
            assert not torch.isnan(body).any(), '%s %s: NaN (NP = %d)' % (tag, k, NP)
            if k in rows:
                assert bool((v[NP:] == SENTINEL).all()), '%s %s: rows at or past NP = %d were written' % (tag, k, NP)
        for k, got, want, tol in pairs:
            err = rel(got, want)
            print('%s NP=%d rpb=%d %-6s rel err %.3g (bound %.0e)' % (tag, NP, rpb, k, err, tol))
            assert err < tol, (tag, k, NP, err)

    fo = settle(forward())
    fwd_rows = ('x1', 'z2s', 'mean2', 'rstd2', 'hraw', 'acts', 'x2')
    check(fo, fwd_rows, [('x1', fo['x1'][:NP], ref['x1'], TOL), ('x2', fo['x2'][:NP], ref['x2'], TOL), ('hraw', fo['hraw'][:NP], ref['hraw'], TOL),
                         ('acts', unsplit4(fo['acts'][:NP]), ref['act'], TOL), ('z2s', unsplit4(fo['z2s'][:NP]), ref['z2'], TOL),
                         ('mean2', fo['mean2'][:NP], ref['mean2'], TOL_STAT), ('rstd2', fo['rstd2'][:NP], ref['rstd2'], TOL_STAT)], 'fwd')
    # the backward reads what the forward saved, behind NaN guard rows of its own
    saved = {k: guarded(fo[k][:NP], device) for k in ('hraw', 'x1', 'mean2', 'rstd2')}
    bo = settle(backward(saved))
    check(bo, ('dhs', 'dx1', 'dao'), [('dhs', unsplit4(bo['dhs'][:NP]), ref['dh'], TOL), ('dx1', bo['dx1'][:NP], ref['dx1'], TOL),
                                      ('dao', bo['dao'][:NP], ref['dao'], TOL), ('dg2', bo['dg2'], ref['dg2'], TOL), ('dbe2', bo['dbe2'], ref['dbe2'], TOL),
                                      ('db1', bo['db1'], ref['db1'], TOL), ('db2', bo['db2'], ref['db2'], TOL), ('dbp', bo['dbp'], ref['dbp'], TOL)], 'bwd')
    # determinism: the same inputs give the same bits
    fo2, bo2 = settle(forward()), settle(backward(saved))
    for a, b in ((fo, fo2), (bo, bo2)):
        for k in a:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), '%s differs between two calls (NP = %d)' % (k, NP)
    return fo, bo


@pytest.mark.parametrize('NP,rpb', CASES)
def test_mlp_operand_prefetch_emulated(NP, rpb):
    with emu.active():
        run_case(emu.lib(), torch.device('cpu'), NP, rpb)


@pytest.mark.gpu
@pytest.mark.parametrize('NP,rpb', CASES)
def test_mlp_operand_prefetch_gpu(NP, rpb):
    run_case(_lib.get(), torch.device('cuda:0'), NP, rpb)
