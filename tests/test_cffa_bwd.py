"""The CFFA backward as a stage of the C ABI (cffm_ln_pool_bwd: k_ln_pool_bwd_tgt per block, k_ln_pool_bwd_ref<D> over the blocks' shared
reference frames, the record reductions and k_pool_matrix_bwd_n -- csrc/cffa_kernels.h, through the launch helpers the layer backward
runs) against fp64 torch autograd through a restatement of the stage: oracle.cffm_oracle.cffa_token_rows = F.layer_norm of the four
frames, zero padding, the target tokens in window order, pool_windows of the target, and for the reference frames F.interpolate
(bilinear) where the pooled grid differs from the padded one, then pool_windows -- rows in the order of cell_row.

The row order is anchored first: the restatement's forward equals the zall of cffm_ln_pool_fwd to 1e-5.  Then, with n blocks that
share the reference frames (each with its own target frame, norm1, pooling parameters and upstream gradient), every gradient is held
to GATE = 1e-5 (the gate of this fp32 stage's forward, tests/test_emu_kernels.py::run_stage_checks): dx_tgt, dgamma, dbeta, the four
pooling-weight gradients of every block and dx_ref (the sum over the blocks, plus the preloaded values with accum_ref) by
helpers.rel_err, the four scalar pool-bias gradients by plain relative error.  Such a gate means something only where the reference
quantity is not a cancelling sum, so the same restatement and autograd run in fp32 torch as well, and that reference-only result must
be within REF_GATE = 3e-6 of the fp64 one for every checked quantity.  For that reason the upstream gradient is noise with mean 0.5
(mean 0 at the one-pixel grid, where a mean makes pool_layers_clips.0.weight's gradient cancel) plus the stage's own forward output
(case_data), and the fp32 evaluation sums in a way that does not depend on torch's thread count (reference).  Measured on the MI355X
and its host, largest over the cases: kernels <= 4.3e-7, fp32 torch <= 1.23e-6 (dx_ref; the parameter gradients <= 8.2e-7); the table is
in DESIGN.md, section 3g.

Cases (the smallest at which each path can fail): one valid pixel of 49; one full window; 1x3 windows ragged on both axes with
n = 1..4 (every k_ln_pool_bwd_ref<D>) and n = 5 (a 4 + 1 pair of launches, the second accumulating), once with accum_ref on a
preloaded dx_ref; 2x3 windows.  The frames come as slots of [B,4,HW,256] stacks (clip stride 4 HW 256, the other slots NaN) or dense;
dres is NULL in one case.  Also per case: every output starts as NaN and comes back finite, sentinel rows behind dx_tgt / dx_ref and
the untouched slots of the stacks survive, the three floats behind each pooling tensor survive with cffm_grad_slices_padded(0) and
are zero with (1) (all but the 4-element weight, whose slice has no padding: nothing behind it is written), the dzall rows of padded target pixels have no influence (same bits), and a repeated call gives the same bits.
CPU: emulator build; GPU: product library."""
import ctypes as C
import functools

import pytest
import torch

from oracle import cffm_oracle as O, recipe as R
from tests import emu, helpers as H
from vss_cffm_amd import _lib, ops

GATE = 1e-5
REF_GATE = 3e-6
REF_PARTS = 16       # see reference()
GUARD = 4            # sentinel rows behind dx_tgt / dx_ref
SENTINEL = -7.0
NAN = float('nan')
POOL_W = ('pool_layers.0.weight', 'pool_layers_clips.0.weight', 'pool_layers_clips.1.weight', 'pool_layers_clips.2.weight')
POOL_B = ('pool_layers.0.bias', 'pool_layers_clips.0.bias', 'pool_layers_clips.1.bias', 'pool_layers_clips.2.bias')
KEYS = ('norm1.weight', 'norm1.bias') + POOL_W + POOL_B

# (grid (B, H0, W0), blocks, options)
CASES = [((1, 1, 1), 1, {}),
         ((1, 7, 7), 1, {'dres': False}),
         ((1, 7, 7), 2, {'stacked': False}),
         ((2, 6, 15), 1, {}),
         ((2, 6, 15), 1, {'accum': True, 'stacked': False}),
         ((2, 6, 15), 2, {}),
         ((2, 6, 15), 3, {'stacked': False}),
         ((2, 6, 15), 4, {}),
         ((2, 6, 15), 5, {}),
         ((2, 13, 16), 1, {'stacked': False}),
         ((2, 13, 16), 2, {})]
IDS = ['%dx%dx%d-n%d%s' % (g + (n, ''.join('-' + k + ('' if v else '0') for k, v in sorted(o.items())))) for g, n, o in CASES]


def P(t, offset=0):
    return C.c_void_p(t.data_ptr() + 4 * offset)


def reference(x_ref, x_tgt, params, dz, dres, pre, dtype, parts=1):
    """The restatement and autograd through it in `dtype`: {quantity: tensor}, and the forward rows of every block.
    parts > 1 (the fp32 evaluation): the backward runs in `parts` passes, pass j with the upstream gradient of the rows j mod parts and
    zeros elsewhere.  The stage is linear in its upstream gradient, so the passes add up to the same gradients, but torch's own
    reduction for a pooling weight -- one chain of up to 27 648 products when it runs on one thread -- becomes `parts` short ones:
    in one pass fp32 torch was 3.7e-6 .. 4.5e-6 from fp64 on one thread and 0.3e-6 on eight for the same well-conditioned quantity,
    which measures the thread count and not the quantity.  A cancelling quantity still shows: its passes cancel against each other."""
    b = x_ref.shape[0]
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    xr = leaf(x_ref)
    out, rows_all = {}, []
    for d, (xt, p) in enumerate(zip(x_tgt, params)):
        xt = leaf(xt)
        p = {k: leaf(v) for k, v in p.items()}
        rows = O.cffa_token_rows(torch.cat([xr, xt[:, None]], dim=1), p)
        up = dz[d].to(dtype)
        part = torch.arange(up.shape[0] * up.shape[1]).view(up.shape[0], -1, 1) % parts
        for j in range(parts):                     # (the stage is linear in its upstream gradient: the passes add up in .grad)
            rows.backward(up * (part == j) if parts > 1 else up, retain_graph=j + 1 < parts)
        rows_all.append(rows.detach())
        out['%d.dx_tgt' % d] = xt.grad.reshape(b, -1, 256) + (dres[d].to(dtype) if dres is not None else 0)
        for k in KEYS:
            out['%d.%s' % (d, k)] = p[k].grad
    out['dx_ref'] = xr.grad.reshape(b, 3, -1, 256) + (pre.to(dtype) if pre is not None else 0)
    return out, rows_all


def quantity_err(name, got, ref):
    if name.endswith('.bias') and 'pool_layers' in name:      # a scalar: plain relative error
        return abs(float(got.reshape(-1)[0]) - float(ref.reshape(-1)[0])) / abs(float(ref.reshape(-1)[0]))
    return H.rel_err(got.reshape(-1), ref.reshape(-1))


@functools.lru_cache(maxsize=None)
def case_data(grid, n, accum, dres):
    """Inputs of a case and both references (computed once, shared by the emulator and the GPU test)."""
    b, h0, w0 = grid
    hp, wp = O.padded_size(h0, w0)
    nw, hw = (hp // 7) * (wp // 7), h0 * w0
    gen = torch.Generator().manual_seed(4000 + 100 * h0 + 10 * w0 + n)
    rn = lambda *s: torch.randn(*s, generator=gen)
    st = R.layer_state(n, seed=21)
    params = [{k: v for k, v in O.split_block_params(st, d).items() if k in KEYS} for d in range(n)]
    x_ref = rn(b, 3, h0, w0, 256)
    x_tgt = [rn(b, h0, w0, 256) for _ in range(n)]
    # The upstream gradient: noise + a mean + the stage's own output (the gradient of <rows, noise + mean> + own |rows|^2 / 2).  The last
    # term is what keeps the parameter gradients from being cancelling sums: with noise alone a pooling-weight gradient is a random
    # walk over every cell and channel, and fp32 torch itself was 4.2e-6 from fp64 on one host (1.8e-6 on another) for the 9-element one.
    # (one pixel: a pooling weight's gradient has 256 terms and the window's weight on that pixel is ~1/49, so the output counts 8-fold)
    mean, own = (0.0, 8.0) if hw == 1 else (0.5, 1.0)
    with torch.no_grad():
        fwd = [O.cffa_token_rows(torch.cat([x_ref, xt[:, None]], dim=1).double(), {k: v.double() for k, v in p.items()}).float()
               for xt, p in zip(x_tgt, params)]
    dz = [rn(b, 64 * nw, 256) + mean + own * fwd[d] for d in range(n)]
    dr = [rn(b, hw, 256) for _ in range(n)] if dres else None
    pre = rn(b, 3, hw, 256) if accum else None
    ref64, rows = reference(x_ref, x_tgt, params, dz, dr, pre, torch.float64)
    ref32, _ = reference(x_ref, x_tgt, params, dz, dr, pre, torch.float32, parts=REF_PARTS)
    # target-token rows of padded pixels (window-major): z is the constant 0 there
    win = torch.from_numpy(O.window_pixels(hp, wp)).view(-1)
    padded = ((win // wp) >= h0) | ((win % wp) >= w0)
    return dict(params=params, x_ref=x_ref, x_tgt=x_tgt, dz=dz, dres=dr, pre=pre, ref64=ref64, ref32=ref32, rows=rows, padded=padded, nw=nw)


def run_case(lib, device, grid, n, accum=False, dres=True, stacked=True):
    b, h0, w0 = grid
    D = case_data(grid, n, accum, dres)
    g = ops.make_geom(lib, b, h0, w0)
    hw, rc, nw = g.HW, g.RC, g.nW
    assert (hw, rc, nw) == (h0 * w0, 64 * D['nw'], D['nw'])
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == 'cuda' else None
    dev = lambda t: t.to(device).contiguous()
    full = lambda shape, v: torch.full(shape, v, device=device)
    slots, nt = (4, 2) if stacked else (3, 1)       # frames per clip in the buffer of dx_ref / of a dx_tgt
    # ---- inputs: the frames as slots of a [B,4,HW,256] stack (what is not passed is NaN) or dense
    if stacked:
        stacks = [full((b, 4, hw, 256), NAN) for _ in range(n)]
        stacks[0][:, :3] = dev(D['x_ref'].reshape(b, 3, hw, 256))
        for d in range(n):
            stacks[d][:, 3] = dev(D['x_tgt'][d].reshape(b, hw, 256))
        x_ref, ref_bs = P(stacks[0]), 4 * hw * 256
        x_tgt, tgt_bs = [P(s, 3 * hw * 256) for s in stacks], 4 * hw * 256
    else:
        stacks = [dev(D['x_ref'].reshape(b, 3, hw, 256))] + [dev(t.reshape(b, hw, 256)) for t in D['x_tgt']]
        x_ref, ref_bs = P(stacks[0]), 3 * hw * 256
        x_tgt, tgt_bs = [P(s) for s in stacks[1:]], hw * 256
    prm = [{k: dev(v) for k, v in p.items()} for p in D['params']]
    # ---- forward through the library: M, zall (the anchor of the row order), mean / rstd
    Ms, means, rstds = [], [], []
    for d in range(n):
        pw = (C.c_void_p * 4)(*[prm[d][k].data_ptr() for k in POOL_W])
        pb = (C.c_void_p * 4)(*[prm[d][k].data_ptr() for k in POOL_B])
        M, zall, mean, rstd = full((15 * 49,), NAN), full((b, rc, 256), NAN), full((b * 4 * hw,), NAN), full((b * 4 * hw,), NAN)
        _lib.check(lib.cffm_pool_matrix(pw, P(M), stream), lib)
        _lib.check(lib.cffm_ln_pool_fwd(C.byref(g), x_ref, ref_bs, x_tgt[d], tgt_bs, P(prm[d]['norm1.weight']), P(prm[d]['norm1.bias']), P(M), pb,
                                        P(zall), P(mean), P(rstd), stream), lib)
        off = 0
        for cnt in (49 * nw, nw, nw, 4 * nw, 9 * nw):
            assert H.rel_err(zall[:, off:off + cnt], D['rows'][d][:, off:off + cnt]) < GATE, (d, off)
            off += cnt
        assert off == rc
        Ms.append(M); means.append(mean); rstds.append(rstd)
    dres_d = [dev(t) for t in D['dres']] if dres else [None] * n

    def call(dz, pads):
        """One cffm_ln_pool_bwd on fresh NaN-filled outputs -> every output buffer, on the CPU."""
        dz = [dev(t) for t in dz]
        out = {}
        dxr = full((b * slots * hw + GUARD, 256), NAN)
        dxr[b * slots * hw:] = SENTINEL
        if accum:
            dxr[:b * slots * hw].view(b, slots, hw, 256)[:, :3] = dev(D['pre'])
        out['dx_ref'] = dxr
        blocks = (_lib.CffaBwdBlock * n)()
        for d in range(n):
            dxt = full((b * nt * hw + GUARD, 256), NAN)       # stacked: the second slot of [B,2,HW,256]; dense: [B,HW,256]
            dxt[b * nt * hw:] = SENTINEL
            out['%d.dx_tgt' % d] = dxt
            for k in KEYS:
                numel = prm[d][k].numel()
                t = full((numel + 3,) if 'pool_layers' in k else (numel,), NAN)
                t[numel:] = SENTINEL
                out['%d.%s' % (d, k)] = t
            B = blocks[d]
            B.x_tgt, B.tgt_bs, B.gamma, B.beta = x_tgt[d], tgt_bs, P(prm[d]['norm1.weight']), P(prm[d]['norm1.bias'])
            B.M, B.mean, B.rstd, B.dzall, B.dres = P(Ms[d]), P(means[d]), P(rstds[d]), P(dz[d]), P(dres_d[d]) if dres else None
            B.dx_tgt, B.dtgt_bs = (P(dxt, hw * 256), 2 * hw * 256) if stacked else (P(dxt), hw * 256)
            B.dgamma, B.dbeta = P(out['%d.norm1.weight' % d]), P(out['%d.norm1.bias' % d])
            B.dpool_w = (C.c_void_p * 4)(*[out['%d.%s' % (d, k)].data_ptr() for k in POOL_W])
            B.dpool_b = (C.c_void_p * 4)(*[out['%d.%s' % (d, k)].data_ptr() for k in POOL_B])
        lib.cffm_grad_slices_padded(pads)
        try:
            _lib.check(lib.cffm_ln_pool_bwd(C.byref(g), n, blocks, x_ref, ref_bs, P(dxr), slots * hw * 256, 1 if accum else 0, stream), lib)
        finally:
            lib.cffm_grad_slices_padded(0)
        return {k: v.cpu() for k, v in out.items()}

    def split(out):
        """-> ({quantity: the written part}, {name: what must stay as it was})"""
        val, rest = {}, {}
        t = out['dx_ref'][:b * slots * hw].view(b, slots, hw, 256)
        val['dx_ref'], rest['dx_ref guard'] = t[:, :3], out['dx_ref'][b * slots * hw:]
        if stacked:
            rest['dx_ref slot 3'] = t[:, 3]
        for d in range(n):
            t = out['%d.dx_tgt' % d]
            val['%d.dx_tgt' % d] = t[:b * nt * hw].view(b, nt, hw, 256)[:, -1]
            rest['%d.dx_tgt guard' % d] = t[b * nt * hw:]
            if stacked:
                rest['%d.dx_tgt slot 0' % d] = t[:b * nt * hw].view(b, nt, hw, 256)[:, 0]
            for k in KEYS:
                numel = D['params'][d][k].numel()
                val['%d.%s' % (d, k)] = out['%d.%s' % (d, k)][:numel]
                if 'pool_layers' in k:
                    rest['%d.%s tail' % (d, k)] = out['%d.%s' % (d, k)][numel:]
        return val, rest

    bits = lambda t: t.contiguous().view(torch.int32)
    val, rest = split(call(D['dz'], 0))
    assert set(val) == set(D['ref64'])
    print('\n%s on %s, n = %d: error against fp64 of the kernels | of fp32 torch' % (grid, device.type, n))
    bad = []
    for name in sorted(val):
        assert torch.isfinite(val[name]).all(), name                       # every element written
        e_k, e_t = quantity_err(name, val[name], D['ref64'][name]), quantity_err(name, D['ref32'][name], D['ref64'][name])
        print('  %-36s %.2e | %.2e' % (name, e_k, e_t))
        assert e_t < REF_GATE, 'the reference itself is ill-conditioned: %s %.2e' % (name, e_t)
        if not e_k < GATE:
            bad.append((name, e_k))
    assert not bad, bad
    for name, t in rest.items():                                            # nothing else written
        if 'slot' in name:
            assert torch.isnan(t).all(), name
        else:
            assert bool((t == SENTINEL).all()), name
    # the padded form: same bits, zeros behind the pooling tensors
    val1, rest1 = split(call(D['dz'], 1))
    for name in val:
        assert torch.equal(bits(val[name]), bits(val1[name])), name
    for name, t in rest1.items():
        if name.endswith('tail') and POOL_W[3] not in name:      # (4 floats: no padding behind it, the sentinel stays)
            assert bool((t == 0).all()) and not bool(torch.signbit(t).any()), name
        else:
            assert torch.equal(bits(t), bits(rest[name])), name
    # the gradient rows of padded target pixels are not part of the function; a repeated call gives the same bits
    dz2 = [t.clone() for t in D['dz']]
    for t in dz2:
        t[:, :49 * nw][:, D['padded']] = torch.randn(b, int(D['padded'].sum()), 256, generator=torch.Generator().manual_seed(5)) * 100
    val2, _ = split(call(dz2, 0))
    for name in val:
        assert torch.equal(bits(val[name]), bits(val2[name])), name


def run_errors(lib):
    g = ops.make_geom(lib, 1, 7, 7)
    one = (_lib.CffaBwdBlock * 1)()
    buf = torch.zeros(16)
    for n, blocks, x_ref, dx_ref in ((1, None, P(buf), P(buf)), (1, one, None, P(buf)), (1, one, P(buf), None), (0, one, P(buf), P(buf)),
                                     (9, one, P(buf), P(buf)), (1, one, P(buf), P(buf))):       # (the last: null fields of the block)
        assert lib.cffm_ln_pool_bwd(C.byref(g), n, blocks, x_ref, 0, dx_ref, 0, 0, None) != 0
        assert b'ln_pool_bwd' in lib.cffm_last_error()
    assert lib.cffm_ln_pool_bwd(None, 1, one, P(buf), 0, P(buf), 0, 0, None) != 0


@pytest.mark.parametrize('grid,n,opts', CASES, ids=IDS)
def test_cffa_bwd_stage_emulated(grid, n, opts):
    run_case(emu.lib(), torch.device('cpu'), grid, n, **opts)


def test_cffa_bwd_bad_arguments_are_reported():
    run_errors(emu.lib())


@pytest.mark.gpu
@pytest.mark.parametrize('grid,n,opts', CASES, ids=IDS)
def test_cffa_bwd_stage_gpu(grid, n, opts):
    run_case(_lib.get(), torch.device('cuda:0'), grid, n, **opts)
