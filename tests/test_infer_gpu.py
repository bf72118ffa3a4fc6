"""The inference forward of BasicLayer3d3 on a real MI355X (the emulator half is tests/test_infer.py): bit-exact against the training
forward at the evaluation shapes, against the reference's golden and the oracle, through the three heads, captured into a HIP
graph, and its peak memory against the training forward's."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest
import torch

from oracle import cffm_oracle as O, recipe as R, ref_import as RI
from tests import helpers as H
from tests import test_infer as T
from vss_cffm_amd import _lib, ops
from vss_cffm_amd.registry import build_head

pytestmark = pytest.mark.gpu
FWD_TOL = T.FWD_TOL
HEAD_TOL = 1e-3       # tests/test_boundary.py: the north-star contract on logits


def dev():
    return torch.device('cuda:0')


def seeded(b, h, w, depth, seed):
    st = R.layer_state(depth, seed=seed)
    x = R.synth_input('x', (b, 4, 256, h, w), seed=seed + 1)
    return st, x


def bit_exact(st, x, depth):
    """inference == training forward (torch.equal), rows and whole output; returns the whole output"""
    b, _, _, h, w = x.shape
    params = T.flat_params(st, depth, dev())
    xd = x.to(dev())
    xr = T.to_rows(xd)
    with torch.no_grad():
        y_train = ops.cffm_layer(xd, depth, params)
        yr_train = ops.cffm_layer_rows(xr, h, w, depth, params)
    prepared = ops.layer_prepare(depth, params)
    y = ops.cffm_layer_infer(xd, depth, params, prepared)
    yr = ops.cffm_layer_rows_infer(xr, h, w, depth, params, prepared)
    torch.cuda.synchronize()
    assert torch.equal(yr, yr_train)
    assert torch.equal(y, y_train)
    assert torch.equal(yr, T.to_rows(y)[:, 3])
    return y


@pytest.mark.parametrize('case', T.SMALL_CASES + ['seeded_8x8_d4', 'seeded_33x34_d1'])
def test_small_cases_bit_exact_and_poisoned(case):
    T.run_poisoned(case, dev())


def test_60x60_b1_bit_exact_and_reference_golden():
    g = H.load_golden('layer_b1_60x60_d2')
    b, h, w, depth, st, x, _ = H.layer_case_inputs(g)
    assert (b, h, w, depth) == (1, 60, 60, 2)
    y = bit_exact(st, x, depth)
    H.check_layer_forward(g, y[:, -1], FWD_TOL)
    T.run_poisoned('layer_b1_60x60_d2', dev())


def test_60x60_b2_bit_exact():
    st, x = seeded(2, 60, 60, 2, seed=40)
    bit_exact(st, x, 2)


def test_60x108_depth2_bit_exact_and_oracle():
    """the reference's evaluation shape (480 x 864 frames -> a 60 x 108 grid, one clip), as tests/test_gpu_parity.py::
    test_nonsquare_vspw_test_shape_forward checks the training forward"""
    depth, b, h, w = 2, 1, 60, 108
    st = R.layer_state(depth, seed=8)
    x = R.synth_input('x', (b, 4, 256, h, w), seed=9)
    y = bit_exact(st, x, depth)
    yo = O.layer_forward(x, st, depth)
    e = H.rel_err(y[:, -1].cpu(), yo[:, -1])
    print('60x108 depth 2: forward rel err %.3e' % e)
    assert e < FWD_TOL


def test_60x108_depth4_bit_exact():
    st, x = seeded(1, 60, 108, 4, seed=44)
    bit_exact(st, x, 4)


def test_cache_validity_gpu():
    T.run_cache_validity(dev())


def test_dispatch_gpu():
    T.run_dispatch(dev())


# ---------------------------------------------------------------------------------------------- heads
class CallSpy:
    """counts calls of library entry points through the binding"""

    def __init__(self, lib, *names):
        self.lib, self.real, self.n = lib, {k: getattr(lib, k) for k in names}, {k: 0 for k in names}

    def __enter__(self):
        for k, fn in self.real.items():
            def counted(*a, _k=k, _fn=fn):
                self.n[_k] += 1
                return _fn(*a)
            setattr(self.lib, k, counted)
        return self

    def __exit__(self, *exc):
        for k, fn in self.real.items():
            setattr(self.lib, k, fn)


def my_head(kind, seed, **cfg):
    m = build_head(RI.head_cfg(kind=kind, **cfg))
    assert not m.load_state_dict(R.synth_state(m, seed=seed), strict=False).unexpected_keys
    for d in (m.dropout, getattr(m, 'dropout3', None)):
        if d is not None:
            d.p = 0.0
    return m.to(dev()).eval()


def stats(t):
    t = torch.as_tensor(t).detach().cpu().double()
    return np.array([float(t.sum()), float(t.abs().sum()), float(t.square().sum()), float(t.abs().max())])


def test_heads_eval_no_grad_reproduce_the_head_goldens():
    """head.eval() + torch.no_grad() reaches the inference path through decoder_focal and reproduces the eval logits of the goldens
    tests/test_boundary.py checks (same fixtures, same 1e-3): the base head and the CFFM++ head at the B0 64 x 64 and the B1 480 x 480
    shapes.  The prototype-generating head never calls decoder_focal (cffm_head.py:161-300 returns the last frame's logits and
    writes k-means centres) and the goldens hold no logits of it: it is run for completeness only."""
    from tests.golden.make_golden_head import feature_maps
    from tests.golden import make_golden_head_b1 as G
    lib = _lib.get()
    g0 = H.load_golden('head_b0_64')
    feats = [f.to(dev()) for f in feature_maps(1, 4, 64)]
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad(), \
            CallSpy(lib, 'cffm_layer_infer_rows', 'cffm_layer_infer_full', 'cffm_layer_prepare', 'cffm_layer_saved_floats') as spy:
        infer_calls = lambda: spy.n['cffm_layer_infer_rows'] + spy.n['cffm_layer_infer_full']
        os.makedirs(os.path.join(tmp, 'vid0'))
        metas = [{'filename': tmp + '/data/vid0/origin/0001.jpg'}]
        # ---- B0, 64 x 64
        head = my_head('CFFMHead_clips_resize1_8', 30)
        assert H.rel_err(head(feats, 1, 4).cpu(), g0['eval_logits']) < HEAD_TOL
        assert H.rel_err(head.forward_test(feats, None, None, 1, 4).cpu(), g0['eval_logits']) < HEAD_TOL
        assert infer_calls() == 2 and spy.n['cffm_layer_prepare'] == 1 and spy.n['cffm_layer_saved_floats'] == 0
        pp = my_head('CFFMHead_clips_resize1_8_finetune_w_prototype3', 34)
        torch.save(R.synth_input('centers', (1, 8, 256), seed=35, scale=1.0), os.path.join(tmp, 'vid0', 'centers.pt'))
        pp.save_path = tmp + '/'
        assert H.rel_err(pp(feats, 1, 4, None, metas).cpu(), g0['pp_eval_logits']) < HEAD_TOL
        assert infer_calls() == 3 and spy.n['cffm_layer_saved_floats'] == 0
        gene = my_head('CFFMHead_clips_resize1_8_gene_prototype', 30)
        gene.save_path = tmp + '/gene/'
        gene.n_clusters = 8
        out = gene(feats, 1, 4, None, metas)
        assert out.shape == (1, 124, 16, 16) and torch.isfinite(out).all()
        assert os.path.isfile(tmp + '/gene/vid0/centers.pt')
        # ---- B1, 480 x 480 (depth 2)
        g1 = H.load_golden('head_b1_480')
        m = my_head('CFFMHead_clips_resize1_8', 70, in_channels=G.B1, depths=2)
        f1 = [f.to(dev()) for f in feature_maps(1, 4, G.SIZE, chans=G.B1, seed=71)]
        y = m(f1, 1, 4)
        assert H.rel_err(y[..., ::G.STRIDE, ::G.STRIDE].cpu(), g1['eval_logits_s4']) < HEAD_TOL
        np.testing.assert_allclose(stats(y)[1:3], g1['eval_logits_stats'][1:3], rtol=HEAD_TOL)
        gp = H.load_golden('headpp_b1_480_k8')
        pp1 = my_head('CFFMHead_clips_resize1_8_finetune_w_prototype3', 90, in_channels=G.B1, depths=2)
        f2 = [f.to(dev()) for f in feature_maps(1, 4, G.SIZE, chans=G.B1, seed=91)]
        torch.save(R.synth_input('centers', (1, 8, 256), seed=92, scale=1.0), os.path.join(tmp, 'vid0', 'centers.pt'))
        pp1.save_path = tmp + '/'
        y = pp1(f2, 1, 4, None, metas)
        assert H.rel_err(y[..., ::G.STRIDE, ::G.STRIDE].cpu(), gp['eval_logits_s4']) < HEAD_TOL
        np.testing.assert_allclose(stats(y)[1:3], gp['eval_logits_stats'][1:3], rtol=HEAD_TOL)
        assert infer_calls() == 5 and spy.n['cffm_layer_saved_floats'] == 0


# ---------------------------------------------------------------------------------------------- HIP graph, memory
@pytest.mark.parametrize('shape', [(1, 60, 108, 2), (2, 60, 60, 2)])
def test_captured_call_replays_bit_for_bit(shape):
    """one inference call captured with torch.cuda.graph (everything is on the caller's stream: a single chain) and replayed
    equals the eager call; a replay after the input changed equals the eager call on the new input"""
    b, h, w, depth = shape
    lib = _lib.get()
    st, x = seeded(b, h, w, depth, seed=50)
    params = T.flat_params(st, depth, dev())
    prepared = ops.layer_prepare(depth, params)
    xr = T.to_rows(x.to(dev()))
    eager = ops.cffm_layer_rows_infer(xr, h, w, depth, params, prepared)
    ws = torch.empty(lib.cffm_layer_infer_ws_floats(C.byref(ops.make_geom(lib, b, h, w))), dtype=torch.float32, device=dev())
    out = torch.full_like(eager, float('nan'))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.cffm_layer_rows_infer(xr, h, w, depth, params, prepared, ws=ws, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    xr.mul_(0.5)
    ws.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.cffm_layer_rows_infer(xr, h, w, depth, params, prepared))
    assert not torch.equal(out, eager)


def test_peak_memory_drops_by_three_block_workspaces():
    """60 x 108, depth 4: the rise of max_memory_allocated over one no_grad forward of the layer is below the rise over one forward
    with grad enabled by at least 3 x cffm_block_ws.total x 4 bytes (three of the four per-block workspaces no longer exist;
    from the layout, not measured)."""
    depth, b, h, w = 4, 1, 60, 108
    lib = _lib.get()
    st, x = seeded(b, h, w, depth, seed=44)
    m = T.build_layer(depth, st, dev())
    xd = x.to(dev())
    blk = ops.block_ws_layout(lib, ops.make_geom(lib, b, h, w)).total

    def rise(grad):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        with torch.set_grad_enabled(grad):
            y = m(xd)
        torch.cuda.synchronize()
        assert (y.grad_fn is not None) == grad
        r = torch.cuda.max_memory_allocated() - base
        del y
        return r

    m.eval()
    rise(False)                  # (the prepared parameter data and the geometry tables are built here, once: not part of a call)
    r_inf, r_train = rise(False), rise(True)
    need = 3 * blk * 4
    print('peak rise: no_grad %.1f MB, grad %.1f MB, difference %.1f MB, required >= %.1f MB' % (r_inf / 2**20, r_train / 2**20,
                                                                                                  (r_train - r_inf) / 2**20, need / 2**20))
    assert r_train - r_inf >= need
