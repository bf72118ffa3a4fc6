"""The inference forward of BasicLayer3d3 (include/cffm_hip.h ABI 12: cffm_layer_prepare / cffm_layer_infer_rows / _infer_full) on the
CPU through the fiber emulator: bit-exact against the training forward, against the reference's goldens, workspace size and
poisoning, validity of the module's prepared-parameter cache, dispatch.  The GPU half is tests/test_infer_gpu.py."""
import ctypes as C

import pytest
import torch

import vss_cffm_amd as V
from oracle import recipe as R
from tests import emu, helpers as H
from vss_cffm_amd import _lib, ops

FWD_TOL = 5e-4      # the forward gate of the parity tests (tests/test_gpu_parity.py)
SMALL_CASES = [c for c in H.LAYER_CASES if '60x60' not in c]     # 8x8 d1, 8x8 B=2 d2, 14x21 d2, 13x30 d1 (the 60x60 one is for the GPU)


def flat_params(st, depth, device='cpu'):
    return [st['blocks.%d.%s' % (i, k)].clone().to(device) for i in range(depth) for k, _, _ in ops.BLOCK_PARAM_KEYS]


def to_rows(x):
    """[B,4,256,H,W] -> token rows [B,4,H*W,256]"""
    b, t, c, h, w = x.shape
    return x.permute(0, 1, 3, 4, 2).reshape(b, t, h * w, c).contiguous()


def case_inputs(case):
    """(b, h, w, depth, state, x, golden or None); 'seeded_*': no golden, seeded parameters (depth 4 on the 8x8 grid; 33x34 depth 1)"""
    if case == 'seeded_8x8_d4':
        return 1, 8, 8, 4, R.layer_state(4, seed=61), R.synth_input('x', (1, 4, 256, 8, 8), seed=62), None
    if case == 'seeded_33x34_d1':          # 1122 rows: the 16-row panels of the inference Mlp kernel (over 1024 rows), ragged last panel
        return 1, 33, 34, 1, R.layer_state(1, seed=63), R.synth_input('x', (1, 4, 256, 33, 34), seed=64), None
    g = H.load_golden(case)
    b, h, w, depth, st, x, _ = H.layer_case_inputs(g)
    return b, h, w, depth, st, x, g


def build_layer(depth, st, device='cpu'):
    m = V.BasicLayer3d3(dim=256, depth=depth, num_heads=8, window_size=7, expand_size=3, pool_method='fc', focal_level=2,
                        focal_window=5, focal_l_clips=[1, 2, 3], focal_kernel_clips=[7, 5, 3])
    m.load_state_dict(st, strict=False)
    return m.to(device)


def run_bit_exact(case, device):
    """Same parameters and input: the inference forward equals the training forward with torch.equal (same arithmetic in the same
    order), on rows and on the reference's whole output.  Returns what the golden checks need."""
    b, h, w, depth, st, x, g = case_inputs(case)
    params = flat_params(st, depth, device)
    x = x.to(device)
    xr = to_rows(x)
    with torch.no_grad():
        y_train = ops.cffm_layer(x, depth, params)
        yr_train = ops.cffm_layer_rows(xr, h, w, depth, params)
    prepared = ops.layer_prepare(depth, params)
    y = ops.cffm_layer_infer(x, depth, params, prepared)
    yr = ops.cffm_layer_rows_infer(xr, h, w, depth, params, prepared)
    assert y.grad_fn is None and yr.grad_fn is None
    assert torch.equal(yr, yr_train)
    assert torch.equal(y, y_train)
    assert torch.equal(y[:, :3], x[:, :3])
    return g, y, yr, (b, h, w, depth, params, prepared, x, xr)


@pytest.mark.parametrize('case', SMALL_CASES + ['seeded_8x8_d4'])
def test_infer_equals_training_forward_bit_for_bit(case):
    with emu.active():
        run_bit_exact(case, torch.device('cpu'))


@pytest.mark.parametrize('case', SMALL_CASES)
def test_infer_against_reference_golden(case):
    with emu.active():
        g, y, yr, (b, h, w, *_rest) = run_bit_exact(case, torch.device('cpu'))
    H.check_layer_forward(g, y[:, -1], FWD_TOL)
    H.check_layer_forward(g, yr.reshape(b, h, w, 256).permute(0, 3, 1, 2), FWD_TOL)


def test_workspace_is_independent_of_depth_and_small():
    """cffm_layer_infer_ws_floats takes no depth; at (B = 1, 60 x 60) it is at most half of ONE block's training workspace (from
    the layout: zall 1.33 M + f16 q|k|v 1.99 M + ao 0.92 M + 2 x x2 0.92 M = 6.08 M of 19.0 M floats)."""
    lib = emu.lib()
    assert _lib.SIGNATURES['cffm_layer_infer_ws_floats'][1] == [_lib.GP]
    g = ops.make_geom(lib, 1, 60, 60)
    ws = lib.cffm_layer_infer_ws_floats(C.byref(g))
    blk = ops.block_ws_layout(lib, g).total
    print('inference workspace %d floats, block workspace %d floats, ratio %.3f' % (ws, blk, ws / blk))
    assert 0 < ws <= blk // 2
    assert ws == 5184 * 256 + 5184 * 768 // 2 + 3 * 3600 * 256
    # the prepared data does not depend on the geometry and grows linearly with depth
    assert lib.cffm_layer_prepared_floats(4) == 4 * lib.cffm_layer_prepared_floats(1) > 0
    assert lib.cffm_layer_prepared_floats(0) < 0


def run_poisoned(case, device):
    """Workspace and output filled with NaN before the call: the output is finite and equals the unpoisoned one (every element the
    kernels read has been written by the same call; 13 x 30 = 390 rows ends in ragged panels)."""
    g, y, yr, (b, h, w, depth, params, prepared, x, xr) = run_bit_exact(case, device)
    lib = _lib.get()
    n = lib.cffm_layer_infer_ws_floats(C.byref(ops.make_geom(lib, b, h, w)))
    nan = float('nan')
    ws = torch.full((n,), nan, dtype=torch.float32, device=device)
    out = torch.full((b, h * w, 256), nan, dtype=torch.float32, device=device)
    got = ops.cffm_layer_rows_infer(xr, h, w, depth, params, prepared, ws=ws, out=out)
    assert got is out and torch.isfinite(out).all() and torch.equal(out, yr)
    ws.fill_(nan)
    out = torch.full((b, 4, 256, h, w), nan, dtype=torch.float32, device=device)
    got = ops.cffm_layer_infer(x, depth, params, prepared, ws=ws, out=out)
    assert got is out and torch.isfinite(out).all() and torch.equal(out, y)


@pytest.mark.parametrize('case', SMALL_CASES + ['seeded_8x8_d4', 'seeded_33x34_d1'])
def test_poisoned_workspace_and_output(case):
    with emu.active():
        run_poisoned(case, torch.device('cpu'))


def test_argument_checks():
    with emu.active() as lib:
        g, y, yr, (b, h, w, depth, params, prepared, x, xr) = run_bit_exact('layer_b1_8x8_d1', torch.device('cpu'))
        geom = ops.make_geom(lib, b, h, w)
        ks, qd = ops.device_tables(h, w, x.device)[:2]
        ps = ops.block_structs(params, depth)
        P = lambda t: C.c_void_p(t.data_ptr())
        ws = torch.empty(lib.cffm_layer_infer_ws_floats(C.byref(geom)))
        assert lib.cffm_layer_infer_rows(C.byref(geom), depth, ps, None, P(xr), P(yr), P(ks), P(qd), P(ws), None) < 0
        assert b'bad arguments' in lib.cffm_last_error()
        assert lib.cffm_layer_infer_rows(C.byref(geom), 0, ps, P(prepared), P(xr), P(yr), P(ks), P(qd), P(ws), None) < 0
        assert lib.cffm_layer_infer_full(C.byref(geom), depth, ps, P(prepared), P(x), P(x), P(ks), P(qd), P(ws), None) < 0
        assert b'alias' in lib.cffm_last_error()
        assert lib.cffm_layer_prepare(depth, ps, None, None) < 0
        with pytest.raises(_lib.CffmError):
            ops.cffm_layer_rows_infer(xr, h, w, depth, params, prepared, ws=torch.empty(16))
        with pytest.raises(_lib.CffmError):
            ops.cffm_layer_rows_infer(xr, h, w, depth, params, prepared[:100])
        with pytest.raises(IndexError):
            ops.cffm_layer_infer(x[:, :3], depth, params, prepared)


# ---------------------------------------------------------------------------------------------- module: cache and dispatch
class PrepareCounter:
    """counts cffm_layer_prepare calls through the binding"""

    def __init__(self, lib):
        self.lib, self.real, self.n = lib, lib.cffm_layer_prepare, 0

    def __enter__(self):
        def counted(*a):
            self.n += 1
            return self.real(*a)
        self.lib.cffm_layer_prepare = counted
        return self

    def __exit__(self, *exc):
        self.lib.cffm_layer_prepare = self.real


def fresh_forward(m, x):
    """the module's eval forward with a cache built from scratch"""
    m.drop_prepared()
    with torch.no_grad():
        return m(x)


def run_cache_validity(device):
    lib = _lib.get()
    depth = 2
    st = R.layer_state(depth, seed=0)
    x = R.synth_input('x', (1, 4, 256, 8, 8), seed=1).to(device)
    m = build_layer(depth, st, device).eval()
    w = m.blocks[1].mlp.fc2.weight
    with PrepareCounter(lib) as cnt:
        with torch.no_grad():
            y0 = m(x)
            assert cnt.n == 1
            y0b = m(x)                         # unchanged weights: the prepared data is reused
            y0r = m.forward_rows(to_rows(x), 8, 8)
        assert cnt.n == 1 and torch.equal(y0, y0b)
        assert torch.equal(y0r, to_rows(y0)[:, 3])
        # ---- an in-place update through the parameter, as torch's optimisers do it: seen through _version, no mode call needed
        with torch.no_grad():
            w.add_(0.05 * torch.ones_like(w))
            y1 = m(x)
        assert cnt.n == 2
        assert not torch.equal(y1, y0)
        assert torch.equal(y1, fresh_forward(m, x))
        # ---- p.data.add_: `p.data` has a version counter of its own, p._version does not move -- the eval() call drops the cache
        with torch.no_grad():
            y1 = m(x)
        v = w._version
        w.data.add_(0.05 * torch.ones_like(w))
        assert w._version == v
        m.eval()
        with torch.no_grad():
            y1b = m(x)
        assert not torch.equal(y1b, y1)
        assert torch.equal(y1b, fresh_forward(m, x))
        # ---- one step of the library's AdamW (updates through raw pointers, bumps no _version) through train() / eval()
        n_before = cnt.n
        with torch.no_grad():
            y1 = m(x)                          # (the cache fresh_forward rebuilt is valid for the current weights)
        assert cnt.n == n_before
        m.train()
        opt = V.optim.AdamW(m.parameters(), lr=1e-2, weight_decay=0.0)
        gen = torch.Generator().manual_seed(3)
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=gen).to(device)
        versions = [p._version for p in m.parameters()]
        opt.step()
        if device.type == 'cuda':
            torch.cuda.synchronize()
        m.eval()
        with torch.no_grad():
            y2 = m(x)
        assert not torch.equal(y2, y1)
        assert torch.equal(y2, fresh_forward(m, x))
        # (documented reason for dropping the cache in train(True): this optimiser does not bump the versions)
        print('AdamW bumped parameter versions:', versions != [p._version for p in m.parameters()])
        # ---- load_state_dict, on the module itself and on a module above it
        with torch.no_grad():
            y2 = m(x)
        m.load_state_dict(st, strict=False)
        with torch.no_grad():
            y3 = m(x)
        assert not torch.equal(y3, y2) and torch.equal(y3, y0)
        assert torch.equal(y3, fresh_forward(m, x))
        outer = torch.nn.ModuleDict({'layer': m})
        st2 = {'layer.' + k: v for k, v in R.layer_state(depth, seed=5).items()}
        with torch.no_grad():
            y3 = m(x)
        n = cnt.n
        outer.load_state_dict(st2, strict=False)
        with torch.no_grad():
            y4 = m(x)
        assert cnt.n == n + 1 and not torch.equal(y4, y3)
        assert torch.equal(y4, fresh_forward(m, x))


def test_cache_validity_emulated():
    with emu.active():
        run_cache_validity(torch.device('cpu'))


def run_dispatch(device):
    """Grad enabled and a parameter requiring grad: the module still calls what it called before (a grad_fn, the same output and
    gradients as ops._LayerFullFn.apply); under no_grad, or with nothing requiring grad, no grad_fn and no saved activations."""
    lib = _lib.get()
    depth = 2
    st = R.layer_state(depth, seed=0)
    x = R.synth_input('x', (1, 4, 256, 8, 8), seed=1).to(device)
    gy = R.synth_input('g', (1, 4, 256, 8, 8), seed=2, scale=1.0).to(device)
    m = build_layer(depth, st, device)
    params = [p for blk in m.blocks for p in blk.param_list()]
    xa = x.clone().requires_grad_(True)
    y = m(xa)
    assert y.grad_fn is not None
    y.backward(gy)
    got = [xa.grad.clone()] + [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    xb = x.clone().requires_grad_(True)
    yb = ops._LayerFullFn.apply(xb, depth, *params)
    yb.backward(gy)
    assert torch.equal(y, yb)
    for a, b in zip(got, [xb.grad] + [p.grad for p in params]):
        assert torch.equal(a, b)
    yr = m.forward_rows(to_rows(x), 8, 8)
    assert yr.grad_fn is not None and torch.equal(yr, to_rows(y.detach())[:, 3])
    # ---- nothing to record: the inference path, which never asks for the training workspace
    real = lib.cffm_layer_saved_floats
    calls = []

    def spy(*a):
        calls.append(a)
        return real(*a)
    lib.cffm_layer_saved_floats = spy
    try:
        with torch.no_grad():
            yn = m(x)
            ynr = m.forward_rows(to_rows(x), 8, 8)
        assert not calls
        for p in params:
            p.requires_grad_(False)
        yf = m(x)                              # grad mode on, but neither the input nor a parameter requires grad
        assert not calls
        yg = m(x.clone().requires_grad_(True))  # frozen parameters, input requires grad: recorded again
        assert len(calls) == 1 and yg.grad_fn is not None
    finally:
        lib.cffm_layer_saved_floats = real
    assert yn.grad_fn is None and ynr.grad_fn is None and yf.grad_fn is None
    assert torch.equal(yn, y.detach()) and torch.equal(yf, yn) and torch.equal(ynr, yr.detach())


def test_dispatch_emulated():
    with emu.active():
        run_dispatch(torch.device('cpu'))
