"""The block's q|k|v Linear as a stage of the C ABI (cffm_panel_qkv_fwd; csrc/panel_kernels.h k_panel_qkv3: one workgroup per
(row panel, q / k / v column third), panels dealt so that the three thirds of a panel share an XCD) against fp64:
    qkv16 = f16((x W^T + b) * [32^-0.5 on the first 256 columns])
from x in split-4 storage and W in fragment order, under the gate tests/test_emu_kernels.py uses for this quantity (rel_err < 1e-3:
f16 storage).  Row counts: 64 (the second panel is ragged at 48 rows), 144 (whole panels), 200 (the last 16-row tile is partly out of
range), 512 (more than 8 panels: the XCD mapping and its tail guard) -- all of them 32-row panels, which is what the host picks for a
grid of one round -- and 5512, where it picks 48-row panels (5441 .. 8160 rows: two rounds of 32-row panels against one of 48) and the
last panel ends inside a 32-row k-step of the T-frag copy (5512 mod 96 = 40; on the emulator that size runs once, in the T-frag test,
which checks the output as well).  Also: rows past M are not written, the optional T-frag copy of x equals cffm_tfrag_pack of the same
rows bit for bit with zeros past M, and two calls give identical bytes.  CPU: emulator build; GPU: product library."""
import ctypes as C

import pytest
import torch

from tests import emu, helpers as H
from vss_cffm_amd import _lib

SIZES = (64, 144, 200, 512, 5512)
SIZES_T = (64, 200, 5512)
SENTINEL = -7.0


def P(t):
    return C.c_void_p(t.data_ptr())


def split4(x):
    """fp32 [M][256] -> split-4 storage: per 4 consecutive floats 16 bytes = 4 bf16 hi = bf16(x), then 4 bf16 lo = bf16(x - hi)."""
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    m = x.shape[0]
    both = torch.cat([hi.view(torch.int16).reshape(m, -1, 4), lo.view(torch.int16).reshape(m, -1, 4)], dim=2)
    return both.reshape(m, -1).contiguous().view(torch.float32), hi, lo


def tfrag_rows(t, m, c=256):
    """T-frag storage (include/cffm_hip.h, ABI 9) -> (hi, lo) as int16 [R32][c]: unit (ks, jt, h), lane l15 + 16 g, element e holds
    x[32 ks + 8 g + e][16 jt + l15]."""
    r32 = (m + 31) // 32 * 32
    u = t.cpu().view(torch.int16).reshape(r32 // 32, c // 16, 2, 4, 16, 8)       # ks, jt, h, g, l15, e
    rows = u.permute(2, 0, 3, 5, 1, 4).reshape(2, r32, c)                         # h, (ks, g, e), (jt, l15)
    return rows[0], rows[1]


@pytest.fixture(scope='module')
def problem():
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(max(SIZES), 256, generator=gen)
    w = torch.randn(768, 256, generator=gen) * 0.08
    b = torch.randn(768, generator=gen) * 0.1
    ref = x.double() @ w.double().T + b.double()
    ref[:, :256] *= 32 ** -0.5
    return x, w, b, ref.half()


def run_stage(lib, device, problem, m, with_t):
    x, w, b, ref = problem
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == 'cuda' else None
    xs, hi, lo = split4(x[:m])
    xs, wd, bd = xs.to(device), w.to(device), b.to(device)
    wf = torch.empty(768 * 256, device=device)
    _lib.check(lib.cffm_panel_pack_weight(P(wd), 768, 256, 0, P(wf), stream), lib)
    x_t = torch.full((lib.cffm_tfrag_floats(m, 256),), SENTINEL, device=device) if with_t else None
    outs = []
    for _ in range(2):
        qkv = torch.full((m + 64, 768), SENTINEL, dtype=torch.float16, device=device)
        _lib.check(lib.cffm_panel_qkv_fwd(P(xs), P(wf), P(bd), P(qkv), m, P(x_t) if with_t else None, stream), lib)
        outs.append(qkv.cpu())
    err = H.rel_err(outs[0][:m].float(), ref[:m].float())
    print('M = %d: rel_err %.3e' % (m, err))
    assert err < 1e-3                                                        # f16 storage
    assert bool((outs[0][m:] == SENTINEL).all())                             # rows past M are untouched
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))   # repeats are bit-identical
    if with_t:
        want = torch.full_like(x_t, SENTINEL)
        _lib.check(lib.cffm_tfrag_pack(P(x[:m].contiguous().to(device)), P(want), m, 256, stream), lib)
        assert torch.equal(x_t.cpu().view(torch.int32), want.cpu().view(torch.int32))
        th, tl = tfrag_rows(x_t, m)
        assert torch.equal(th[:m], hi.view(torch.int16)) and torch.equal(tl[:m], lo.view(torch.int16))
        assert not bool(th[m:].any()) and not bool(tl[m:].any())             # rows past M are zero


def run_errors(lib):
    assert lib.cffm_panel_qkv_fwd(None, None, None, None, 64, None, None) != 0
    assert b'panel_qkv_fwd' in lib.cffm_last_error()


@pytest.mark.parametrize('m', SIZES[:4])
def test_panel_qkv_stage_emulated(problem, m):
    run_stage(emu.lib(), torch.device('cpu'), problem, m, with_t=False)


@pytest.mark.parametrize('m', SIZES_T)
def test_panel_qkv_tfrag_copy_emulated(problem, m):
    run_stage(emu.lib(), torch.device('cpu'), problem, m, with_t=True)


def test_panel_qkv_bad_arguments_are_reported():
    run_errors(emu.lib())


@pytest.mark.gpu
@pytest.mark.parametrize('m', SIZES)
def test_panel_qkv_stage_gpu(problem, m):
    run_stage(_lib.get(), torch.device('cuda:0'), problem, m, with_t=False)


@pytest.mark.gpu
@pytest.mark.parametrize('m', SIZES_T)
def test_panel_qkv_tfrag_copy_gpu(problem, m):
    run_stage(_lib.get(), torch.device('cuda:0'), problem, m, with_t=True)
