"""The block's q|k|v input gradient as a stage of the C ABI (cffm_panel_qkv_bwd_input; csrc/panel_kernels.h k_panel_gemm<MT, 2, false, 0>
with K = 768, the launch of the block backward with its column-sum records and the optional T-frag copy of dqkv) against fp64:
    dx = dqkv w,   db = the column sums of dqkv (qkv.bias.grad, after the block backward's record reduction)
from fp32 dqkv and w in fragment order (input-gradient form), under the gate of tests/test_panel.py for the same split-bf16 operand
format (norm-relative error < 2e-5).  Row counts: 1, 17, 33, 200 (the last 16-row tile is partly out of range), 520 (more than 16
panels) -- all of them 32-row panels -- and 8200, where the host picks 48-row panels (8193 .. 12288 rows) and the last panel is ragged
against 48, 32 and 16 rows (8200 mod 48 = 40); on the emulator that size takes one call, without the
variants below.  dqkv is followed by 64 rows of NaN: nothing past
row M may be read (the buffer bounds of the kernel make such reads zero), so a NaN in dx or db means the bounds are wrong.  Also:
sentinel rows behind dx survive, the T-frag copy equals cffm_tfrag_pack of the same rows bit for bit with zeros past M, dx has the
same bits with and without db / dqkv_t, and two calls give the same bits.  CPU: emulator build; GPU: product library."""
import ctypes as C

import pytest
import torch

from tests import emu
from vss_cffm_amd import _lib

TOL = 2e-5                # tests/test_panel.py: split-bf16 operands (hi + lo, ~2^-17 per product)

SIZES = (1, 17, 33, 200, 520)
SIZE_48 = 8200            # 48-row panels
NAN_ROWS = 64
SENTINEL = -7.0


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def rel(a, b):
    b = b.double()
    return float((a.double().cpu() - b.cpu()).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope='module')
def problem():
    gen = torch.Generator().manual_seed(29)
    dqkv = torch.randn(SIZE_48, 768, generator=gen)
    w = torch.randn(768, 256, generator=gen) * 0.08
    return dqkv, w, dqkv.double() @ w.double()


def run_stage(lib, device, problem, m, variants=True):
    dqkv, w, ref = problem
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == 'cuda' else None
    dq = torch.full((m + NAN_ROWS, 768), float('nan'), device=device)
    dq[:m] = dqkv[:m].to(device)
    wf = torch.empty(768 * 256, device=device)
    _lib.check(lib.cffm_panel_pack_weight(P(w.to(device)), 768, 256, 1, P(wf), stream), lib)
    nt = lib.cffm_tfrag_floats(m, 768)

    def call(with_db, with_t):
        dx = torch.full((m + NAN_ROWS, 256), SENTINEL, device=device)
        db = torch.full((768,), float('nan'), device=device) if with_db else None
        dq_t = torch.full((nt,), SENTINEL, device=device) if with_t else None
        _lib.check(lib.cffm_panel_qkv_bwd_input(P(dq), P(wf), P(dx), P(db), P(dq_t), m, stream), lib)
        return dx.cpu(), db.cpu() if with_db else None, dq_t.cpu() if with_t else None

    dx, db, dq_t = call(True, True)
    assert torch.isfinite(dx).all() and torch.isfinite(db).all()             # nothing past row M of dqkv was read
    e_dx, e_db = rel(dx[:m], ref[:m]), rel(db, dqkv[:m].double().sum(0))
    print('M = %d: dx %.3e, db %.3e' % (m, e_dx, e_db))
    assert e_dx < TOL and e_db < TOL
    assert bool((dx[m:] == SENTINEL).all())                                  # rows past M are untouched
    want = torch.full((nt,), SENTINEL, device=device)
    _lib.check(lib.cffm_tfrag_pack(P(dq[:m]), P(want), m, 768, stream), lib)
    assert torch.equal(dq_t.view(torch.int32), want.cpu().view(torch.int32))
    m32 = (m + 31) // 32 * 32
    rows = dq_t.view(torch.int16).reshape(m32 // 32, 768 // 16, 2, 4, 16, 8).permute(2, 0, 3, 5, 1, 4).reshape(2, m32, 768)   # tests/test_panel_qkv.py
    assert not bool(rows[:, m:].any())                                       # rows past M are zero
    hi = dqkv[:m].bfloat16()
    assert torch.equal(rows[0, :m], hi.view(torch.int16)) and torch.equal(rows[1, :m], (dqkv[:m] - hi.float()).bfloat16().view(torch.int16))
    if not variants:
        return
    bits = lambda t: t.view(torch.int32)
    for with_db, with_t in ((True, True), (False, False), (True, False), (False, True)):     # (the first: a repeated call)
        dx2, db2, dq_t2 = call(with_db, with_t)
        assert torch.equal(bits(dx), bits(dx2)), (with_db, with_t)
        assert not with_db or torch.equal(bits(db), bits(db2))
        assert not with_t or torch.equal(bits(dq_t), bits(dq_t2))


def run_errors(lib):
    t = torch.zeros(768)
    for args in ((None, P(t), P(t), None, None, 1), (P(t), None, P(t), None, None, 1), (P(t), P(t), None, None, None, 1),
                 (P(t), P(t), P(t), None, None, 0), (P(t), P(t), P(t), None, None, 1 << 21)):
        assert lib.cffm_panel_qkv_bwd_input(*args, None) != 0
        assert b'panel_qkv_bwd_input' in lib.cffm_last_error()


@pytest.mark.parametrize('m', SIZES)
def test_panel_qkv_bwd_stage_emulated(problem, m):
    run_stage(emu.lib(), torch.device('cpu'), problem, m)


def test_panel_qkv_bwd_48_row_panels_emulated(problem):
    run_stage(emu.lib(), torch.device('cpu'), problem, SIZE_48, variants=False)      # (one call: seconds on the emulator)


def test_panel_qkv_bwd_bad_arguments_are_reported():
    run_errors(emu.lib())


@pytest.mark.gpu
@pytest.mark.parametrize('m', SIZES + (SIZE_48,))
def test_panel_qkv_bwd_stage_gpu(problem, m):
    run_stage(_lib.get(), torch.device('cuda:0'), problem, m)
