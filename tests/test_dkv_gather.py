"""The dK / dV gather on its own (cffm_dkv_gather, csrc/cfm_attn_kernels.h k_dkv_gather) against a NumPy float32 restatement of its
summation order, bit for bit: per element the readers of a row in inv_idx order, whole batches of four as
((x0 s0 + x1 s1) + (x2 s2 + x3 s3)) added to the sum one batch after the other, then the remaining one to three singly.

Inputs as the attention backward leaves them: f16 partial rows, one power-of-two scale per (window, head) with differing exponents --
every product x s is then exact in float32, so whether the compiler contracts a product into the following addition cannot change a
bit, only the order of the additions can.  Every slot that key_src marks absent holds NaN (never read), dqkv starts as a sentinel."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import emu
from vss_cffm_amd import _lib, geometry, ops

SENTINEL = np.float32(-12345.678)

# the reader counts that exist: (1,7,7) one window, <= 4 readers; (2,13,30) ragged, two clips (the clip stride of the partial rows, the
# scales and dqkv); (1,28,28) counts 6, 9, 12, 16; (1,35,35) 15, 20, 25 (remainders 3, 0, 1); (1,49,49) 28 ... 49 with 49 = 12 x 4 + 1,
# 42 = 10 x 4 + 2, 35 = 8 x 4 + 3: the longest chain, crossing an 8- or 16-deep request boundary three times
GRIDS = [(1, 7, 7), (2, 13, 30), (1, 28, 28), (1, 35, 35), (1, 49, 49)]
EXPECTED_COUNTS = {(1, 28, 28): {6, 9, 12, 16}, (1, 35, 35): {15, 20, 25}, (1, 49, 49): {28, 35, 42, 49}}


def P(t):
    return C.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def case(b, h0, w0):
    """-> (workspace float32 [b nW (304*256 + 8)], expected k|v float32 [b, RC, 512], nW): computed once, shared, never modified"""
    rng = np.random.default_rng(b * 1000 + h0 * 31 + w0)
    key_src, _ = geometry.tables(h0, w0)
    inv_ptr, inv_idx = geometry.inverse_tables(h0, w0)
    nw = key_src.shape[0]
    rc = 64 * nw
    counts = set(np.diff(inv_ptr).tolist())
    assert EXPECTED_COUNTS.get((b, h0, w0), set()) <= counts, counts
    part = (rng.standard_normal((b, nw * 304, 512)) * np.exp2(rng.integers(-6, 5, (b, nw * 304, 1)))).astype(np.float16)
    part[:, key_src.reshape(-1) < 0] = np.float16('nan')
    scale = np.exp2(rng.integers(-20, 5, (b, nw, 8))).astype(np.float32)
    ws = np.concatenate([part.reshape(-1).view(np.float32), scale.reshape(-1)])
    assert ws.size == b * nw * (304 * 256 + 8)
    # the partial rows in units of their scale: exact float32 products
    col_head = np.arange(512) // 64
    expect = np.zeros((b, rc, 512), dtype=np.float32)
    n_of_row = np.diff(inv_ptr)
    for n in sorted(counts):
        rows = np.nonzero(n_of_row == n)[0]
        if n == 0 or rows.size == 0:
            continue
        idx = inv_idx[inv_ptr[rows][:, None] + np.arange(n)[None, :]]                       # [rows, n]
        v = part[:, idx].astype(np.float32) * scale[:, idx // 304][..., col_head]           # [b, rows, n, 512]
        assert np.isfinite(v).all()
        acc = np.zeros((b, rows.size, 512), dtype=np.float32)
        e = 0
        while e + 3 < n:
            acc = acc + ((v[:, :, e] + v[:, :, e + 1]) + (v[:, :, e + 2] + v[:, :, e + 3]))
            e += 4
        while e < n:
            acc = acc + v[:, :, e]
            e += 1
        expect[:, rows] = acc
    # partial-row columns (head, K 32 | V 32) -> dqkv columns 256 + (K | V) 256 + head 32 + channel
    c = np.arange(512)
    out_col = 256 * ((c // 32) & 1) + 32 * (c // 64) + c % 32
    kv = np.empty_like(expect)
    kv[:, :, out_col] = expect
    ws.setflags(write=False)
    kv.setflags(write=False)
    return ws, kv, nw


def run(lib, device, b, h0, w0):
    ws, kv, nw = case(b, h0, w0)
    rc = 64 * nw
    g = ops.make_geom(lib, b, h0, w0)
    _, _, ip_t, ii_t = ops.device_tables(h0, w0, device)
    ws_t = torch.from_numpy(np.array(ws)).to(device)
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == 'cuda' else None
    outs = []
    for _ in range(2):
        dqkv = torch.full((b * rc, 768), float(SENTINEL), device=device)
        _lib.check(lib.cffm_dkv_gather(C.byref(g), P(ip_t), P(ii_t), P(ws_t), P(dqkv), stream), lib)
        outs.append(dqkv.cpu().numpy().reshape(b, rc, 768))
    got, again = outs
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))                      # the same bits twice
    assert np.array_equal(got[:, :, 256:].view(np.uint32), kv.view(np.uint32))              # every k|v element, exactly
    assert (got[:, 49 * nw:, :256].view(np.uint32) == 0).all()                              # pooled rows: q third zeroed (+0.0)
    assert (got[:, :49 * nw, :256] == SENTINEL).all()                                       # target rows: q third untouched


@pytest.mark.parametrize('grid', GRIDS)
def test_dkv_gather_emulated(grid):
    run(emu.lib(), torch.device('cpu'), *grid)


@pytest.mark.gpu
@pytest.mark.parametrize('grid', GRIDS)
def test_dkv_gather_gpu(grid):
    run(_lib.get(), torch.device('cuda'), *grid)
