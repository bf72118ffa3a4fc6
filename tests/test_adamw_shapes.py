"""cffm_adamw_step_rows through the C ABI: the one-launch form (tickets: the step count advanced inside the update launch, a workgroup
walking several entries of the chunk table) against the two-launch form (no tickets: tick kernel, then one workgroup per entry),
bit for bit over two consecutive steps, at the table shapes where the one-launch kernel takes another path:

* tensors of 1, 2047, 2048, 2049 and 3 x 2048 + 5 elements (short, whole and trailing chunks; odd numbers of entries per tensor, so
  a workgroup's entries come from different tensors and different rows);
* one tensor that starts 4 bytes off 16-byte alignment (its whole chunk takes the element-wise path);
* three rows with differing constants, one of them inactive (no entry names it: its step count must stay);
* a table of fewer than 64 entries and one of more than 64 (the two ticket levels);
* gradients addressed through `grad_base` + byte offsets and directly (grad_base NULL)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import emu
from vss_cffm_amd import _lib

CHUNK = 2048
NCONST = 12
SIZES = [1, 2047, 2048, 2049, 3 * 2048 + 5]
MISALIGNED = 2048 + 3            # starts one float behind a 16-byte boundary
BIG = 66 * 2048 + 7              # 67 entries: with the others more than 64


def P(t):
    return C.c_void_p(t.data_ptr())


def layout(big):
    """-> [(float offset into the flat buffers, elements, row)], total floats; rows 0 and 1 alternate, row 2 owns nothing"""
    sizes = SIZES + [MISALIGNED] + ([BIG] if big else [])
    items, off = [], 0
    for i, n in enumerate(sizes):
        off = (off + 3) // 4 * 4 + (1 if n == MISALIGNED else 0)
        items.append((off, n, i % 2))
        off += n
    return items, off + 4


def run_form(lib, device, big, use_base, tickets, steps=2):
    items, total = layout(big)
    gen = torch.Generator().manual_seed(77 + big)
    flat = lambda scale: (torch.randn(total, generator=gen) * scale).to(device)
    p, m, v = flat(1.0), flat(1e-2), flat(1e-4).abs()
    assert p.data_ptr() % 16 == 0 and m.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0
    grads = [flat(1e-1) for _ in range(steps)]
    g = torch.empty(total, device=device)
    rows = []
    for off, n, row in items:
        o = np.arange(0, n, CHUNK, dtype=np.int64)
        r = np.empty((o.size, 5), dtype=np.int64)
        r[:, 0] = p.data_ptr() + 4 * (off + o)
        r[:, 1] = (0 if use_base else g.data_ptr()) + 4 * (off + o)
        r[:, 2] = m.data_ptr() + 4 * (off + o)
        r[:, 3] = v.data_ptr() + 4 * (off + o)
        r[:, 4] = np.minimum(CHUNK, n - o) | (np.int64(row) << 32)
        rows.append(r)
    tab = torch.from_numpy(np.concatenate(rows)).to(device)
    assert (tab.shape[0] > 64) == big
    consts = torch.zeros(3, NCONST, dtype=torch.float64)
    consts[:, 0] = torch.tensor([0.9, 0.8, 0.95])
    consts[:, 1] = torch.tensor([0.999, 0.99, 0.98])
    consts[:, 2] = torch.tensor([1e-8, 1e-6, 1e-7])
    consts[0, 3:10] = torch.tensor([1.0, 50.0, 1.0, 0.0, 8.0, 1e-3, 0.0])     # row 0: poly decay with warm-up, evaluated on the device
    consts[:, 10] = 5.0
    consts = consts.to(device)
    state = torch.zeros(3, 4)
    state[:, 0] = torch.tensor([5.0, 2.0, 7.0])
    state[2, 1:] = torch.tensor([0.25, 0.5, 0.75])                            # the inactive row's factors: must survive
    state = state.to(device)
    sched = torch.tensor([[2e-3, 0.05], [1e-3, 0.0], [3e-3, 0.01]]).to(device)
    active = torch.tensor([1, 1, 0], dtype=torch.int32).to(device)
    ticket = torch.zeros(65, dtype=torch.int32, device=device)
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == 'cuda' else None
    snaps = []
    for s in range(steps):
        g.copy_(grads[s])
        _lib.check(lib.cffm_adamw_step_rows(P(tab), tab.shape[0], P(g) if use_base else None, P(state), P(sched), P(consts), 3, P(active),
                                            P(ticket) if tickets else None, stream), lib)
        assert int(ticket.abs().sum()) == 0                                    # the tickets are back at zero
        st, cs = state.cpu(), consts.cpu()
        assert st[:, 0].tolist() == [6.0 + s, 3.0 + s, 7.0]                    # active rows advanced, the inactive one kept
        assert st[2, 1:].tolist() == [0.25, 0.5, 0.75]
        assert cs[:, 10].tolist() == [6.0 + s] * 3                             # the global iteration: every row
        snaps.append([t.cpu().clone() for t in (p, m, v, state, consts)])
    return snaps


def compare(lib, device, big, use_base):
    one, two = run_form(lib, device, big, use_base, True), run_form(lib, device, big, use_base, False)
    for a, b in zip(one, two):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    items, total = layout(big)
    # every element of every tensor was updated (the first moment moves whenever g != m), nothing between the tensors was
    gen = torch.Generator().manual_seed(77 + big)
    torch.randn(total, generator=gen)
    m0, m2 = torch.randn(total, generator=gen) * 1e-2, one[-1][1]
    for off, n, _ in items:
        assert bool((m2[off:off + n] != m0[off:off + n]).all())
    for (off, n, _), (nxt, _, _) in zip(items, items[1:]):
        assert torch.equal(m2[off + n:nxt], m0[off + n:nxt])


CASES = [(False, True), (False, False), (True, True), (True, False)]


@pytest.mark.parametrize('big,use_base', CASES)
def test_adamw_table_shapes_emulated(big, use_base):
    compare(emu.lib(), torch.device('cpu'), big, use_base)


@pytest.mark.gpu
@pytest.mark.parametrize('big,use_base', CASES)
def test_adamw_table_shapes_gpu(big, use_base):
    compare(_lib.get(), torch.device('cuda'), big, use_base)
