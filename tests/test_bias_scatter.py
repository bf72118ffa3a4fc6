"""The adjoint of the position-bias assembly as a stage of the C ABI (cffm_bias_scatter; csrc/rowops_kernels.h k_bias_scatter gathers
dbiasT [8 heads][304 keys][64 queries], as the attention backward leaves it, into the gradients of the six tables) against fp64
autograd of oracle.cffm_oracle.assemble_bias.  dbiasT holds random integers in [-8, 8] EVERYWHERE, the query columns 49..63 and key
rows 289..303 included, which must not reach any table; every table entry is then a sum of at most 49 small integers, exact in fp32
in any order, so the comparison is torch.equal.  The tables start as NaN: every entry must be written.
CPU: emulator build; GPU: product library."""
import ctypes as C

import pytest
import torch

from oracle import cffm_oracle as O, recipe as R
from tests import emu
from vss_cffm_amd import _lib

OWN, RING = 'attn.relative_position_bias_table', 'attn.relative_position_bias_table_to_neighbors'
POOL = ('attn.relative_position_bias_table_to_windows.0', 'attn.relative_position_bias_table_to_windows_clips.0',
        'attn.relative_position_bias_table_to_windows_clips.1', 'attn.relative_position_bias_table_to_windows_clips.2')


def P(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(scope='module')
def problem():
    dbiasT = torch.randint(-8, 9, (8, 304, 64), generator=torch.Generator().manual_seed(31)).float()
    shapes = R.block_param_shapes()
    p = {k: torch.zeros(shapes[k], dtype=torch.float64, requires_grad=True) for k in (OWN, RING) + POOL}
    O.assemble_bias(p).backward(dbiasT.double().transpose(1, 2)[:, :49, :289])
    return dbiasT, {k: v.grad for k, v in p.items()}


def run_scatter(lib, device, problem):
    dbiasT, ref = problem
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == 'cuda' else None
    got = {k: torch.full(v.shape, float('nan'), device=device) for k, v in ref.items()}
    pool = (C.c_void_p * 4)(*[got[k].data_ptr() for k in POOL])
    _lib.check(lib.cffm_bias_scatter(P(dbiasT.to(device)), P(got[OWN]), P(got[RING]), pool, stream), lib)
    for k, v in ref.items():
        assert k == RING or bool(v.abs().max() > 8), k         # (the shared tables sum many entries; the ring table is one to one)
        assert torch.equal(got[k].cpu().double(), v), k


def test_bias_scatter_emulated(problem):
    run_scatter(emu.lib(), torch.device('cpu'), problem)


def test_bias_scatter_bad_arguments_are_reported():
    lib = emu.lib()
    t = torch.zeros(8)
    pool = (C.c_void_p * 4)(P(t), P(t), None, P(t))
    for args in ((None, P(t), P(t), pool), (P(t), None, P(t), pool), (P(t), P(t), None, pool), (P(t), P(t), P(t), None),
                 (P(t), P(t), P(t), pool)):                    # (the last: a null table inside the array)
        assert lib.cffm_bias_scatter(*args, None) != 0
        assert b'bias_scatter' in lib.cffm_last_error()


@pytest.mark.gpu
def test_bias_scatter_gpu(problem):
    run_scatter(_lib.get(), torch.device('cuda:0'), problem)
