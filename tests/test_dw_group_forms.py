"""The grouped weight-gradient kernel (k_gemm_group_tt) in every operand storage form, through the stage entry
cffm_linear_bwd_weight_group_forms, against fp64 products of the operands the kernel is handed, at tests/test_linear.py's gate for the
grouped entry (2e-5 relative to the result's norm: split-bf16 operands, fp32 accumulation).

The forms with a body of their own are (dy, x) = (fp32, split-4), (split-4, split-4), (fp32, fp32); the contraction lengths walk the edges
of the K-loop's pipeline (prologue, whole-tile fast loop, tail loop), at one K-tile in flight as built and at two (GROUP_PF = 2).  With the
workgroup target low enough that a k-slice holds the whole contraction: 32 rows (one K-tile: prologue only), 64 and 96 (two and three tiles:
the first fast iterations, or the tail loop only at two tiles in flight), 160 (five tiles: fast iterations, then the tail at either depth),
145 (ragged last tile: the slow path from the start); with the default target the minimal 128-row slices (four K-tiles, 145 rows: a second,
ragged slice).  1216 rows of 128x128 and 256x128 outputs in 480-row slices: many fast iterations, partial slabs and the summation launch.  The
fourth problem of a group is (split-4, fp32), which runs the run-time body, as does the on-load GELU (x_pre = 2), once on its own.

Guards: every operand is followed by rows of NaN past M, and the same launch runs first on all-NaN operands, which leaves NaN in every
partial slab of the library's scratch.  Every case runs twice: the results must be bit-equal.  CPU: emulator build; GPU: product library."""
import ctypes as C
import functools

import pytest
import torch

from tests import emu
from vss_cffm_amd import _lib

TOL = 2e-5
GUARD = 40          # NaN rows behind every operand: more than one 32-row K-tile

FORMS4 = [(0, 1), (1, 1), (0, 0), (1, 0)]
SQ4 = [(128, 128)] * 4
# (name, rows M, [(N, K)], [(dy_pre, x_pre)], target_wgs)
CASES = [
    ('m32', 32, SQ4, FORMS4, 0),
    ('m64', 64, SQ4, FORMS4, 4),
    ('m96', 96, SQ4, FORMS4, 4),
    ('m160', 160, SQ4, FORMS4, 4),
    ('m145_one_slice', 145, SQ4, FORMS4, 4),
    ('m145_two_slices', 145, SQ4, FORMS4, 0),
    ('m1216_slabs', 1216, [(128, 128), (256, 128), (128, 128), (256, 128)], FORMS4, 16),
    ('gelu_m160', 160, [(128, 128)], [(0, 2)], 1),
    ('gelu_m1216_slabs', 1216, [(256, 128)], [(0, 2)], 8),
]


class WGrad(C.Structure):
    _fields_ = [('dy', C.c_void_p), ('x', C.c_void_p), ('dw', C.c_void_p), ('M', C.c_long), ('N', C.c_int), ('K', C.c_int)]


class WForm(C.Structure):
    _fields_ = [('dy_pre', C.c_int), ('x_pre', C.c_int), ('x_bias', C.c_void_p)]


def split4_store(x):
    """fp32 [R, C] -> (split-4 storage of it as an fp32 tensor [R, C], the fp64 values that storage represents)"""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    R, Cc = x.shape
    packed = torch.cat([hi.view(R, Cc // 4, 4), lo.view(R, Cc // 4, 4)], dim=2).contiguous()
    return packed.view(torch.float32).reshape(R, Cc), hi.double() + lo.double()


def guarded(x):
    return torch.cat([x, torch.full((GUARD, x.shape[1]), float('nan'))], dim=0)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """host operands (with guard rows, in their storage form), the bias or None, and the fp64 result, per problem"""
    _, M, shapes, forms, _ = next(c for c in CASES if c[0] == name)
    gen = torch.Generator().manual_seed(11 + sum(map(ord, name)))
    out = []
    for (N, K), (dy_pre, x_pre) in zip(shapes, forms):
        dy, x = torch.randn(M, N, generator=gen), torch.randn(M, K, generator=gen)
        bias = None
        dy_val, x_val = dy.double(), x.double()
        dy_st, x_st = guarded(dy), guarded(x)
        if dy_pre == 1:
            dy_st, v = split4_store(guarded(dy))
            dy_val = v[:M]
        if x_pre == 1:
            x_st, v = split4_store(guarded(x))
            x_val = v[:M]
        elif x_pre == 2:
            bias = 0.5 * torch.randn(K, generator=gen)
            x_val = torch.nn.functional.gelu(x.double() + bias.double())
        out.append((dy_st, x_st, bias, dy_val.T @ x_val))
    return out


def run_case(lib, device, name):
    _, M, shapes, forms, target = next(c for c in CASES if c[0] == name)
    data = case_data(name)
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if device.type == 'cuda' else None
    n = len(shapes)
    prob, form, dws, nan_dws, keep = (WGrad * n)(), (WForm * n)(), [], [], []   # keep: the operands' device tensors stay alive
    nanp = (WGrad * n)()
    for i, ((N, K), (dy_pre, x_pre), (dy_st, x_st, bias, _)) in enumerate(zip(shapes, forms, data)):
        dyd, xd, dw = dy_st.to(device), x_st.to(device), torch.full((N, K), 7., device=device)
        # 0x7fc07fc0: NaN as fp32 and as both bf16 halves, whichever form the operand is read in
        dyn, xn = (torch.full(t.shape, 0x7fc07fc0, dtype=torch.int32, device=device).view(torch.float32) for t in (dyd, xd))
        dwn = torch.empty_like(dw)
        bd = bias.to(device) if bias is not None else None
        dws.append(dw)
        nan_dws.append(dwn)
        keep.append((dyd, xd, dyn, xn, bd))
        prob[i] = WGrad(dyd.data_ptr(), xd.data_ptr(), dw.data_ptr(), M, N, K)
        nanp[i] = WGrad(dyn.data_ptr(), xn.data_ptr(), dwn.data_ptr(), M, N, K)
        form[i] = WForm(dy_pre, x_pre, bd.data_ptr() if bd is not None else None)
    runs = []
    for _ in range(2):
        assert lib.cffm_linear_bwd_weight_group_forms(nanp, form, n, target, stream) == 0      # NaN into every partial slab
        for i in range(n):
            assert bool(torch.isnan(nan_dws[i]).all()), (name, i)
            dws[i].fill_(7.)
        assert lib.cffm_linear_bwd_weight_group_forms(prob, form, n, target, stream) == 0
        runs.append([dw.cpu() for dw in dws])
    errs = [float((runs[0][i].double() - data[i][3]).norm() / data[i][3].norm()) for i in range(n)]
    print('%s (M %d, target %d): rel err per problem %s' % (name, M, target, ' '.join('%.2e' % e for e in errs)))
    for i in range(n):
        assert errs[i] < TOL, (name, i, errs[i])
        assert torch.equal(runs[0][i].view(torch.int32), runs[1][i].view(torch.int32)), (name, i)
    return runs[0]


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_dw_group_forms_emulated(name):
    with emu.active():
        run_case(emu.lib(), torch.device('cpu'), name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_dw_group_forms_gpu(name):
    run_case(_lib.get(), torch.device('cuda:0'), name)


def test_dw_group_forms_rejects():
    """the on-load GELU exists in the grouped kernel only: a shape it cannot tile is an error, and so is an unknown form"""
    with emu.active():
        lib = emu.lib()
        dy, x, dw, b = torch.randn(70, 96), torch.randn(70, 40), torch.zeros(96, 40), torch.zeros(40)
        prob, form = (WGrad * 1)(), (WForm * 1)()
        prob[0] = WGrad(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), 70, 96, 40)
        form[0] = WForm(0, 2, b.data_ptr())
        assert lib.cffm_linear_bwd_weight_group_forms(prob, form, 1, 0, None) != 0
        form[0] = WForm(0, 3, None)
        assert lib.cffm_linear_bwd_weight_group_forms(prob, form, 1, 0, None) != 0
        form[0] = WForm(0, 0, None)
        assert lib.cffm_linear_bwd_weight_group_forms(prob, form, 1, 0, None) == 0
        assert float((dw.double() - dy.double().T @ x.double()).norm() / (dy.double().T @ x.double()).norm()) < TOL
