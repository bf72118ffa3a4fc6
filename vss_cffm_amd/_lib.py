"""ctypes binding of libcffm_hip.so (C ABI: include/cffm_hip.h).

The product path loads ONLY ``libcffm_hip.so`` (built by ``__graft_entry__.build()`` with hipcc for
gfx950) and raises if it is missing -- there is no CPU fallback.  ``bind(path)`` is the generic
signature binder; the test-suite uses it to load the emulator build of the same sources
(tests/emu.py) and ``_override`` is the single seam through which it does so.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libcffm_hip.so')
ABI_VERSION = 13

vp, ci, cl, cd, cf = C.c_void_p, C.c_int, C.c_long, C.c_double, C.c_float


class Geom(C.Structure):
    _fields_ = [(n, ci) for n in ('B', 'H0', 'W0', 'Hp', 'Wp', 'gy', 'gx', 'nW', 'HW', 'RC')]


class BlockPtrs(C.Structure):
    """cffm_block_params / cffm_block_grads (same field order)."""
    _fields_ = [('norm1_w', vp), ('norm1_b', vp), ('pool_w', vp * 4), ('pool_b', vp * 4), ('rpb_own', vp),
                ('rpb_ring', vp), ('rpb_pool', vp * 4), ('qkv_w', vp), ('qkv_b', vp), ('proj_w', vp), ('proj_b', vp),
                ('norm2_w', vp), ('norm2_b', vp), ('fc1_w', vp), ('fc1_b', vp), ('fc2_w', vp), ('fc2_b', vp)]


class BlockWs(C.Structure):
    _fields_ = [(n, cl) for n in ('mean1', 'rstd1', 'M', 'zall', 'qkv', 'bias', 'biasT', 'lse', 'ao', 'x1', 'mean2',
                                  'rstd2', 'z2', 'hraw', 'act', 'x2', 'w_split', 'w_frag', 'ao_t', 'zall_t', 'total')]


class CffaBwdBlock(C.Structure):
    """cffm_cffa_bwd_block"""
    _fields_ = ([('x_tgt', vp), ('tgt_bs', cl)] + [(n, vp) for n in ('gamma', 'beta', 'M', 'mean', 'rstd', 'dzall', 'dres')]
                + [('dx_tgt', vp), ('dtgt_bs', cl), ('dgamma', vp), ('dbeta', vp), ('dpool_w', vp * 4), ('dpool_b', vp * 4)])


class RecordSet(C.Structure):
    """cffm_record_set"""
    _fields_ = [('rec', vp), ('count', ci), ('stride', ci), ('total', ci), ('nseg', ci), ('off', ci * 8), ('width', ci * 8),
                ('accumulate', ci * 8), ('out', vp * 8)]


class PoolGrads(C.Structure):
    """cffm_pool_grads"""
    _fields_ = [('dM', vp), ('dpool_w', vp * 4), ('dpool_b', vp * 4)]


class TailTranspose(C.Structure):
    """cffm_tail_transpose"""
    _fields_ = [('src', vp), ('dst', vp), ('batch', ci), ('rows', ci), ('cols', ci), ('src_bs', cl), ('dst_bs', cl), ('addend', vp),
                ('add_mod', ci), ('add_skip', ci)]


class GtcPtrs(C.Structure):
    """cffm_gtc_params / cffm_gtc_grads (same field order)."""
    _fields_ = [(n, vp) for n in ('norm1_w', 'norm1_b', 'qkv_w', 'qkv_b', 'kv_w', 'kv_b', 'proj_w', 'proj_b', 'norm2_w', 'norm2_b',
                                  'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b')]


class MitBlockPtrs(C.Structure):
    """cffm_mit_block_params / cffm_mit_block_grad_ptrs (same field order)"""
    _fields_ = [(n, vp) for n in ('n1_g', 'n1_b', 'q_w', 'q_b', 'kv_w', 'kv_b', 'sr_w', 'sr_b', 'srn_g', 'srn_b', 'proj_w', 'proj_b',
                                  'n2_g', 'n2_b', 'fc1_w', 'fc1_b', 'dw_w', 'dw_b', 'fc2_w', 'fc2_b')]


class MitBlockScales(C.Structure):
    """cffm_mit_block_scales"""
    _fields_ = [('scale_attn', vp), ('scale_mlp', vp)]


class MitStageCfg(C.Structure):
    """cffm_mit_stage_cfg"""
    _fields_ = ([(n, ci) for n in ('B', 'H', 'W', 'C', 'heads', 'hidden', 'sr_ratio', 'depth')]
                + [(n, cf) for n in ('scale', 'eps_embed', 'eps_block', 'eps_sr', 'eps_out')])


class MitStage(C.Structure):
    """cffm_mit_stage"""
    _fields_ = ([('cfg', MitStageCfg)] + [(n, ci) for n in ('Cin', 'Hin', 'Win', 'k', 'stride')]
                + [(n, vp) for n in ('conv_w', 'conv_b', 'embed_g', 'embed_b', 'out_g', 'out_b')] + [('blocks', C.POINTER(MitBlockPtrs))])


GP, BP = C.POINTER(Geom), C.POINTER(BlockPtrs)
MBP, MCP = C.POINTER(MitBlockPtrs), C.POINTER(MitStageCfg)
MSP = C.POINTER(MitStage)
MSC = C.POINTER(MitBlockScales)
GTP = C.POINTER(GtcPtrs)
CBP = C.POINTER(CffaBwdBlock)
P4 = vp * 4

SIGNATURES = {
    'cffm_abi_version': (ci, []),
    'cffm_last_error': (C.c_char_p, []),
    'cffm_geom_init': (ci, [GP, ci, ci, ci]),
    'cffm_block_ws_layout': (ci, [GP, C.POINTER(BlockWs)]),
    'cffm_layer_saved_floats': (cl, [GP, ci]),
    'cffm_layer_scratch_floats': (cl, [GP]),
    'cffm_profile_enable': (ci, [C.c_longlong]),
    'cffm_profile_sample_every': (ci, [ci]),
    'cffm_side_streams': (ci, [ci]),
    'cffm_branch_begin': (vp, [vp, ci]),
    'cffm_branch_join': (ci, [vp]),
    'cffm_branch_mark': (ci, [vp]),
    'cffm_defer_begin': (vp, [vp]),
    'cffm_defer_join': (ci, [vp]),
    'cffm_add_inplace': (ci, [vp, vp, cl, vp]),
    'cffm_branch_take': (vp, [vp, ci]),
    'cffm_fuse_compose_fwd': (ci, [vp, vp, vp, vp, ci, ci, vp, vp, vp]),
    'cffm_fuse_compose_bwd': (ci, [vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp]),
    'cffm_profile_stage_count': (ci, []),
    'cffm_profile_null_pair': (ci, [vp]),
    'cffm_profile_stage_name': (C.c_char_p, [ci]),
    'cffm_profile_collect': (ci, [vp, vp]),
    'cffm_profile_collect_graph': (ci, [vp, vp, ci]),
    'cffm_transpose': (ci, [vp, vp, ci, ci, ci, cl, cl, vp]),
    'cffm_pool_matrix': (ci, [P4, vp, vp]),
    'cffm_grad_slices_padded': (None, [ci]),
    'cffm_ln_pool_fwd': (ci, [GP, vp, cl, vp, cl, vp, vp, vp, P4, vp, vp, vp, vp]),
    'cffm_bias_assemble': (ci, [vp, vp, P4, vp, vp, vp]),
    'cffm_linear_qkv_fwd': (ci, [vp, vp, vp, vp, cl, vp]),
    'cffm_attn_fwd': (ci, [GP, vp, vp, vp, vp, vp, vp, vp]),
    'cffm_attn_bwd': (ci, [GP, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    'cffm_dkv_gather': (ci, [GP, vp, vp, vp, vp, vp]),
    'cffm_linear_fwd': (ci, [vp, vp, vp, cl, ci, ci, vp]),
    'cffm_linear_bias_fwd': (ci, [vp, vp, vp, vp, cl, ci, ci, vp]),
    'cffm_linear_bwd_input': (ci, [vp, vp, vp, cl, ci, ci, vp]),
    'cffm_linear_bwd_weight': (ci, [vp, vp, vp, cl, ci, ci, vp]),
    'cffm_linear_bwd_weight_group': (ci, [vp, ci, vp]),
    'cffm_linear_bwd_weight_group_forms': (ci, [vp, vp, ci, ci, vp]),
    'cffm_tfrag_floats': (cl, [cl, ci]),
    'cffm_dw_stream': (ci, [ci]),
    'cffm_tfrag_pack': (ci, [vp, vp, cl, ci, vp]),
    'cffm_linear_bwd_weight_tfrag': (ci, [vp, vp, vp, cl, ci, ci, vp]),
    'cffm_linear_bwd_weight_tfrag_group': (ci, [vp, ci, vp]),
    'cffm_colsum': (ci, [vp, cl, ci, vp, vp]),
    'cffm_panel_pack_weight': (ci, [vp, ci, ci, ci, vp, vp]),
    'cffm_panel_qkv_fwd': (ci, [vp, vp, vp, vp, cl, vp, vp]),
    'cffm_ln_pool_bwd': (ci, [GP, ci, CBP, vp, cl, vp, cl, ci, vp]),
    'cffm_reduce_records': (ci, [ci, C.POINTER(RecordSet), vp]),
    'cffm_pool_matrix_bwd': (ci, [ci, C.POINTER(PoolGrads), vp]),
    'cffm_bwd_tail': (ci, [ci, C.POINTER(RecordSet), C.POINTER(TailTranspose), vp]),
    'cffm_panel_qkv_bwd_input': (ci, [vp, vp, vp, vp, vp, cl, vp]),
    'cffm_bias_scatter': (ci, [vp, vp, vp, C.POINTER(vp), vp]),
    'cffm_mlp_fwd': (ci, [vp, vp, cl, ci] + [vp] * 15 + [cl, vp]),
    'cffm_mlp_bwd': (ci, [vp] * 18 + [cl, vp]),
    'cffm_mlp_fwd_nchw': (ci, [vp, vp, cl, ci] + [vp] * 15 + [cl, cl, vp]),
    'cffm_mlp_bwd_nchw': (ci, [vp, cl, ci] + [vp] * 18 + [cl, vp]),
    'cffm_block_forward': (ci, [GP, BP, vp, cl, vp, cl, vp, vp, vp, vp, vp]),
    'cffm_block_backward': (ci, [GP, BP, BP, vp, cl, vp, cl, vp, vp, vp, vp, vp, vp, vp, cl, ci, vp, cl, vp, vp]),
    'cffm_layer_forward': (ci, [GP, ci, BP, vp, vp, vp, vp, vp, vp, vp]),
    'cffm_layer_backward': (ci, [GP, ci, BP, BP, vp, cl, vp, vp, vp, vp, vp, vp, vp, vp]),
    'cffm_layer_backward_range': (ci, [GP, ci, BP, BP, vp, cl, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp]),
    'cffm_layer_forward_full': (ci, [GP, ci, BP, vp, vp, vp, vp, vp, vp, vp]),
    'cffm_layer_backward_full': (ci, [GP, ci, BP, BP, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp]),
    'cffm_gtc_attn_fwd': (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]),
    'cffm_gtc_attn_bwd': (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]),
    'cffm_gtc_ws_floats': (cl, [ci, ci, ci]),
    'cffm_gtc_block_forward': (ci, [GTP, vp, vp, vp, vp, ci, ci, ci, vp]),
    'cffm_gtc_block_backward': (ci, [GTP, GTP, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]),
    'cffm_segfuse_fwd': (ci, [vp, vp, vp * 3, ci * 3, ci * 3, ci, ci, ci, ci, vp]),
    'cffm_segfuse_bwd': (ci, [vp, vp * 3, ci * 3, ci * 3, ci, ci, ci, ci, vp]),
    'cffm_seg_counts': (ci, [vp, vp, cl, ci, ci, ci, vp, vp]),
    'cffm_vc_counts': (ci, [vp, vp, ci, cl, ci, vp, vp]),
    'cffm_layer_forward_rows': (ci, [GP, ci, BP, vp, vp, vp, vp, vp, vp, vp]),
    'cffm_layer_backward_rows': (ci, [GP, ci, BP, BP, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    'cffm_layer_prepared_floats': (cl, [ci]),
    'cffm_layer_prepare': (ci, [ci, BP, vp, vp]),
    'cffm_layer_infer_ws_floats': (cl, [GP]),
    'cffm_layer_infer_rows': (ci, [GP, ci, BP, vp, vp, vp, vp, vp, vp, vp]),
    'cffm_layer_infer_full': (ci, [GP, ci, BP, vp, vp, vp, vp, vp, vp, vp]),
    'cffm_colstats_records': (cl, [cl]),
    'cffm_colstats': (ci, [vp, cl, vp, vp]),
    'cffm_bn_relu_pool_records': (cl, [ci, ci, ci]),
    'cffm_bn_relu_pool_fwd': (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]),
    'cffm_bn_relu_pool_bwd1': (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]),
    'cffm_bn_bwd2': (ci, [vp, vp, vp, vp, vp, vp, vp, cl, vp]),
    'cffm_bn_finalize_fwd': (ci, [vp, cl, cd, vp, vp, vp, vp, cf, cf, vp, vp]),
    'cffm_bn_finalize_bwd': (ci, [vp, cl, cd, vp, vp, ci, vp, vp]),
    'cffm_rows_resize_fwd': (ci, [vp, cl, vp, cl, ci, ci, ci, ci, ci, ci, vp]),
    'cffm_rows_resize_bwd': (ci, [vp, cl, vp, cl, ci, ci, ci, ci, ci, ci, vp]),
    'cffm_clip_format_hsv': (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, C.c_float * 3, C.c_float * 3, ci, C.c_float, ci, ci, vp, vp, vp, vp, vp, vp]),
    'cffm_clip_resize': (ci, [vp, vp, ci, ci, ci, vp, vp, ci, ci, vp]),
    'cffm_upce_blocks': (cl, [ci, ci, ci]),
    'cffm_upce_fwd': (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]),
    'cffm_upce_bwd': (ci, [vp, vp, vp, vp, C.c_float, vp, ci, ci, ci, ci, ci, ci, ci, vp]),
    'cffm_upce_maps_finalize': (ci, [vp, ci, cl, vp, vp, vp, vp]),
    'cffm_upce_maps_fwd': (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, cl, cl, ci, ci, vp]),
    'cffm_upce_maps_bwd': (ci, [vp, vp, vp, vp, vp, vp, C.c_float, vp, ci, ci, ci, ci, ci, ci, ci, ci, cl, cl, ci, ci, vp]),
    'cffm_adamw_step_rows': (ci, [vp, ci, vp, vp, vp, vp, ci, vp, vp, vp]),
    'cffm_kmeans_workspace_bytes': (cl, [cl, ci]),
    'cffm_kmeans': (ci, [vp, cl, ci, ci, vp, vp, vp, vp, vp]),
    'cffm_predict': (ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, cl, cl, ci, ci, vp]),
    'cffm_dwconv_gelu_fwd': (ci, [vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    'cffm_dwconv_gelu_bwd_workspace_bytes': (cl, [ci, ci, ci, ci]),
    'cffm_dwconv_gelu_bwd': (ci, [vp] * 8 + [ci, ci, ci, ci, vp]),
    'cffm_sra_attn_fwd': (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, cf, vp]),
    'cffm_sra_attn_bwd_workspace_bytes': (cl, [ci, ci, ci, ci, ci]),
    'cffm_sra_attn_bwd': (ci, [vp] * 8 + [ci, ci, ci, ci, ci, cf, vp]),
    'cffm_sr_ln_fwd': (ci, [vp] * 8 + [ci, ci, ci, ci, ci, cf, vp]),
    'cffm_sr_ln_bwd_workspace_bytes': (cl, [ci, ci, ci, ci, ci]),
    'cffm_sr_ln_bwd': (ci, [vp] * 12 + [ci, ci, ci, ci, ci, cf, vp]),
    'cffm_ln_rows': (ci, [vp, vp, vp, vp, cl, ci, cf, vp]),
    'cffm_nchw_ln_rows': (ci, [vp, vp, vp, vp, ci, ci, ci, ci, cf, vp]),
    'cffm_ln_rows_nchw': (ci, [vp, vp, vp, vp, ci, ci, ci, ci, cf, vp]),
    'cffm_ln_bwd_workspace_bytes': (cl, [cl, ci, ci]),
    'cffm_ln_rows_bwd': (ci, [vp] * 7 + [cl, ci, cf, vp]),
    'cffm_nchw_ln_rows_bwd': (ci, [vp] * 7 + [ci, ci, ci, ci, cf, vp]),
    'cffm_ln_rows_nchw_bwd': (ci, [vp] * 7 + [ci, ci, ci, ci, cf, vp]),
    'cffm_mit_stage_infer_ws_floats': (cl, [MCP]),
    'cffm_mit_stage_infer': (ci, [MCP, MBP, vp, vp, vp, vp, vp, vp, vp, vp]),
    'cffm_patch_embed_fwd': (ci, [vp] * 6 + [ci] * 7 + [cf, vp]),
    'cffm_patch_embed_fwd_train': (ci, [vp] * 7 + [ci] * 7 + [cf, vp]),
    'cffm_patch_embed_bwd_workspace_bytes': (cl, [ci] * 8),
    'cffm_patch_embed_bwd': (ci, [vp] * 11 + [ci] * 7 + [cf, vp]),
    'cffm_linear_rows_fwd': (ci, [vp] * 6 + [cl, ci, ci, ci, vp]),
    'cffm_linear_rows_bwd_workspace_bytes': (cl, [cl, ci, ci, ci, ci, ci]),
    'cffm_linear_rows_bwd': (ci, [vp] * 8 + [cl, ci, ci, ci, vp]),
    'cffm_mit_infer_ws_floats': (cl, [MSP, ci]),
    'cffm_mit_infer': (ci, [MSP, ci, vp, C.POINTER(vp), vp, vp]),
    'cffm_ln_rows_bwd_add': (ci, [vp] * 9 + [cl, ci, cf, vp]),
    'cffm_mit_blocks_train_saved_floats': (cl, [MCP]),
    'cffm_mit_blocks_train_fwd_ws_floats': (cl, [MCP]),
    'cffm_mit_blocks_train_bwd_ws_floats': (cl, [MCP]),
    'cffm_mit_blocks_train_fwd': (ci, [MCP, MBP, MSC, vp, vp, vp, vp, vp]),
    'cffm_mit_blocks_train_bwd': (ci, [MCP, MBP, MSC, MBP, vp, vp, vp, vp, vp, vp]),
    'cffm_segfuse_pool_fwd': (ci, [vp, vp, vp * 3, ci * 3, ci * 3, ci, vp, vp, vp, cl, ci, vp, ci, ci, ci, ci, vp]),
    'cffm_layer_infer_rows_ring': (ci, [GP, ci, BP, vp, vp, cl, ci, vp, cl, vp, vp, vp, vp, vp]),
    'cffm_segfuse_pool_fwd_frames': (ci, [vp, vp, vp * 3, ci * 3, ci * 3, ci, vp, vp, vp, cl, ci, vp, ci, ci, ci, vp]),
    'cffm_layer_infer_rows_ring_tables': (ci, [GP, ci, BP, vp, vp, cl, ci, vp, vp, vp, vp, vp, vp]),
}


class CffmError(RuntimeError):
    pass


def bind(path):
    """Load a library exporting the C ABI of include/cffm_hip.h and attach the signatures."""
    lib = C.CDLL(path)
    missing = [n for n in SIGNATURES if not hasattr(lib, n)]
    if missing:
        raise CffmError('%s does not export %s' % (path, ', '.join(missing)))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    if lib.cffm_abi_version() != ABI_VERSION:
        raise CffmError('%s: ABI version %d, expected %d' % (path, lib.cffm_abi_version(), ABI_VERSION))
    return lib


_lib = None
_override = None   # set only by tests/emu.py (emulator build of the same kernel sources)


def get():
    """The product library.  Raises CffmError when it has not been built: no fallback."""
    global _lib
    if _override is not None:
        return _override
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise CffmError('libcffm_hip.so is missing (%s): build it with `python -c "import __graft_entry__ as g; '
                            'g.build()"`; the CFFM hot path has no CPU fallback' % LIB_PATH)
        _lib = bind(LIB_PATH)
    return _lib


def check(rc, lib):
    if rc != 0:
        raise CffmError('libcffm_hip: %s (code %d)' % (lib.cffm_last_error().decode(), rc))
