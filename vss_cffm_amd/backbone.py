"""Mix Transformer backbones ``mit_b0`` .. ``mit_b5`` (SegFormer's encoder; the reference's mmseg/models/backbones/mix_transformer.py)
under the reference's class, constructor-keyword and attribute names, so a reference checkpoint's ``backbone.*`` keys load key for key.

Four stages; each is an overlapping patch embedding (strided Conv2d + LayerNorm on token rows), `depth` blocks of spatial-reduction
attention + Mix-FFN with stochastic depth, and a LayerNorm; each stage hands a contiguous NCHW map (strides 4 / 8 / 16 / 32) to the head.

The Mix-FFN is fc1 -> depthwise 3 x 3 Conv2d on the NCHW view -> GELU -> fc2.  With ``Mlp.dwconv_impl = 'hip'`` everything between the
two Linear layers is ONE pass of libcffm_hip.so over the token rows (``ops.dwconv_gelu`` -> cffm_dwconv_gelu_fwd / _bwd): no NCHW view,
no transpose copies, and two saved activations instead of three.  ``'torch'`` is the reference's op sequence in stock PyTorch: the A/B
partner in the tests and what CPU tensors, other dtypes, other activations and dropout > 0 get.

The attention core -- everything between the q / kv Linear layers and proj -- is, with ``Attention.attn_impl = 'hip'``, one forward and
one backward pass of the library (``ops.sra_attention`` -> cffm_sra_attn_fwd / _bwd): q and kv are read where the Linear layers left
them, the score tensor [B, heads, N, Nk] never exists and one log-sum-exp per query is kept for the backward.  ``'torch'`` is the
reference's reshape / permute, matmul, scale, softmax, matmul, transpose / reshape: the A/B partner in the tests and what CPU tensors,
other dtypes, attention dropout > 0 and head sizes other than 32 / 64 get.

In front of kv, stages with sr_ratio > 1 reduce the map with the `sr` convolution (kernel = stride = sr_ratio) and a LayerNorm.  With
``Attention.sr_impl = 'hip'`` both are one GEMM with a LayerNorm epilogue on the token rows (``ops.sr_reduce`` -> cffm_sr_ln_fwd / _bwd):
no NCHW view, no transposes, the Conv2d weight read in its own layout.  ``'torch'`` is the reference's permute / reshape, Conv2d,
reshape / permute, LayerNorm: the default (the fused pass is exact fp32 but, as measured, not faster at model level),
the A/B partner in the tests and what CPU tensors, other dtypes and shapes outside the kernel's limits get.  `sr_impl` is independent
of `attn_impl`.  The three Linear layers are stock PyTorch either way (unless `linear_impl`, below, says otherwise).

For inference, ``MixVisionTransformer.stage_impl = 'hip'`` runs everything of a stage behind ``patch_embed.proj`` -- the embedding's
LayerNorm, every block, the stage's LayerNorm and the change to an NCHW map -- as ONE library call (``ops.mit_stage_infer`` ->
cffm_mit_stage_infer), the Linear layers as the library's bf16-split GEMMs.  ``'torch'`` (the default) is the path described above.  A
stage takes the call only when nothing would be differentiated and it is inside the library's limits (`_stage_fused`); any other stage
takes the path above, stage by stage and silently.  `dwconv_impl`, `attn_impl` and `sr_impl` have no say in the stage call.

With ``MixVisionTransformer.embed_impl = 'hip'`` on top of ``stage_impl = 'hip'`` the patch-embedding convolutions join in: every maximal
run of consecutive stages that take the stage call and whose ``patch_embed.proj`` is inside the limits of the library's patch-embedding
kernel goes out as ONE call (``ops.mit_infer`` -> cffm_mit_infer) -- for ``mit_b0`` .. ``mit_b5`` the whole evaluation forward, with one
workspace (the largest stage's) and the same bits on every call.  ``'torch'`` (the default) leaves the convolutions to stock Conv2d.

On the modules' own path -- the one a training pass takes -- ``norm_impl = 'hip'`` (``MixVisionTransformer.set_norm_impl``) hands every
LayerNorm to the library in both directions (``ops.layer_norm_rows`` / ``nchw_layer_norm_rows`` / ``layer_norm_rows_nchw`` -> cffm_ln_rows* and
their ``_bwd`` partners): the embedding's flatten / transpose and the stage's reshape / permute / contiguous happen inside the same pass, the
backward recomputes mean and rstd from the saved input, and the weight / bias gradients are summed in a fixed order.  ``'torch'`` (the
default) is stock nn.LayerNorm, which is also what any norm outside the kernels' limits gets.

On the same path ``conv_impl = 'hip'`` (``MixVisionTransformer.set_conv_impl``) hands each overlapping patch embedding -- the strided
convolution, flatten / transpose and its LayerNorm -- to the library as one call per direction (``ops.overlap_patch_embed`` ->
cffm_patch_embed_fwd_train / cffm_patch_embed_bwd): bf16-split products, every gradient summed in a fixed order.  ``'torch'`` (the default)
is stock Conv2d, which is also what a convolution outside the kernel's limits and a 7 x 7 embedding whose input requires grad get.

And ``linear_impl = 'hip'`` (``MixVisionTransformer.set_linear_impl``) hands the five Linear layers of every block to the library in both
directions (``ops.linear_rows`` -> cffm_linear_rows_fwd / cffm_linear_rows_bwd): q, kv and fc1 as they are; proj and fc2 with the block input
as the residual and the DropPath factor of each sample as a scale in the GEMM's epilogue, so that each residual line of ``Block.forward`` is one
call.  The factor is drawn as ``DropPath.forward`` draws it, so both settings consume the generator alike and drop the same samples.  ``'torch'``
(the default) is stock nn.Linear and the reference's residual lines, which is also what tensors outside the limits, other dtypes, CPU tensors
and modules with ``proj_drop`` / ``drop`` > 0 get.

On top of these, ``block_impl = 'hip'`` (``MixVisionTransformer.set_block_impl``) hands ALL blocks of a stage to the library as one call per
direction in a training pass (``ops.mit_blocks_train`` -> cffm_mit_blocks_train_fwd / _bwd): the same kernels in the same order as the five
per-op switches on 'hip', with one `saved` buffer, one workspace and no eager call between them, and the two adds autograd puts around a
block's LayerNorms inside the LayerNorm backward.  The result and every gradient have the bits of the per-op path, the DropPath factors are
drawn before the call in the modules' order, so the same samples drop.  ``'torch'`` (the default) is the path described above, which is also
what a stage gets under no_grad, with nothing to differentiate, outside the library's limits or with a block that is not plain
(`_blocks_fused`).  The patch embedding and the stage's norm stay on the modules' own path either way.
"""
import math
from functools import partial

import torch
import torch.nn as nn

from . import _lib
from .checkpoint import load_reference_checkpoint
from .ops import (dwconv_gelu, layer_norm_rows, layer_norm_rows_nchw, linear_rows, linear_rows_supported, ln_supported, mit_blocks_cfg,
                  mit_blocks_train, mit_blocks_train_supported, mit_infer, mit_stage_cfg, mit_stage_infer, mit_stage_supported, mit_stage_tensors, mit_stages, nchw_layer_norm_rows, overlap_patch_embed,
                  patch_embed_out_hw, patch_embed_supported, sr_reduce, sr_reduce_supported, sra_attention)
from .registry import BACKBONES


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _norm_fused(impl, norm, x, c):
    """whether `norm` of x, whose rows are c wide, takes the library's LayerNorm (norm_impl = 'hip'): a plain affine nn.LayerNorm over the
    last c channels, fp32 tensors on the GPU (or under the emulator override), inside the kernels' limits.  Anything else: the stock line."""
    return (impl == 'hip' and type(norm) is nn.LayerNorm and norm.elementwise_affine and norm.bias is not None
            and tuple(norm.normalized_shape) == (c,) and (x.is_cuda or _lib._override is not None) and x.dtype == torch.float32
            and norm.weight.dtype == torch.float32 and norm.weight.device == x.device and ln_supported(c, x.numel()))


def _norm_rows(impl, norm, x):
    """norm(x) of token rows [..., C]: one library call per direction with norm_impl = 'hip', the module's own forward otherwise"""
    if _norm_fused(impl, norm, x, x.shape[-1]):
        return layer_norm_rows(x, norm.weight, norm.bias, norm.eps)
    return norm(x)


def _linear_fused(impl, lin, x, drop=None):
    """whether `lin` of the token rows x takes the library's Linear (linear_impl = 'hip'): a plain nn.Linear on fp32 rows [B, N, C] or [M, C] on
    the GPU (or under the emulator override), parameters where x is, inside the kernels' limits, and no dropout (`drop`: the nn.Dropout of the
    owning module that sits behind its last Linear).  Anything else: the stock line."""
    if impl != 'hip' or type(lin) is not nn.Linear or not (x.is_cuda or _lib._override is not None) or x.dtype != torch.float32:
        return False
    if x.dim() not in (2, 3) or x.numel() == 0 or x.shape[-1] != lin.in_features or (drop is not None and drop.p != 0):
        return False
    if any(t is not None and (t.dtype != torch.float32 or t.device != x.device) for t in (lin.weight, lin.bias)):
        return False
    return linear_rows_supported(lin.in_features, lin.out_features, x.numel() // x.shape[-1])


def _linear_rows(impl, lin, x, drop=None):
    """lin(x) of token rows: one library call per direction with linear_impl = 'hip', the module's own forward otherwise"""
    if _linear_fused(impl, lin, x, drop):
        return linear_rows(x, lin.weight, lin.bias)
    return lin(x)


def _drop_scale(drop_path, x):
    """the factor DropPath.forward multiplies each sample of x with, as a [B] tensor, drawn with DropPath's own torch.rand call (the same
    shape, dtype and device: the generator moves as it does there); None where DropPath is the identity"""
    if type(drop_path) is not DropPath or drop_path.drop_prob == 0. or not drop_path.training:
        return None
    keep = 1 - drop_path.drop_prob
    mask = keep + torch.rand((x.shape[0],) + (1,) * (x.dim() - 1), dtype=x.dtype, device=x.device)
    return mask.floor_().div_(keep).reshape(-1)


def _residual_linear(impl, lin, x, drop, residual, drop_path):
    """residual + drop_path(drop(lin(x))): with linear_impl = 'hip' one library call, DropPath's factor and the residual in the GEMM's
    epilogue; the reference's line otherwise"""
    if (_linear_fused(impl, lin, x, drop) and type(drop_path) in (DropPath, nn.Identity) and residual.dtype == torch.float32
            and residual.device == x.device and tuple(residual.shape) == tuple(x.shape[:-1]) + (lin.out_features,)):
        return linear_rows(x, lin.weight, lin.bias, residual, _drop_scale(drop_path, x))
    return residual + drop_path(drop(lin(x)))


def _init_weights(m):
    """the reference's _init_weights: Linear ~ truncated N(0, 0.02) with zero bias, LayerNorm 1 / 0, Conv2d ~ N(0, sqrt(2 / fan_out))"""
    if isinstance(m, nn.Linear):
        nn.init.trunc_normal_(m.weight, std=.02)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, nn.LayerNorm):
        nn.init.constant_(m.bias, 0)
        nn.init.constant_(m.weight, 1.0)
    elif isinstance(m, nn.Conv2d):
        fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
        m.weight.data.normal_(0, math.sqrt(2.0 / fan_out))
        if m.bias is not None:
            m.bias.data.zero_()


class DropPath(nn.Module):
    """Stochastic depth per sample (timm's DropPath): in training the residual branch of a sample is dropped with probability
    `drop_prob` and the kept ones are scaled by 1 / keep.  Identity in eval mode and at drop_prob = 0."""

    def __init__(self, drop_prob=0.):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        if self.drop_prob == 0. or not self.training:
            return x
        keep = 1 - self.drop_prob
        mask = keep + torch.rand((x.shape[0],) + (1,) * (x.dim() - 1), dtype=x.dtype, device=x.device)
        return x.div(keep) * mask.floor_()

    def extra_repr(self):
        return 'drop_prob=%s' % (self.drop_prob,)


class DWConv(nn.Module):
    """depthwise 3 x 3 convolution of token rows [B, H*W, C] through their NCHW view"""

    def __init__(self, dim=768):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, 3, 1, 1, bias=True, groups=dim)

    def forward(self, x, H, W):
        B, N, C = x.shape
        x = self.dwconv(x.transpose(1, 2).view(B, C, H, W))
        return x.flatten(2).transpose(1, 2)


class Mlp(nn.Module):
    # 'hip': dwconv + bias + GELU in one kernel of libcffm_hip.so for fp32 GPU tensors (it raises when the library is missing);
    # 'torch': the reference's op sequence (what everything else gets, and the A/B partner in the tests)
    dwconv_impl = 'hip'
    linear_impl = 'torch'      # 'hip': fc1 / fc2 are the library's Linear, forward and backward (see MixVisionTransformer.linear_impl)

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.dwconv = DWConv(hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)
        self.apply(_init_weights)

    def _fused(self, x):
        return (self.dwconv_impl == 'hip' and (x.is_cuda or _lib._override is not None) and x.dtype == torch.float32
                and type(self.act) is nn.GELU and getattr(self.act, 'approximate', 'none') == 'none' and self.drop.p == 0
                and x.shape[-1] % 4 == 0)

    def forward(self, x, H, W, residual=None, drop_path=None):
        """residual / drop_path: handed in by a Block with linear_impl = 'hip'; the result is then the whole residual line
        residual + drop_path(mlp(x))"""
        x = _linear_rows(self.linear_impl, self.fc1, x, self.drop)
        if self._fused(x):
            x = dwconv_gelu(x, self.dwconv.dwconv.weight, self.dwconv.dwconv.bias, H, W)
        else:
            x = self.drop(self.act(self.dwconv(x, H, W)))
        if residual is not None:
            return _residual_linear(self.linear_impl, self.fc2, x, self.drop, residual, drop_path)
        return self.drop(_linear_rows(self.linear_impl, self.fc2, x, self.drop))


class Attention(nn.Module):
    """multi-head self-attention whose keys / values come from the map reduced by a strided `sr` convolution (sr_ratio > 1)"""
    # 'hip': q k^T, scale, softmax, attn v in one kernel of libcffm_hip.so for fp32 GPU tensors (it raises when the library is missing);
    # 'torch': the reference's op sequence (what everything else gets, and the A/B partner in the tests)
    attn_impl = 'hip'
    # 'hip': the `sr` convolution + LayerNorm as one pass of libcffm_hip.so over the token rows for fp32 GPU tensors inside the kernel's
    # limits (it raises when the library is missing); 'torch': the reference's op sequence, what everything else gets -- and the
    # default: as measured the fused pass does not make a mit_b1 training pass faster
    sr_impl = 'torch'
    # 'hip': the LayerNorm behind the stock `sr` convolution is the library's, forward and backward (see MixVisionTransformer.norm_impl)
    norm_impl = 'torch'
    # 'hip': q / kv / proj are the library's Linear, forward and backward (see MixVisionTransformer.linear_impl)
    linear_impl = 'torch'

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0., sr_ratio=1):
        super().__init__()
        assert dim % num_heads == 0, 'dim %d should be divided by num_heads %d.' % (dim, num_heads)
        self.dim = dim
        self.num_heads = num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.q = nn.Linear(dim, dim, bias=qkv_bias)
        self.kv = nn.Linear(dim, dim * 2, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.sr_ratio = sr_ratio
        if sr_ratio > 1:
            self.sr = nn.Conv2d(dim, dim, kernel_size=sr_ratio, stride=sr_ratio)
            self.norm = nn.LayerNorm(dim)
        self.apply(_init_weights)

    def _fused(self, x):
        return (self.attn_impl == 'hip' and (x.is_cuda or _lib._override is not None) and x.dtype == torch.float32
                and self.attn_drop.p == 0 and x.shape[-1] // self.num_heads in (32, 64) and self.scale > 0)

    def _sr_fused(self, x, H, W):
        # (decided by the tensors' dtype alone, as _fused: under torch.autocast the 'hip' pass stays fp32 where the Conv2d would not)
        return (self.sr_impl == 'hip' and self.sr_ratio > 1 and (x.is_cuda or _lib._override is not None) and x.dtype == torch.float32
                and self.sr.weight.dtype == torch.float32 and sr_reduce_supported(x.shape[0], H, W, x.shape[2], self.sr_ratio))

    def _reduced(self, x, H, W):
        B, N, C = x.shape
        if self._sr_fused(x, H, W):
            return sr_reduce(x, self.sr.weight, self.sr.bias, self.norm.weight, self.norm.bias, H, W, self.sr_ratio, self.norm.eps)
        return _norm_rows(self.norm_impl, self.norm, self.sr(x.permute(0, 2, 1).reshape(B, C, H, W)).reshape(B, C, -1).permute(0, 2, 1))

    def _lin(self, lin, x):
        return _linear_rows(self.linear_impl, lin, x, self.proj_drop)

    def _tail(self, x, residual, drop_path):
        if residual is not None:
            return _residual_linear(self.linear_impl, self.proj, x, self.proj_drop, residual, drop_path)
        return self.proj_drop(self._lin(self.proj, x))

    def forward(self, x, H, W, residual=None, drop_path=None):
        """residual / drop_path: handed in by a Block with linear_impl = 'hip'; the result is then the whole residual line
        residual + drop_path(attn(x))"""
        B, N, C = x.shape
        if self._fused(x):
            kv = self._lin(self.kv, self._reduced(x, H, W) if self.sr_ratio > 1 else x)
            return self._tail(sra_attention(self._lin(self.q, x), kv, self.num_heads, self.scale), residual, drop_path)
        hd = C // self.num_heads
        q = self._lin(self.q, x).reshape(B, N, self.num_heads, hd).permute(0, 2, 1, 3)
        if self.sr_ratio > 1:
            x = self._reduced(x, H, W)
        k, v = self._lin(self.kv, x).reshape(B, -1, 2, self.num_heads, hd).permute(2, 0, 3, 1, 4)
        attn = self.attn_drop(((q @ k.transpose(-2, -1)) * self.scale).softmax(dim=-1))
        return self._tail((attn @ v).transpose(1, 2).reshape(B, N, C), residual, drop_path)


class Block(nn.Module):
    norm_impl = 'torch'        # 'hip': norm1 / norm2 are the library's LayerNorm, forward and backward (see MixVisionTransformer.norm_impl)
    # 'hip': each residual line is closed inside attn / mlp, by the library's Linear where proj / fc2 are eligible (MixVisionTransformer.linear_impl)
    linear_impl = 'torch'

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, sr_ratio=1):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop,
                              sr_ratio=sr_ratio)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.apply(_init_weights)

    def forward(self, x, H, W):
        if self.linear_impl == 'hip':
            x = self.attn(_norm_rows(self.norm_impl, self.norm1, x), H, W, residual=x, drop_path=self.drop_path)
            return self.mlp(_norm_rows(self.norm_impl, self.norm2, x), H, W, residual=x, drop_path=self.drop_path)
        x = x + self.drop_path(self.attn(_norm_rows(self.norm_impl, self.norm1, x), H, W))
        return x + self.drop_path(self.mlp(_norm_rows(self.norm_impl, self.norm2, x), H, W))


class OverlapPatchEmbed(nn.Module):
    """image (or the previous stage's map) -> token rows: a strided convolution with overlapping windows, then LayerNorm"""
    # 'hip': flatten / transpose + norm are one library call per direction, no transposed copy (see MixVisionTransformer.norm_impl)
    norm_impl = 'torch'
    # 'hip': convolution + flatten / transpose + norm are one library call per direction (see MixVisionTransformer.conv_impl)
    conv_impl = 'torch'

    def __init__(self, img_size=224, patch_size=7, stride=4, in_chans=3, embed_dim=768):
        super().__init__()
        self.img_size, self.patch_size = _pair(img_size), _pair(patch_size)
        self.H, self.W = self.img_size[0] // self.patch_size[0], self.img_size[1] // self.patch_size[1]
        self.num_patches = self.H * self.W
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=stride,
                              padding=(self.patch_size[0] // 2, self.patch_size[1] // 2))
        self.norm = nn.LayerNorm(embed_dim)
        self.apply(_init_weights)

    def _conv_fused(self, x):
        """whether this input takes the library's embedding (conv_impl = 'hip'): fp32 tensors on the GPU (or under the emulator override), a
        convolution inside the kernel's limits, a plain affine nn.LayerNorm, parameters where the kernels can read them, and no input
        gradient through a 7 x 7 convolution.  Anything else: the stock line."""
        proj, norm = self.proj, self.norm
        if self.conv_impl != 'hip' or not (x.is_cuda or _lib._override is not None) or x.dtype != torch.float32:
            return False
        if not patch_embed_supported(proj, x.shape) or type(norm) is not nn.LayerNorm or not norm.elementwise_affine or norm.bias is None:
            return False
        if tuple(norm.normalized_shape) != (proj.out_channels,):
            return False
        ts = (proj.weight, proj.bias, norm.weight, norm.bias)
        if any(t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous() or t.data_ptr() % 16 for t in ts):
            return False
        return not (proj.kernel_size[0] == 7 and x.requires_grad and torch.is_grad_enabled())

    def forward(self, x):
        if self._conv_fused(x):
            return overlap_patch_embed(x, self.proj, self.norm)
        x = self.proj(x)
        H, W = x.shape[2:]
        if _norm_fused(self.norm_impl, self.norm, x, x.shape[1]):
            return nchw_layer_norm_rows(x, self.norm.weight, self.norm.bias, self.norm.eps), H, W
        return self.norm(x.flatten(2).transpose(1, 2)), H, W


class MixVisionTransformer(nn.Module):
    # 'hip': under no_grad (or with nothing that requires grad) each stage behind its patch-embedding convolution is one call of
    # libcffm_hip.so for fp32 GPU tensors inside the library's limits (it raises when the library is missing); 'torch': the modules'
    # own forward, what everything else gets -- and the default: whether the call is faster is measured, not assumed
    stage_impl = 'torch'
    # 'hip' (with stage_impl = 'hip'): consecutive stages that take the stage call and whose patch-embedding convolution is inside the
    # library's limits are ONE call, convolutions included; 'torch': stock Conv2d in front of every stage call -- the default
    # (DESIGN section 3t has the measurements: not faster at model level)
    embed_impl = 'torch'
    # 'hip': on the modules' own path (the one a training pass takes) every LayerNorm -- the embeddings', the blocks' norm1 / norm2, the
    # one behind a stock `sr` convolution, the stages' -- is the library's, forward and backward, the embeddings' and the stages' with
    # their change of layout in the same pass (ops.layer_norm_rows / nchw_layer_norm_rows / layer_norm_rows_nchw): fp32 GPU tensors and
    # plain affine nn.LayerNorms of a width inside the kernels' limits; any other norm takes the stock line, silently.  'torch': stock
    # F.layer_norm -- the default (DESIGN section 3v has the measurements).  The owners of the call sites carry an attribute of the same
    # name; set_norm_impl sets them all.
    norm_impl = 'torch'
    # 'hip': on the modules' own path each OverlapPatchEmbed -- convolution, flatten / transpose, LayerNorm -- is one library call per
    # direction (ops.overlap_patch_embed): fp32 GPU tensors, a convolution inside the kernel's limits; anything else, and a 7 x 7
    # embedding whose input requires grad, takes the stock line, silently.  'torch': stock Conv2d -- the default (DESIGN section 3w has
    # the measurements).  The inference paths (stage_impl, embed_impl) are not touched and win where they apply.
    conv_impl = 'torch'
    # 'hip': on the modules' own path the five Linear layers of every block -- q, kv, proj, fc1, fc2 -- are the library's bf16-split GEMMs,
    # forward and backward (ops.linear_rows), proj and fc2 with the residual and the DropPath factor in the epilogue: fp32 GPU tensors
    # inside the kernels' limits, proj_drop.p == 0 and mlp.drop.p == 0; anything else takes the stock line, silently.  'torch': stock
    # nn.Linear -- the default (DESIGN section 3z has the measurements).  Attention, Mlp and Block carry an attribute of the same name;
    # set_linear_impl sets them all.
    linear_impl = 'torch'
    # 'hip': in a training pass (grad mode on, something to differentiate) all blocks of a stage are ONE library call per direction
    # (ops.mit_blocks_train): fp32 GPU tensors, a stage inside the limits of cffm_mit_stage_infer, plain blocks (nn.Linear, affine
    # nn.LayerNorm, no dropout, DropPath or Identity); any other stage takes the loop over its blocks, silently, and under no_grad the
    # switch has no say.  'torch': the loop over the blocks -- the default (DESIGN section 3aa has the measurements).
    block_impl = 'torch'

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dims=[64, 128, 256, 512], num_heads=[1, 2, 4, 8],
                 mlp_ratios=[4, 4, 4, 4], qkv_bias=False, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.,
                 norm_layer=nn.LayerNorm, depths=[3, 4, 6, 3], sr_ratios=[8, 4, 2, 1]):
        super().__init__()
        self.num_classes = num_classes
        self.depths = depths
        dpr = self._rates(drop_path_rate)
        chans = [in_chans] + list(embed_dims)
        for i in range(4):
            self.add_module('patch_embed%d' % (i + 1), OverlapPatchEmbed(
                img_size=img_size if i == 0 else img_size // (2 ** (i + 1)), patch_size=7 if i == 0 else 3, stride=4 if i == 0 else 2,
                in_chans=chans[i], embed_dim=chans[i + 1]))
        # (all patch embeddings first, then block1, norm1, block2, ...: the order of the reference's state_dict)
        for i in range(4):
            self.add_module('block%d' % (i + 1), nn.ModuleList([
                Block(dim=embed_dims[i], num_heads=num_heads[i], mlp_ratio=mlp_ratios[i], qkv_bias=qkv_bias, qk_scale=qk_scale,
                      drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[i][j], norm_layer=norm_layer, sr_ratio=sr_ratios[i])
                for j in range(depths[i])]))
            self.add_module('norm%d' % (i + 1), norm_layer(embed_dims[i]))
        self.apply(_init_weights)

    def _rates(self, drop_path_rate):
        """the drop-path rate of every block, rising linearly from 0 to `drop_path_rate` over all blocks, per stage"""
        flat = [x.item() for x in torch.linspace(0, drop_path_rate, sum(self.depths))]
        out, cur = [], 0
        for d in self.depths:
            out.append(flat[cur:cur + d])
            cur += d
        return out

    def init_weights(self, pretrained=None, trusted=False):
        """pretrained: a checkpoint path, loaded non-strictly (missing / unexpected / mismatched keys are reported, not raised): a bare
        backbone state dict (ImageNet files carry extra ``head.*`` keys) or an mmcv-format model checkpoint, of which the
        ``backbone.``-prefixed keys are taken.  Returns (missing, unexpected) for a path, None otherwise."""
        if not (isinstance(pretrained, (str, bytes)) or hasattr(pretrained, '__fspath__')):
            return None
        missing, unexpected, _ = load_reference_checkpoint(self, pretrained, prefix='backbone.', strict=False, trusted=trusted)
        if missing or unexpected:
            print('%s.init_weights(%s): missing keys %s, unexpected keys %s' % (type(self).__name__, pretrained, missing, unexpected))
        return missing, unexpected

    def reset_drop_path(self, drop_path_rate):
        for i, rates in enumerate(self._rates(drop_path_rate)):
            for blk, r in zip(getattr(self, 'block%d' % (i + 1)), rates):
                blk.drop_path.drop_prob = r

    def set_norm_impl(self, impl):
        """norm_impl of the model and of every submodule that owns a LayerNorm call site"""
        if impl not in ('torch', 'hip'):
            raise ValueError("norm_impl must be 'torch' or 'hip', got %r" % (impl,))
        for m in self.modules():
            if hasattr(type(m), 'norm_impl'):
                m.norm_impl = impl

    def set_conv_impl(self, impl):
        """conv_impl of the model and of every patch embedding"""
        if impl not in ('torch', 'hip'):
            raise ValueError("conv_impl must be 'torch' or 'hip', got %r" % (impl,))
        for m in self.modules():
            if hasattr(type(m), 'conv_impl'):
                m.conv_impl = impl

    def set_linear_impl(self, impl):
        """linear_impl of the model and of every Attention, Mlp and Block"""
        if impl not in ('torch', 'hip'):
            raise ValueError("linear_impl must be 'torch' or 'hip', got %r" % (impl,))
        for m in self.modules():
            if hasattr(type(m), 'linear_impl'):
                m.linear_impl = impl

    def set_block_impl(self, impl):
        """block_impl of the model: 'hip' = every eligible stage's blocks as one library call per direction in a training pass"""
        if impl not in ('torch', 'hip'):
            raise ValueError("block_impl must be 'torch' or 'hip', got %r" % (impl,))
        self.block_impl = impl

    def _blocks_fused(self, blocks, x, H, W):
        """whether the blocks of a stage take the one-call training path for these token rows: block_impl = 'hip', grad mode on and something
        to differentiate, fp32 tensors on the GPU (or under the emulator override), plain blocks of one configuration, parameters where
        the kernels can read them, sizes inside the library's limits"""
        if self.block_impl != 'hip' or len(blocks) == 0 or not torch.is_grad_enabled():
            return False
        if not (x.is_cuda or _lib._override is not None) or x.dtype != torch.float32 or x.dim() != 3 or x.numel() == 0:
            return False
        c, b0 = x.shape[-1], blocks[0]
        ts = []
        for blk in blocks:
            a, m = blk.attn, blk.mlp
            norms = [blk.norm1, blk.norm2] + ([a.norm] if a.sr_ratio > 1 else [])
            if any(type(n) is not nn.LayerNorm or not n.elementwise_affine or n.bias is None or tuple(n.normalized_shape) != (c,) for n in norms):
                return False
            if blk.norm1.eps != b0.norm1.eps or blk.norm2.eps != b0.norm1.eps or (a.sr_ratio > 1 and a.norm.eps != b0.attn.norm.eps):
                return False
            if any(type(lin) is not nn.Linear for lin in (a.q, a.kv, a.proj, m.fc1, m.fc2)):
                return False
            if any(lin.bias is None for lin in (a.proj, m.fc1, m.fc2)) or a.attn_drop.p or a.proj_drop.p or m.drop.p:
                return False
            if type(blk.drop_path) not in (DropPath, nn.Identity):
                return False
            if type(m.act) is not nn.GELU or getattr(m.act, 'approximate', 'none') != 'none':
                return False
            if (a.num_heads, a.scale, a.sr_ratio, m.fc1.out_features) != (b0.attn.num_heads, b0.attn.scale, b0.attn.sr_ratio, b0.mlp.fc1.out_features):
                return False
            if (a.q.in_features, a.q.out_features, a.kv.out_features, a.proj.out_features, m.fc1.in_features, m.fc2.out_features) != (c, c, 2 * c, c, c, c):
                return False
            dw = m.dwconv.dwconv
            if type(dw) is not nn.Conv2d or tuple(dw.weight.shape) != (m.fc1.out_features, 1, 3, 3) or dw.bias is None or dw.padding != (1, 1) or dw.stride != (1, 1):
                return False
            if a.sr_ratio > 1:
                s = a.sr_ratio
                if type(a.sr) is not nn.Conv2d or tuple(a.sr.weight.shape) != (c, c, s, s) or a.sr.bias is None or a.sr.stride != (s, s) or a.sr.padding != (0, 0):
                    return False
            ts += [p for p in blk.parameters()]
        if any(t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous() or t.data_ptr() % 16 for t in ts):
            return False
        if not (x.requires_grad or any(t.requires_grad for t in ts)):
            return False
        return mit_blocks_train_supported(mit_blocks_cfg(x.shape, H, W, blocks))

    def freeze_patch_emb(self):
        self.patch_embed1.requires_grad = False      # (as in the reference: an attribute on the module, the parameters keep theirs)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'pos_embed1', 'pos_embed2', 'pos_embed3', 'pos_embed4', 'cls_token'}

    def _stage_fused(self, i, x):
        """whether stage i takes the one-call inference path for this input (the convolution's output shape decides the sizes)"""
        return self._stage_fused_at(i, tuple(x.shape), x)

    def _stage_fused_at(self, i, shape, x):
        """_stage_fused for an input of `shape` that is like x in everything else (device, dtype, requires_grad)"""
        pe, blocks, norm = getattr(self, 'patch_embed%d' % i), getattr(self, 'block%d' % i), getattr(self, 'norm%d' % i)
        if self.stage_impl != 'hip' or not (x.is_cuda or _lib._override is not None) or x.dtype != torch.float32 or len(blocks) == 0:
            return False
        if type(pe.norm) is not nn.LayerNorm or type(norm) is not nn.LayerNorm:
            return False
        b0 = blocks[0]
        for blk in blocks:
            a, m = blk.attn, blk.mlp
            if type(blk.norm1) is not nn.LayerNorm or type(blk.norm2) is not nn.LayerNorm or blk.norm1.eps != b0.norm1.eps or blk.norm2.eps != b0.norm1.eps:
                return False
            if a.sr_ratio > 1 and (type(a.norm) is not nn.LayerNorm or a.norm.eps != b0.attn.norm.eps):
                return False
            if (a.num_heads, a.scale, a.sr_ratio, m.fc1.out_features) != (b0.attn.num_heads, b0.attn.scale, b0.attn.sr_ratio, b0.mlp.fc1.out_features):
                return False
            if type(m.act) is not nn.GELU or getattr(m.act, 'approximate', 'none') != 'none':
                return False
            if self.training and (a.attn_drop.p or a.proj_drop.p or m.drop.p or getattr(blk.drop_path, 'drop_prob', 0.)):
                return False
        norms = [pe.norm, norm] + [n for blk in blocks for n in (blk.norm1, blk.norm2)] + [blk.attn.norm for blk in blocks if blk.attn.sr_ratio > 1]
        if any(not n.elementwise_affine or n.bias is None for n in norms):
            return False
        ts = [t for t in mit_stage_tensors(blocks, pe.norm, norm) if t is not None]
        if any(t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous() or t.data_ptr() % 16 for t in ts):
            return False
        if any(t is None for t in (b0.attn.proj.bias, b0.mlp.fc1.bias, b0.mlp.fc2.bias)):
            return False
        conv = pe.proj
        if torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in ts + list(conv.parameters()))):
            return False
        hw = [(shape[2 + d] + 2 * conv.padding[d] - conv.dilation[d] * (conv.kernel_size[d] - 1) - 1) // conv.stride[d] + 1 for d in (0, 1)]
        return mit_stage_supported(mit_stage_cfg((shape[0], conv.out_channels, hw[0], hw[1]), blocks, pe.norm, norm))

    def _embed_fused_at(self, i, shape, x):
        """whether stage i's patch-embedding convolution, on an input of `shape` that is like x in everything else, is inside the limits
        of the library's kernel (asked only of a stage that passes _stage_fused_at)"""
        conv = getattr(self, 'patch_embed%d' % i).proj
        if self.embed_impl != 'hip' or not patch_embed_supported(conv, shape):
            return False
        return not any(t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous() or t.data_ptr() % 16 for t in (conv.weight, conv.bias))

    def _run_from(self, i, x):
        """the maximal run of consecutive stages from stage i on that go out as one cffm_mit_infer call for this input (may be empty), and
        the shapes of their outputs"""
        run, shapes, shape = [], [], tuple(x.shape)
        while i + len(run) <= 4:
            j = i + len(run)
            if not (self._stage_fused_at(j, shape, x) and self._embed_fused_at(j, shape, x)):
                break
            conv = getattr(self, 'patch_embed%d' % j).proj
            shape = (shape[0], conv.out_channels) + patch_embed_out_hw(conv, shape[2], shape[3])
            run.append(j)
            shapes.append(shape)
        return run, shapes

    def _run_ws(self, run, x, shapes, stages):
        """the workspace of a run's call: one per (first stage, device), the last shapes'; a plain attribute as _stage_workspaces"""
        key = (run[0], x.device, tuple(x.shape)) + tuple(shapes)
        cache = self.__dict__.setdefault('_run_workspaces', {})
        if key not in cache:
            arr, keep, _ = mit_stages(x.shape, stages)
            need = _lib.get().cffm_mit_infer_ws_floats(arr, len(stages))
            if need < 0:
                raise _lib.CffmError('libcffm_hip: %s' % _lib.get().cffm_last_error().decode())
            for k in [k for k in cache if k[0] == run[0] and k[1] == x.device]:
                del cache[k]
            cache[key] = torch.empty(need, dtype=torch.float32, device=x.device)
        return cache[key]

    def _stage_ws(self, i, y):
        """the stage call's workspace: allocated once per (stage, device, cfg), kept on the module as a plain attribute (no buffer, no
        state_dict entry); the only state of the 'hip' path"""
        blocks = getattr(self, 'block%d' % i)
        cfg = mit_stage_cfg(y.shape, blocks, getattr(self, 'patch_embed%d' % i).norm, getattr(self, 'norm%d' % i))
        key = (i, y.device) + tuple(getattr(cfg, f) for f, _ in cfg._fields_ if f != 'depth')
        cache = self.__dict__.setdefault('_stage_workspaces', {})
        if key not in cache:
            need = _lib.get().cffm_mit_stage_infer_ws_floats(cfg)
            if need < 0:
                raise _lib.CffmError('libcffm_hip: %s' % _lib.get().cffm_last_error().decode())
            for k in [k for k in cache if k[0] == i and k[1] == y.device]:      # one workspace per stage and device: the last shape's
                del cache[k]
            cache[key] = torch.empty(need, dtype=torch.float32, device=y.device)
        return cache[key]

    def forward_features(self, x):
        B = x.shape[0]
        outs = []
        skip = 0
        for i in range(1, 5):
            if skip:                                  # (part of the run a call below has finished)
                skip -= 1
                continue
            run, shapes = self._run_from(i, x) if self.embed_impl == 'hip' and self.stage_impl == 'hip' else ([], [])
            if run:
                stages = [(getattr(self, 'patch_embed%d' % j), getattr(self, 'block%d' % j), getattr(self, 'norm%d' % j)) for j in run]
                with torch.no_grad():
                    outs += mit_infer(x, stages, ws=self._run_ws(run, x, shapes, stages))
                x, skip = outs[-1], len(run) - 1
                continue
            if self._stage_fused(i, x):
                pe = getattr(self, 'patch_embed%d' % i)
                with torch.no_grad():
                    y = pe.proj(x)
                    x = mit_stage_infer(y, pe.norm, getattr(self, 'block%d' % i), getattr(self, 'norm%d' % i), ws=self._stage_ws(i, y))
                outs.append(x)
                continue
            x, H, W = getattr(self, 'patch_embed%d' % i)(x)
            blocks = getattr(self, 'block%d' % i)
            if self._blocks_fused(blocks, x, H, W):
                # the DropPath factors in the order the modules draw them: block 0 attention line, block 0 Mix-FFN line, block 1 ...
                scales = [(_drop_scale(blk.drop_path, x), _drop_scale(blk.drop_path, x)) for blk in blocks]
                x = mit_blocks_train(x, blocks, H, W, scales)
            else:
                for blk in blocks:
                    x = blk(x, H, W)
            norm = getattr(self, 'norm%d' % i)
            if _norm_fused(self.norm_impl, norm, x, x.shape[-1]):
                x = layer_norm_rows_nchw(x, norm.weight, norm.bias, H, W, norm.eps)
            else:
                x = norm(x).reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()
            outs.append(x)
        return outs

    def forward(self, x):
        return self.forward_features(x)


def _variant(name, embed_dims, depths):
    def __init__(self, **kwargs):          # the configs pass style='pytorch' (and nothing else is honoured by the reference either)
        MixVisionTransformer.__init__(self, patch_size=4, embed_dims=list(embed_dims), num_heads=[1, 2, 5, 8], mlp_ratios=[4, 4, 4, 4],
                                      qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), depths=list(depths),
                                      sr_ratios=[8, 4, 2, 1], drop_rate=0.0, drop_path_rate=0.1)
    cls = type(name, (MixVisionTransformer,), {'__init__': __init__, '__module__': __name__, '__qualname__': name})
    return BACKBONES.register_module()(cls)


_WIDE = (64, 128, 320, 512)
mit_b0 = _variant('mit_b0', (32, 64, 160, 256), (2, 2, 2, 2))
mit_b1 = _variant('mit_b1', _WIDE, (2, 2, 2, 2))
mit_b2 = _variant('mit_b2', _WIDE, (3, 4, 6, 3))
mit_b3 = _variant('mit_b3', _WIDE, (3, 4, 18, 3))
mit_b4 = _variant('mit_b4', _WIDE, (3, 8, 27, 3))
mit_b5 = _variant('mit_b5', _WIDE, (3, 6, 40, 3))
