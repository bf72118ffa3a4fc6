"""Torch-facing operators of the CFFM hot path: thin plumbing over the C ABI (include/cffm_hip.h).

PyTorch supplies device memory, the current HIP stream and autograd bookkeeping; all arithmetic of
the hot path happens inside libcffm_hip.so.  Tensors must be fp32, contiguous and on the GPU; a CPU
tensor raises (there is no CPU fallback -- the reference's CPU path is the oracle under oracle/,
which this package never imports).
"""
import contextlib
import ctypes as C
import weakref

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib, geometry

# field order of one block's parameters as the autograd function receives them (state_dict keys of
# CffmTransformerBlock3d3) -> (struct field, index inside an array field)
BLOCK_PARAM_KEYS = (
    ('norm1.weight', 'norm1_w', None), ('norm1.bias', 'norm1_b', None),
    ('pool_layers.0.weight', 'pool_w', 0), ('pool_layers.0.bias', 'pool_b', 0),
    ('pool_layers_clips.0.weight', 'pool_w', 1), ('pool_layers_clips.0.bias', 'pool_b', 1),
    ('pool_layers_clips.1.weight', 'pool_w', 2), ('pool_layers_clips.1.bias', 'pool_b', 2),
    ('pool_layers_clips.2.weight', 'pool_w', 3), ('pool_layers_clips.2.bias', 'pool_b', 3),
    ('attn.relative_position_bias_table', 'rpb_own', None),
    ('attn.relative_position_bias_table_to_neighbors', 'rpb_ring', None),
    ('attn.relative_position_bias_table_to_windows.0', 'rpb_pool', 0),
    ('attn.relative_position_bias_table_to_windows_clips.0', 'rpb_pool', 1),
    ('attn.relative_position_bias_table_to_windows_clips.1', 'rpb_pool', 2),
    ('attn.relative_position_bias_table_to_windows_clips.2', 'rpb_pool', 3),
    ('attn.qkv.weight', 'qkv_w', None), ('attn.qkv.bias', 'qkv_b', None),
    ('attn.proj.weight', 'proj_w', None), ('attn.proj.bias', 'proj_b', None),
    ('norm2.weight', 'norm2_w', None), ('norm2.bias', 'norm2_b', None),
    ('mlp.fc1.weight', 'fc1_w', None), ('mlp.fc1.bias', 'fc1_b', None),
    ('mlp.fc2.weight', 'fc2_w', None), ('mlp.fc2.bias', 'fc2_b', None),
)
NPB = len(BLOCK_PARAM_KEYS)   # tensors per block


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream(t):
    if t.is_cuda:
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return C.c_void_p(0)


@contextlib.contextmanager
def _branches(lib, st):
    """`with _branches(lib, st) as take:` -- stage calls side by side: entry marks this point of `st` (cffm_branch_mark), take(i) is library
    stream i (0..3) ordered behind the mark, the exit -- also when a stage call raises -- makes `st` continue behind every branch
    (cffm_branch_join).  The caller launches its own (longest) chain on `st` first and takes the branches afterwards: under stream capture the
    first-launched dependant of a node keeps the node's hardware queue.  A branch waits for the MARK only and the caching allocator knows nothing
    of these streams, so a region is prepare -> scope -> finish: whatever torch enqueues on `st` or allocates (.contiguous(), _to_rows, empty /
    zeros, zero_()) comes BEFORE the scope, inside are library calls only, and every tensor they touch stays referenced until it closes."""
    lib.cffm_branch_mark(st)
    try:
        yield lambda i: C.c_void_p(lib.cffm_branch_take(st, i))
    finally:
        lib.cffm_branch_join(st)


class _WGrad(C.Structure):
    """cffm_wgrad"""
    _fields_ = [('dy', C.c_void_p), ('x', C.c_void_p), ('dw', C.c_void_p), ('M', C.c_long), ('N', C.c_int), ('K', C.c_int)]


def _require_device(t, what):
    if _lib._override is None and not t.is_cuda:
        raise _lib.CffmError('%s: the CFFM hot path runs only on the GPU (got a %s tensor); there is no CPU '
                             'fallback' % (what, t.device))
    if t.dtype != torch.float32:
        raise _lib.CffmError('%s: fp32 expected, got %s' % (what, t.dtype))


def _require_int64(t, what):
    if _lib._override is None and not t.is_cuda:
        raise _lib.CffmError('%s: runs only on the GPU (got a %s tensor); there is no CPU fallback' % (what, t.device))
    if t.dtype != torch.int64:
        raise _lib.CffmError('%s: int64 expected, got %s' % (what, t.dtype))
    return t.contiguous()


_geom_cache = {}


def _checked_padded(lib, fn, *args):
    """A layer backward whose gradients are 16-byte-aligned slices of ONE flat buffer (_flat_grads): the library zeroes the padding behind
    the odd-sized ones itself (include/cffm_hip.h cffm_grad_slices_padded).  Switched on only around this call: a caller of the C ABI with
    gradient tensors of their own (tests/test_emu_kernels.py block API) must not have 3 floats written behind them."""
    lib.cffm_grad_slices_padded(1)
    try:
        _lib.check(fn(*args), lib)
    finally:
        lib.cffm_grad_slices_padded(0)


def make_geom(lib, b, h0, w0):
    key = (id(lib), b, h0, w0)
    g = _geom_cache.get(key)
    if g is None:
        g = _lib.Geom()
        _lib.check(lib.cffm_geom_init(C.byref(g), b, h0, w0), lib)
        _geom_cache[key] = g
    return g


_table_cache = {}


def device_tables(h0, w0, device):
    key = (h0, w0, str(device))
    if key not in _table_cache:
        ks, qd = geometry.tables(h0, w0)
        ip, ii = geometry.inverse_tables(h0, w0)
        _table_cache[key] = tuple(torch.from_numpy(np.array(a)).to(device) for a in (ks, qd, ip, ii))
    return _table_cache[key]


def block_ptrs(tensors):
    """26 tensors in BLOCK_PARAM_KEYS order -> a cffm_block_params / cffm_block_grads struct."""
    s = _lib.BlockPtrs()
    for t, (_, field, idx) in zip(tensors, BLOCK_PARAM_KEYS):
        if idx is None:
            setattr(s, field, t.data_ptr())
        else:
            getattr(s, field)[idx] = t.data_ptr()
    return s


_struct_cache = {}


def block_structs(tensors, depth):
    """(BlockPtrs * depth) for a flat tensor list; cached on the addresses (parameters do not move between steps)."""
    key = tuple(t.data_ptr() for t in tensors)
    st = _struct_cache.get(key)
    if st is None:
        if len(_struct_cache) > 64:
            _struct_cache.clear()
        st = (_lib.BlockPtrs * depth)(*[block_ptrs(tensors[i * NPB:(i + 1) * NPB]) for i in range(depth)])
        _struct_cache[key] = st
    return st


def block_ws_layout(lib, g):
    w = _lib.BlockWs()
    _lib.check(lib.cffm_block_ws_layout(C.byref(g), C.byref(w)), lib)
    return w


# Optional callable(block_index, flat_gradient_slice, depth), invoked by the layer's backward right after block `block_index`'s
# kernels have been enqueued on the current stream (blocks come last-to-first).  None: the whole backward is one library call.
block_grad_hook = None
# While a layer's backward hands its blocks to the hook: the parameter tensors of THAT layer (26 * depth, block-major).  A hook that
# serves several layers (one BlockwiseReducer for two CFFM layers) looks here to tell "this layer's .grad tensors exist already"
# (gradient accumulation: nothing may be exchanged block by block) from "another layer's backward has just adopted its gradients".
current_backward_params = None


def _check_stack(x):                # the layer's NCHW input: a clip stack [B,4,256,H,W]
    _require_device(x, 'cffm layer input')
    if x.dim() != 5 or x.shape[2] != 256:
        raise _lib.CffmError('expected x [B,T,256,H,W], got %s' % (tuple(x.shape),))
    if x.shape[1] != 4:
        raise IndexError('CFFM block needs T == 4 frames (3 reference + target), got T=%d' % x.shape[1])


def _check_rows(x_rows, h0, w0):    # the layer's input on token rows: [B,4,H*W,256]
    _require_device(x_rows, 'cffm layer input')
    if x_rows.dim() != 4 or x_rows.shape[1] != 4 or x_rows.shape[2] != h0 * w0 or x_rows.shape[3] != 256:
        raise _lib.CffmError('expected x_rows [B,4,%d,256], got %s' % (h0 * w0, tuple(x_rows.shape)))


def _layer_geom(lib, b, h0, w0, dev):       # -> geometry, (key_src, q_dst, inv_ptr, inv_idx) of a layer call
    return make_geom(lib, b, h0, w0), device_tables(h0, w0, dev)


def _layer_buffers(lib, g, depth, dev):     # -> `saved`, `scratch` of a forward that a backward follows
    return (torch.empty(lib.cffm_layer_saved_floats(C.byref(g), depth), dtype=torch.float32, device=dev),
            torch.empty(lib.cffm_layer_scratch_floats(C.byref(g)), dtype=torch.float32, device=dev))


def _flat_grads(params, dev, zero=False):
    """One allocation for every parameter gradient -> (flat, views of it shaped like `params`, floats per block): 16-byte aligned slices, block
    i's are flat[i * per_block:(i + 1) * per_block].  The <= 12-byte padding gaps between slices travel through the gradient all-reduce with
    them and must not carry NaN / Inf bit patterns of recycled memory: the library zeroes them inside the backward of the pooling Linears -- the
    only tensors with a gap behind them -- see cffm_grad_slices_padded in include/cffm_hip.h (a zero-fill of the whole 6.8 MB buffer was a 7 us
    kernel in front of the backward, an index_fill_ of the gaps a 4.7 us one).  `zero`: for slices read before their block's backward (LayerPieces)."""
    sizes = [(p.numel() + 3) // 4 * 4 for p in params]
    flat = (torch.zeros if zero else torch.empty)(sum(sizes), dtype=torch.float32, device=dev)
    grads = [c[:p.numel()].view(p.shape) if c.numel() != p.numel() else c.view(p.shape) for c, p in zip(flat.split(sizes), params)]
    return flat, grads, sum(sizes[:NPB])


class LayerPieces:
    """The layer's forward and backward as explicit pieces over STATIC buffers, without autograd: what a data-parallel training
    loop replays from HIP graphs when it wants the gradient exchange of block i to overlap the backward of block i - 1 --
    graph(forward + backward of the last blocks) | all-reduce(those blocks' gradient slices, asynchronous) | graph(backward of
    block 0) | all-reduce(block 0's slice) | graph(optimizer)  (bench.py, N > 1).  ``cffm_layer_forward`` / ``cffm_layer_backward_range``
    on the new target frame; ``grads`` are views of one flat buffer (``flat``), ``block_slice(i)`` is block i's part of it."""

    def __init__(self, x, depth, params):
        lib = _lib.get()
        _require_device(x, 'cffm layer input')
        if x.dim() != 5 or x.shape[1] != 4 or x.shape[2] != 256:
            raise _lib.CffmError('expected x [B,4,256,H,W], got %s' % (tuple(x.shape),))
        self.lib, self.x, self.depth, self.params = lib, x.contiguous(), depth, list(params)
        b, _, _, h0, w0 = x.shape
        dev = x.device
        self.g, self.tables = _layer_geom(lib, b, h0, w0, dev)
        self.saved, self.scratch = _layer_buffers(lib, self.g, depth, dev)
        self.y = torch.empty(b, 256, h0, w0, dtype=torch.float32, device=dev)
        self.dx = torch.empty(b, 4, 256, h0, w0, dtype=torch.float32, device=dev)
        self.flat, self.grads, self.per_block = _flat_grads(self.params, dev, zero=True)
        self.pstructs = block_structs(self.params, depth)
        self.gstructs = block_structs(self.grads, depth)

    def block_slice(self, i):
        return self.flat[i * self.per_block:(i + 1) * self.per_block]

    def forward(self):
        key_src, q_dst = self.tables[:2]
        _lib.check(self.lib.cffm_layer_forward(C.byref(self.g), self.depth, self.pstructs, _ptr(self.x), _ptr(self.y), _ptr(key_src),
                                               _ptr(q_dst), _ptr(self.saved), _ptr(self.scratch), _stream(self.x)), self.lib)
        return self.y

    def backward(self, dy, first_block, last_block):
        """blocks first_block .. last_block (descending) of the backward from dy [B,256,H,W] (a dense tensor or the last-frame
        slice of a [B,4,256,H,W] gradient)."""
        key_src, q_dst, inv_ptr, inv_idx = self.tables
        b, h0, w0 = self.x.shape[0], self.x.shape[3], self.x.shape[4]
        img = 256 * h0 * w0
        if not (dy.dim() == 4 and dy.stride()[1:] == (h0 * w0, w0, 1) and (b == 1 or dy.stride(0) >= img)):
            raise _lib.CffmError('LayerPieces.backward: dy must be dense inside a clip')
        dy_bs = dy.stride(0) if b > 1 else img
        _checked_padded(self.lib, self.lib.cffm_layer_backward_range, C.byref(self.g), self.depth, self.pstructs, self.gstructs, _ptr(dy), dy_bs,
                                                      _ptr(self.dx), _ptr(key_src), _ptr(q_dst), _ptr(inv_ptr), _ptr(inv_idx),
                                                      _ptr(self.saved), _ptr(self.scratch), first_block, last_block,
                                                      _stream(self.x))


class _LayerFullFn(torch.autograd.Function):
    """BasicLayer3d3.forward with the reference's whole output: x [B,4,256,H,W] -> [B,4,256,H,W] whose frames 0..2 are the input
    frames (cffm_transformer.py:826) and frame 3 is new.  The library writes the pass-through frames itself (side stream) and adds
    their upstream gradient into dx in its final layout pass, so neither torch.cat nor its backward (a zero-fill, a copy and an
    add over the 29 MB stack) runs around the call."""

    @staticmethod
    def forward(ctx, x, depth, *params):
        lib = _lib.get()
        _check_stack(x)
        assert len(params) == NPB * depth
        b, _, _, h0, w0 = x.shape
        x = x.contiguous()
        for p in params:
            if not p.is_contiguous() or p.dtype != torch.float32:
                raise _lib.CffmError('cffm layer parameters must be contiguous float32')
        g, (key_src, q_dst, inv_ptr, inv_idx) = _layer_geom(lib, b, h0, w0, x.device)
        saved, scratch = _layer_buffers(lib, g, depth, x.device)
        y = torch.empty(b, 4, 256, h0, w0, dtype=torch.float32, device=x.device)
        _lib.check(lib.cffm_layer_forward_full(C.byref(g), depth, block_structs(params, depth), _ptr(x), _ptr(y), _ptr(key_src), _ptr(q_dst),
                                               _ptr(saved), _ptr(scratch), _stream(x)), lib)
        ctx.depth, ctx.geom_args = depth, (b, h0, w0)
        ctx.save_for_backward(saved, key_src, q_dst, inv_ptr, inv_idx, *params)
        ctx.scratch = scratch
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.get()
        saved, key_src, q_dst, inv_ptr, inv_idx, *params = ctx.saved_tensors
        depth = ctx.depth
        b, h0, w0 = ctx.geom_args
        g = make_geom(lib, b, h0, w0)
        dy = dy.contiguous()
        flat, grads, per = _flat_grads(params, dy.device)              # torch.empty: the library zeroes the alignment gaps
        dx = torch.empty(b, 4, 256, h0, w0, dtype=torch.float32, device=dy.device)
        pstructs, gstructs = block_structs(params, depth), block_structs(grads, depth)
        hook = block_grad_hook
        global current_backward_params
        current_backward_params = params
        try:
            for first, last in ([(depth - 1, 0)] if hook is None else [(i, i) for i in range(depth - 1, -1, -1)]):
                _checked_padded(lib, lib.cffm_layer_backward_full, C.byref(g), depth, pstructs, gstructs, _ptr(dy), _ptr(dx), _ptr(key_src), _ptr(q_dst),
                                                        _ptr(inv_ptr), _ptr(inv_idx), _ptr(saved), _ptr(ctx.scratch), first, last,
                                                        _stream(dy))
                if hook is not None:
                    hook(first, flat[first * per:(first + 1) * per], depth)
        finally:
            current_backward_params = None
        return (dx, None) + tuple(grads)


def cffm_layer(x, depth, params):
    """x [B,4,256,H,W]; params: flat list of 26*depth tensors (BLOCK_PARAM_KEYS order per block).
    Returns the reference's output [B,4,256,H,W]: frames 0..2 are the input, frame 3 is new."""
    return _LayerFullFn.apply(x, depth, *params)


# ---------------------------------------------------------------------------------------------- NCHW <-> token rows
def _to_rows(lib, x):
    """[N,C,H,W] (any strides) -> contiguous token rows [N,H,W,C].  Plain NCHW goes through the library's tiled transpose,
    channels-last memory is already rows.  (The operators RETURN channels-last views: handing BatchNorm / ReLU / dropout plain
    NCHW instead made the whole head step slower, 5.3 -> 6.4 ms.)"""
    n, c, h, w = x.shape
    if x.is_contiguous() and x.numel() and c > 1 and h * w > 1:
        rows = torch.empty(n, h, w, c, dtype=torch.float32, device=x.device)
        _lib.check(lib.cffm_transpose(_ptr(x), _ptr(rows), n, c, h * w, c * h * w, c * h * w, _stream(x)), lib)
        return rows
    return x.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------- SegFormer embedding
def _segfuse_chains(lib, d, ca):
    """What _SegFuseFn.forward and segformer_fuse_pool share: operands checked, every scale embedded at its own resolution with its composed
    matrix -> (d, feats, mats, toks, zs, the three small maps' (pointers, heights, widths) as the C ABI takes them)."""
    k = len(ca) // 2
    feats, mats = ca[:k], [a.contiguous() for a in ca[k:]]
    if not 1 <= k <= 4:
        raise _lib.CffmError('segformer_fuse: 1..4 feature maps expected, got %d' % k)
    for c in feats + tuple(mats) + (d,):
        _require_device(c, 'segformer_fuse operand')
    n = feats[0].shape[0]
    st, dev = _stream(feats[0]), feats[0].device
    for c, a in zip(feats, mats):
        if c.dim() != 4 or c.shape[0] != n or a.shape != (256, c.shape[1]):
            raise _lib.CffmError('segformer_fuse: feature %s does not fit matrix %s' % (tuple(c.shape), tuple(a.shape)))
    # prepare: plain-NCHW copies of strided features (on the caller's stream: in front of the mark), token rows [N*h*w, C_i], products
    cs, d = [c.contiguous() for c in feats], d.contiguous()
    pix = [c.shape[2] * c.shape[3] for c in cs]
    toks = [torch.empty(n * p, c.shape[1], dtype=torch.float32, device=dev) for c, p in zip(cs, pix)]
    zs = [torch.empty(n * p, 256, dtype=torch.float32, device=dev) for p in pix]
    hs = (C.c_int * 3)(*([c.shape[2] for c in feats[1:]] + [1] * (4 - k)))
    ws = (C.c_int * 3)(*([c.shape[3] for c in feats[1:]] + [1] * (4 - k)))
    zp = (C.c_void_p * 3)(*([z.data_ptr() for z in zs[1:]] + [None] * (4 - k)))
    # every scale is an independent chain NCHW -> token rows -> Linear: the 1/4-scale one (three quarters of the bytes) on the caller's
    # stream, the others on branches beside it (one stream: 107 us of a replayed head step for 64 us of the largest chain)
    with _branches(lib, st) as take:
        for i, (c, a, t, z, p) in enumerate(zip(cs, mats, toks, zs, pix)):
            if n * p:
                ci = c.shape[1]
                s = take(i) if i else st
                _lib.check(lib.cffm_transpose(_ptr(c), _ptr(t), n, ci, p, ci * p, ci * p, s), lib)
                _lib.check(lib.cffm_linear_fwd(_ptr(t), _ptr(a), _ptr(z), n * p, 256, ci, s), lib)
    return d, feats, mats, toks, zs, (zp, hs, ws)


class _SegFuseFn(torch.autograd.Function):
    """sum_i resize_i(A_i c_i) + d on token rows: features c_i [N,C_i,h_i,w_i] (c_0 at the output resolution), composed
    matrices A_i [256,C_i], constant d [256] -> [N,256,H,W] (channels-last memory).  See csrc/segfuse_kernels.h."""

    @staticmethod
    def forward(ctx, d, *ca):
        lib = _lib.get()
        d, feats, mats, toks, zs, (zp, hs, ws) = _segfuse_chains(lib, d, ca)
        k = len(feats)
        n, _, H, W = feats[0].shape
        st = _stream(feats[0])
        y = zs[0]                                                             # updated in place: nothing else needs it
        if n * H * W:
            _lib.check(lib.cffm_segfuse_fwd(_ptr(y), _ptr(d), zp, hs, ws, k - 1, n, H, W, st), lib)
        ctx.save_for_backward(*toks, *mats)
        ctx.shapes = [tuple(c.shape) for c in feats]
        # channels-last memory: torch's BatchNorm runs faster on it than on plain NCHW (head step 4.6 vs 5.8 ms)
        return y.view(n, H, W, 256).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.get()
        shapes = ctx.shapes
        k = len(shapes)
        toks, mats = ctx.saved_tensors[:k], ctx.saved_tensors[k:]
        n, _, H, W = shapes[0]
        g = _to_rows(lib, g)                                                  # [N,H,W,256] rows
        st, dev = _stream(g), g.device
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        dd = new(256)
        rows = n * H * W
        dzs = [g.view(rows, 256)] + [new(n * s_[2] * s_[3], 256) for s_ in shapes[1:]]
        if k > 1 and rows:
            hs = (C.c_int * 3)(*([s_[2] for s_ in shapes[1:]] + [1] * (4 - k)))
            ws = (C.c_int * 3)(*([s_[3] for s_ in shapes[1:]] + [1] * (4 - k)))
            zp = (C.c_void_p * 3)(*([z.data_ptr() for z in dzs[1:]] + [None] * (4 - k)))
            _lib.check(lib.cffm_segfuse_bwd(_ptr(g), zp, hs, ws, k - 1, n, H, W, st), lib)
        # Behind the adjoint of the resizes everything is independent: branch 1 = the k weight gradients as ONE grouped launch and the
        # column sum of g (both use the library's scratch: one after the other on one branch); the input gradients (Linear + back to NCHW)
        # of the 1/4-scale map on the caller's stream, of the small maps on branches 2 / 3.  (One stream: 213 + 34 us of a replayed step.)
        # prepare: every result and temporary, zero-filled where no stage call will write it, and the weight-gradient groups
        pix = [s_[2] * s_[3] for s_ in shapes]
        dmats = [new(256, s_[1]) for s_ in shapes]
        live = [i for i in range(k) if n * pix[i]]
        for i in range(k):
            if i not in live:
                dmats[i].zero_()
        if not rows:
            dd.zero_()
        dts = [new(n * p, s_[1]) if ctx.needs_input_grad[1 + i] else None for i, (s_, p) in enumerate(zip(shapes, pix))]
        dfeats = [new(*s_) if ctx.needs_input_grad[1 + i] else None for i, s_ in enumerate(shapes)]
        # the weight gradients as the arguments of two grouped calls: the 1/4-scale map's | the other scales'
        groups = [[_WGrad(dzs[i].data_ptr(), toks[i].data_ptr(), dmats[i].data_ptr(), n * pix[i], 256, shapes[i][1]) for i in sel if i in live] for sel in ([0], range(1, k))]
        groups = [(_WGrad * len(q))(*q) for q in groups]

        def wgrads(pr, sx):
            if len(pr):
                _lib.check(lib.cffm_linear_bwd_weight_group(pr, len(pr), sx), lib)

        def dx_chain(i, sx):
            ci, p = shapes[i][1], pix[i]
            if dts[i] is not None and n * p:
                _lib.check(lib.cffm_linear_bwd_input(_ptr(dzs[i]), _ptr(mats[i]), _ptr(dts[i]), n * p, 256, ci, sx), lib)
                _lib.check(lib.cffm_transpose(_ptr(dts[i]), _ptr(dfeats[i]), n, p, ci, ci * p, ci * p, sx), lib)
        with _branches(lib, st) as take:
            dx_chain(0, st)                                        # the 1/4-scale chain first: it keeps the caller's stream (and its queue)
            if rows:
                # branch 1: the 1/4-scale weight gradient (three quarters of the rows); branch 2: the other scales' (one grouped call: the
                # library groups what its grouped kernel takes and runs the rest one by one) and the column sum of g; branch 3: the small
                # scales' input gradients.  (Weight gradients and column sums take their scratch from the branch's own pool.)
                wgrads(groups[0], take(1))
                s2 = take(2)
                _lib.check(lib.cffm_colsum(_ptr(g), rows, 256, _ptr(dd), s2), lib)
                wgrads(groups[1], s2)
            if k > 1:
                s3 = take(3)
                for i in range(1, k):
                    dx_chain(i, s3)
        return (dd,) + tuple(dfeats) + tuple(dmats)


def _ptr_array(ts):
    """host array of the tensors' device pointers (NULL for None)"""
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


class _ComposeFn(torch.autograd.Function):
    """(A_1 .. A_k, d): A_i = Wf_i W_i for every scale (Wf_i = the i-th [256,256] input-channel block of the fuse weight, cat order
    c_k..c_1, read in place through its leading dimension) and d = sum_i Wf_i b_i, as ONE library call per direction
    (cffm_fuse_compose_fwd / _bwd: the k products side by side on branches of the library's streams).  (As torch matmuls these
    70-MFLOP products and their backward took 0.4 ms per step; round 5 ran them as 4 + 8 stage GEMMs one behind the other with two
    layout copies of the fuse weight and torch's cat / gemv / ger for the constant: 97 + 120 us of a replayed head step.)"""

    @staticmethod
    def forward(ctx, fuse_w2d, *wb):
        lib = _lib.get()
        k, e = len(wb) // 2, fuse_w2d.shape[0]
        fuse_w2d = fuse_w2d.contiguous()
        lin_w, lin_b = [w.contiguous() for w in wb[:k]], [b_.contiguous() for b_ in wb[k:]]
        dev = fuse_w2d.device
        mats = [torch.empty(e, w.shape[1], dtype=torch.float32, device=dev) for w in lin_w]
        d = torch.empty(e, dtype=torch.float32, device=dev)
        cin = (C.c_int * k)(*[w.shape[1] for w in lin_w])
        _lib.check(lib.cffm_fuse_compose_fwd(_ptr(fuse_w2d), _ptr_array(lin_w), _ptr_array(lin_b), cin, k, e, _ptr_array(mats), _ptr(d),
                                             _stream(fuse_w2d)), lib)
        ctx.save_for_backward(fuse_w2d, *lin_w, *lin_b)
        return tuple(mats) + (d,)

    @staticmethod
    def backward(ctx, *grads):
        lib = _lib.get()
        fuse_w2d = ctx.saved_tensors[0]
        k = (len(ctx.saved_tensors) - 1) // 2
        lin_w, lin_b = ctx.saved_tensors[1:1 + k], ctx.saved_tensors[1 + k:]
        e, dev = fuse_w2d.shape[0], fuse_w2d.device
        dmats = [torch.zeros(e, w.shape[1], dtype=torch.float32, device=dev) if g is None else g.contiguous() for g, w in zip(grads[:k], lin_w)]
        dd = torch.zeros(e, dtype=torch.float32, device=dev) if grads[k] is None else grads[k].contiguous()
        dfw = torch.empty_like(fuse_w2d)
        dws, dbs = [torch.empty_like(w) for w in lin_w], [torch.empty_like(b_) for b_ in lin_b]
        cin = (C.c_int * k)(*[w.shape[1] for w in lin_w])
        _lib.check(lib.cffm_fuse_compose_bwd(_ptr(fuse_w2d), _ptr_array(lin_w), _ptr_array(lin_b), cin, k, e, _ptr_array(dmats), _ptr(dd), _ptr(dfw),
                                             _ptr_array(dws), _ptr_array(dbs), _stream(fuse_w2d)), lib)
        return (dfw,) + tuple(dws) + tuple(dbs)


def segformer_fuse(feats, lin_w, lin_b, fuse_w):
    """The SegFormer embedding of the CFFM heads without the 1024-channel concat (cffm_head.py:102-119):
    conv1x1(cat([resize(linear_c4(c4)), resize(linear_c3(c3)), resize(linear_c2(c2)), linear_c1(c1)]), fuse_w).

    feats: [c1, c2, c3, c4] NCHW (c1 = the 1/4-scale map the others are resized to); lin_w / lin_b: the four `MLP.proj`
    weights [256,C_i] / biases in the same order; fuse_w: `linear_fuse.conv.weight` [256, 4*256, 1, 1] whose input-channel
    blocks are ordered c4, c3, c2, c1 (the reference's cat order).  Returns the pre-BatchNorm map [N,256,H,W].
    The composed matrices Wf_i W_i and the constant sum_i Wf_i b_i come from one library call (_ComposeFn); autograd returns the
    gradients of the nine original tensors."""
    k = len(feats)
    e = fuse_w.shape[0]
    if e != 256 or fuse_w.shape[1] != k * e:
        raise _lib.CffmError('segformer_fuse: fuse weight %s does not fit %d embeddings of 256' % (tuple(fuse_w.shape), k))
    for w in lin_w:
        _require_device(w, 'segformer_fuse weight')
        if w.shape[0] != e or w.shape[1] % 4:
            raise _lib.CffmError('segformer_fuse: embedding weight %s (rows of 16-byte multiples expected)' % (tuple(w.shape),))
    for b_ in lin_b:
        _require_device(b_, 'segformer_fuse bias')
        if b_.shape != (e,):
            raise _lib.CffmError('segformer_fuse: embedding bias %s, [%d] expected' % (tuple(b_.shape), e))
    *mats, d = _ComposeFn.apply(fuse_w.reshape(e, k * e), *lin_w, *lin_b)
    return _SegFuseFn.apply(d, *feats, *mats)


def _check_ring(ring, slots, what):
    """a frame ring [R,B,rows,256] (fp32, contiguous) and its slot table (int32 [4], same device)"""
    _require_device(ring, what + ' ring')
    if ring.dim() != 4 or ring.shape[3] != 256 or ring.shape[0] < 1 or not ring.is_contiguous():
        raise _lib.CffmError('%s: a contiguous ring [R,B,rows,256] with R >= 1 expected, got %s' % (what, tuple(ring.shape)))
    if slots.dtype != torch.int32 or tuple(slots.shape) != (4,) or slots.device != ring.device or not slots.is_contiguous():
        raise _lib.CffmError('%s: the slot table is a contiguous int32 [4] on %s, got %s %s on %s'
                             % (what, ring.device, slots.dtype, tuple(slots.shape), slots.device))


def segformer_fuse_pool(feats, lin_w, lin_b, fuse_w, bn, ring, slots, which):
    """The eval tail of one frame (or of a batch of single frames) in one pass over the 1/4-scale map: what
    ``bn_relu_pool(segformer_fuse(feats, ...), bn)[1]`` returns -- the [B, H/2*W/2, 256] rows the CFFM layer reads, bit for bit -- written
    into ``ring[slots[which]]`` without the pre-BatchNorm map or ``fused`` ever existing (``cffm_segfuse_pool_fwd``).

    feats, lin_w, lin_b, fuse_w as for ``segformer_fuse``; ``bn`` must be in eval mode with running statistics; ``ring`` [R,B,H/2*W/2,256];
    ``slots`` a device int32 [4] the kernel reads (an entry outside 0..R-1 is clamped on the device); ``which`` in 0..3.  Inference only."""
    lib = _lib.get()
    if bn.training or bn.running_mean is None or bn.running_var is None:
        raise _lib.CffmError('segformer_fuse_pool is the eval tail: the BatchNorm must be in eval mode and have running statistics')
    _infer_only(list(feats) + list(lin_w) + list(lin_b) + [fuse_w, bn.weight, bn.bias], 'segformer_fuse_pool')
    _check_ring(ring, slots, 'segformer_fuse_pool')
    if not 0 <= int(which) < 4:
        raise _lib.CffmError('segformer_fuse_pool: `which` indexes the 4-entry slot table, got %r' % (which,))
    k, e = len(feats), fuse_w.shape[0]
    if e != 256 or fuse_w.shape[1] != k * e:
        raise _lib.CffmError('segformer_fuse_pool: fuse weight %s does not fit %d embeddings of 256' % (tuple(fuse_w.shape), k))
    n, _, H, W = feats[0].shape
    if H % 2 or W % 2 or tuple(ring.shape[1:]) != (n, (H // 2) * (W // 2), 256):
        raise _lib.CffmError('segformer_fuse_pool: a [%d,*,%d,%d] map (even sides) does not fit ring slots %s'
                             % (n, H, W, tuple(ring.shape[1:])))
    with torch.no_grad():
        *mats, d = _ComposeFn.apply(fuse_w.detach().reshape(e, k * e), *[w.detach() for w in lin_w], *[b_.detach() for b_ in lin_b])
        d, feats, mats, _toks, zs, (zp, hs, ws) = _segfuse_chains(lib, d, tuple(f.detach() for f in feats) + tuple(mats))
        st, dev = _stream(ring), ring.device
        coef = torch.empty(4, 256, dtype=torch.float32, device=dev)
        w_, b_ = bn.weight.detach().contiguous(), bn.bias.detach().contiguous()
        _lib.check(lib.cffm_bn_finalize_fwd(None, 0, float(n * H * W), _ptr(w_), _ptr(b_), _ptr(bn.running_mean), _ptr(bn.running_var), 0.0,
                                            float(bn.eps), _ptr(coef), st), lib)
        slot_floats = ring.shape[1] * ring.shape[2] * 256
        _lib.check(lib.cffm_segfuse_pool_fwd(_ptr(zs[0]), _ptr(d), zp, hs, ws, k - 1, _ptr(coef[0]), _ptr(coef[1]), _ptr(ring), slot_floats,
                                             ring.shape[0], _ptr(slots), int(which), n, H, W, st), lib)
    return ring


def _check_frame_ring(ring, table, shape, what):
    """a ring of single frames [R,rows,256] (fp32, contiguous) and a device table of slot numbers (int32, contiguous, `shape` with None =
    any size >= 1, same device)"""
    _require_device(ring, what + ' ring')
    if ring.dim() != 3 or ring.shape[2] != 256 or ring.shape[0] < 1 or not ring.is_contiguous():
        raise _lib.CffmError('%s: a contiguous ring [R,rows,256] with R >= 1 expected, got %s' % (what, tuple(ring.shape)))
    fits = table.dim() == len(shape) and table.shape[0] >= 1 and all(s is None or s == t for s, t in zip(shape, table.shape))
    if table.dtype != torch.int32 or not fits or table.device != ring.device or not table.is_contiguous():
        raise _lib.CffmError('%s: the slot table is a contiguous int32 %s on %s, got %s %s on %s'
                             % (what, list(shape), ring.device, table.dtype, tuple(table.shape), table.device))


def segformer_fuse_pool_frames(feats, lin_w, lin_b, fuse_w, bn, ring, slots):
    """``segformer_fuse_pool`` on N frames of ONE video with a slot per frame: frame n's [H/2*W/2, 256] rows are written into
    ``ring[slots[n]]`` (``cffm_segfuse_pool_fwd_frames``, one launch), with the bits N calls of ``segformer_fuse_pool`` at N = 1 leave.

    feats, lin_w, lin_b, fuse_w as for ``segformer_fuse``; ``bn`` in eval mode with running statistics; ``ring`` [R,H/2*W/2,256];
    ``slots`` a device int32 [N] the kernel reads (an entry outside 0..R-1 is clamped on the device; two frames naming one slot leave an
    unspecified mix there).  Inference only."""
    lib = _lib.get()
    if bn.training or bn.running_mean is None or bn.running_var is None:
        raise _lib.CffmError('segformer_fuse_pool_frames is the eval tail: the BatchNorm must be in eval mode and have running statistics')
    _infer_only(list(feats) + list(lin_w) + list(lin_b) + [fuse_w, bn.weight, bn.bias], 'segformer_fuse_pool_frames')
    n, _, H, W = feats[0].shape
    _check_frame_ring(ring, slots, (n,), 'segformer_fuse_pool_frames')
    k, e = len(feats), fuse_w.shape[0]
    if e != 256 or fuse_w.shape[1] != k * e:
        raise _lib.CffmError('segformer_fuse_pool_frames: fuse weight %s does not fit %d embeddings of 256' % (tuple(fuse_w.shape), k))
    if H % 2 or W % 2 or tuple(ring.shape[1:]) != ((H // 2) * (W // 2), 256):
        raise _lib.CffmError('segformer_fuse_pool_frames: a [%d,*,%d,%d] map (even sides) does not fit ring slots %s'
                             % (n, H, W, tuple(ring.shape[1:])))
    with torch.no_grad():
        *mats, d = _ComposeFn.apply(fuse_w.detach().reshape(e, k * e), *[w.detach() for w in lin_w], *[b_.detach() for b_ in lin_b])
        d, feats, mats, _toks, zs, (zp, hs, ws) = _segfuse_chains(lib, d, tuple(f.detach() for f in feats) + tuple(mats))
        st, dev = _stream(ring), ring.device
        coef = torch.empty(4, 256, dtype=torch.float32, device=dev)
        w_, b_ = bn.weight.detach().contiguous(), bn.bias.detach().contiguous()
        _lib.check(lib.cffm_bn_finalize_fwd(None, 0, float(n * H * W), _ptr(w_), _ptr(b_), _ptr(bn.running_mean), _ptr(bn.running_var), 0.0,
                                            float(bn.eps), _ptr(coef), st), lib)
        _lib.check(lib.cffm_segfuse_pool_fwd_frames(_ptr(zs[0]), _ptr(d), zp, hs, ws, k - 1, _ptr(coef[0]), _ptr(coef[1]), _ptr(ring),
                                                    ring.shape[1] * 256, ring.shape[0], _ptr(slots), n, H, W, st), lib)
    return ring


# ---------------------------------------------------------------------------------------------- 1x1 classifiers
class _Conv1x1Fn(torch.autograd.Function):
    """A 1x1 convolution as a Linear GEMM on channels-last token rows: x [N,C,H,W] (any strides; channels-last costs no copy),
    weight [O,C,1,1], bias [O] -> [N,O,H,W] in channels-last memory -- or, with `clips` = B, the same rows viewed as
    [B, N/B, O, H, W] (the head's per-frame logits): the gradient of that view may then arrive as B separately-placed blocks of
    rows (slices of a [B, T+1, H, W, O] buffer, the loss kernel's output) and is consumed block by block, not copied together."""

    @staticmethod
    def forward(ctx, x, weight, bias, clips, extra=0):
        lib = _lib.get()
        for t in (x, weight, bias):
            _require_device(t, 'conv1x1 operand')
        if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[1:]) != (x.shape[1], 1, 1) or bias.shape != (weight.shape[0],):
            raise _lib.CffmError('conv1x1: x %s, weight %s, bias %s do not fit a 1x1 convolution'
                                 % (tuple(x.shape), tuple(weight.shape), tuple(bias.shape)))
        n, c, h, w = x.shape
        o = weight.shape[0]
        if c % 4 or o % 4:
            raise _lib.CffmError('conv1x1: channel counts must be multiples of 4 (16-byte token rows), got %d -> %d' % (c, o))
        if clips and n % clips:
            raise _lib.CffmError('conv1x1: %d maps do not split into %d clips' % (n, clips))
        rows = _to_rows(lib, x)                                   # [N,H,W,C] token rows
        wm, b = weight.reshape(o, c).contiguous(), bias.contiguous()
        ctx.save_for_backward(rows, wm)
        ctx.x_plain = x.is_contiguous()            # hand the input gradient back in the input's own memory layout
        ctx.clips = clips
        if clips and extra:
            # room for `extra` more maps per clip behind the n / clips this call writes (cat_into fills them): the head's [B, T+1, K, h, w]
            # logits are then assembled where they lie -- torch.cat copied the 57 MB of frame logits once more (30 us of a replayed step)
            t = n // clips
            buf = torch.empty(clips, t + extra, h, w, o, dtype=torch.float32, device=x.device)
            per = t * h * w
            for i in range(clips):
                if per:
                    _lib.check(lib.cffm_linear_bias_fwd(C.c_void_p(rows.data_ptr() + 4 * i * per * c), _ptr(wm), _ptr(b), _ptr(buf[i]), per, o, c, _stream(x)), lib)
            return buf[:, :t].permute(0, 1, 4, 2, 3)
        y = torch.empty(n, h, w, o, dtype=torch.float32, device=x.device)
        _lib.check(lib.cffm_linear_bias_fwd(_ptr(rows), _ptr(wm), _ptr(b), _ptr(y), n * h * w, o, c, _stream(x)), lib)
        if clips:
            return y.view(clips, n // clips, h, w, o).permute(0, 1, 4, 2, 3)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.get()
        rows, wm = ctx.saved_tensors
        n, h, w, c = rows.shape
        o = wm.shape[0]
        m, st = n * h * w, _stream(rows)
        # the gradient as blocks of token rows: [(rows tensor, first row, row count)]
        blocks = None
        if ctx.clips:
            d5 = dy.permute(0, 1, 3, 4, 2)                                   # [B,T,H,W,O]
            if d5.is_contiguous():
                blocks = [(d5, 0, m)]
            elif all(d5[i].is_contiguous() for i in range(ctx.clips)):
                per = m // ctx.clips
                blocks = [(d5[i], i * per, per) for i in range(ctx.clips)]
            else:
                dy = dy.reshape(n, o, h, w)
        if blocks is None:
            blocks = [(_to_rows(lib, dy.reshape(n, o, h, w) if dy.dim() == 5 else dy), 0, m)]
        dx = dwm = db = None
        live = [(blk, r0, nr) for blk, r0, nr in blocks if nr]
        # prepare: the input gradient on rows (and in plain NCHW for a plain input), one weight / bias partial per block of rows
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dy.device)
        dxr = new(n, h, w, c) if ctx.needs_input_grad[0] else None
        dxp = new(n, c, h, w) if (dxr is not None and ctx.x_plain and m) else None
        wparts = [new(o, c) for _ in live] if ctx.needs_input_grad[1] else []
        bparts = [new(o) for _ in live] if ctx.needs_input_grad[2] else []
        # the input gradient on the caller's stream; beside it the weight gradient of block j on branch 1 + j % 2 and the column sums on
        # branch 3 (both use the library's scratch: each from the pool of its branch)
        with _branches(lib, st) as take:
            if dxr is not None:
                for blk, r0, nr in live:
                    _lib.check(lib.cffm_linear_bwd_input(_ptr(blk), _ptr(wm), C.c_void_p(dxr.data_ptr() + 4 * r0 * c), nr, o, c, st), lib)
                if dxp is not None:
                    _lib.check(lib.cffm_transpose(_ptr(dxr), _ptr(dxp), n, h * w, c, c * h * w, c * h * w, st), lib)
            if wparts:
                sw = [take(1), take(2)] if len(live) > 1 else [take(1)]
                for j, ((blk, r0, nr), t) in enumerate(zip(live, wparts)):
                    _lib.check(lib.cffm_linear_bwd_weight(_ptr(blk), C.c_void_p(rows.data_ptr() + 4 * r0 * c), _ptr(t), nr, o, c, sw[j % len(sw)]), lib)
            if bparts:
                sb = take(3)
                for (blk, r0, nr), t in zip(live, bparts):
                    _lib.check(lib.cffm_colsum(_ptr(blk), nr, o, _ptr(t), sb), lib)
        if dxr is not None:                        # (dxr, the transpose's source, stays referenced behind the join)
            dx = dxp if dxp is not None else dxr.permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:
            dwm = wparts[0] if wparts else torch.zeros(o, c, dtype=torch.float32, device=dy.device)
            for t in wparts[1:]:
                dwm += t
            dwm = dwm.view(o, c, 1, 1)
        if ctx.needs_input_grad[2]:
            db = bparts[0] if bparts else torch.zeros(o, dtype=torch.float32, device=dy.device)
            for t in bparts[1:]:
                db += t
        return dx, dwm, db, None, None


def conv1x1(x, weight, bias, clips=0, extra=0):
    """nn.Conv2d(C, O, kernel_size=1)(x) (the head's classifiers `linear_pred*`, cffm_head.py:121,147,524) as a split-bf16 MFMA
    GEMM on token rows; returns [N,O,H,W] in channels-last memory, or [clips, N/clips, O, H, W] (same memory) when `clips` is given.
    `extra` (with `clips`): the rows are written into a [clips, N/clips + extra, H, W, O] buffer, so that `cat_into` can append the clip-level
    maps (cffm_head.py:150 `torch.cat([x, x2], 1)`) without copying these."""
    y = _Conv1x1Fn.apply(x, weight, bias, int(clips), int(extra))
    if clips and extra:
        _ROOMS[y.untyped_storage()] = (y.storage_offset(), y.shape, y.stride(), int(extra))
    return y


# storage of a conv1x1(..., clips, extra=e) buffer whose room is still free -> (offset, shape, strides of its front view, e).  Keyed weakly on
# the storage object (one per buffer, whichever tensor asks for it): an entry neither keeps its buffer alive nor outlives it.
_ROOMS = weakref.WeakKeyDictionary()


class _CatIntoFn(torch.autograd.Function):
    """torch.cat([x, x2], 1) of logits maps that live as token rows, where x = buf[:, :T] is the front of a [B, T+e, h, w, K] buffer
    (conv1x1(..., extra=e)): only x2 is copied; the result is the whole buffer viewed as [B, T+e, K, h, w].  Backward: two views."""

    @staticmethod
    def forward(ctx, x, x2):
        t, e = x.shape[1], x2.shape[1]
        rows = x.permute(0, 1, 3, 4, 2)                                   # [B, T, h, w, K]: contiguous slices of the buffer
        buf = torch.as_strided(rows, (x.shape[0], t + e, rows.shape[2], rows.shape[3], rows.shape[4]), rows.stride(), rows.storage_offset())
        buf[:, t:].copy_(x2.permute(0, 1, 3, 4, 2))
        ctx.t = t
        return buf.permute(0, 1, 4, 2, 3)

    @staticmethod
    def backward(ctx, g):
        return g[:, :ctx.t], g[:, ctx.t:]


_DEFERRED = []         # tensors the deferred branch (cffm_defer_begin) still touches; cleared by _join_deferred


def _join_deferred():
    """the caller's stream continues behind the deferred branch (no-op when nothing is pending): called by whoever consumes deferred results
    (bn_relu_pool's backward) and once more at the end of every backward pass that deferred something"""
    if _DEFERRED:
        lib = _lib.get()
        lib.cffm_defer_join(_stream(_DEFERRED[0][0]))
        del _DEFERRED[:]


@contextlib.contextmanager
def _deferred(lib, st, keep):
    """`with _deferred(lib, st, keep) as sd:` (inside a backward pass) -- stage calls on the library's deferred stream sd, ordered behind `st` as
    it stands (cffm_defer_begin).  No join on exit: `st` continues at once, whoever reads the results calls _join_deferred() first, and the end of
    the backward pass joins in any case.  `keep` -- every tensor the stage calls touch, allocated BEFORE the scope as for _branches -- is registered
    before the first stage call and released by the join; when a stage call raises, the join happens here.  The end-of-pass callback is queued every
    time (joining nothing is a no-op): a pass that died after deferring never ran its own, and the next join -- at the latest the end of the next pass that defers -- releases what it left."""
    sd = C.c_void_p(lib.cffm_defer_begin(st))
    if sd.value != st.value:
        _DEFERRED.append(keep)
        torch.autograd.Variable._execution_engine.queue_callback(_join_deferred)
    try:
        yield sd
    except BaseException:
        if sd.value != st.value:
            _join_deferred()
        raise


class _LateGradFn(torch.autograd.Function):
    """Identity on parameters whose gradients will come from the deferred branch.  Autograd accumulates a parameter gradient (and may CLONE
    it) the moment the producing node returns -- for a gradient still being computed on another stream that is a race (found by
    tests/test_headfuse.py::test_head_step_replayed_equals_eager_gpu: linear_pred.bias.grad was a copy of stale memory).  Applied EARLY in the
    forward, this node runs LATE in the backward (the engine takes ready nodes in reverse creation order); it joins the deferred branch and
    hands the gradients on, so whatever autograd does with them happens behind the join."""

    @staticmethod
    def forward(ctx, *ps):
        return tuple(p.view_as(p) for p in ps)

    @staticmethod
    def backward(ctx, *gs):
        _join_deferred()
        return gs


def late_params(*ps):
    return _LateGradFn.apply(*ps)


class _FrameLogitsCatFn(torch.autograd.Function):
    """torch.cat([linear_pred(fused) viewed [B,T,K,h,w], x2], 1) (cffm_head.py:121 + :150) as ONE node, created LAST in the forward -- so it
    is the FIRST node of the backward, and the classifier's backward (input gradient: needed by linear_fuse's BatchNorm backward; weight /
    bias gradients: needed by the optimizer) goes to the library's deferred branch and runs BESIDE the clip-level path's and the whole CFFM
    layer's backward instead of behind them (110 us of a replayed head step).  The returned input gradient must not be read on the caller's
    stream before _join_deferred(): ops.bn_relu_pool's backward -- its only consumer on the heads' rows path -- joins first, and the end of
    the backward pass joins in any case.  `weight` / `bias` must come through ops.late_params (their gradients are deferred too)."""

    @staticmethod
    def forward(ctx, fused, weight, bias, x2, clips):
        lib = _lib.get()
        for t in (fused, weight, bias, x2):
            _require_device(t, 'frame_logits_cat operand')
        n, c, h, w = fused.shape
        o = weight.shape[0]
        if weight.dim() != 4 or tuple(weight.shape[1:]) != (c, 1, 1) or bias.shape != (o,) or c % 4 or o % 4 or n % clips:
            raise _lib.CffmError('frame_logits_cat: fused %s, weight %s, bias %s, %d clips do not fit' % (tuple(fused.shape), tuple(weight.shape), tuple(bias.shape), clips))
        t = n // clips
        e = x2.shape[1]
        if x2.shape != (clips, e, o, h, w):
            raise _lib.CffmError('frame_logits_cat: clip-level maps %s, [%d, e, %d, %d, %d] expected' % (tuple(x2.shape), clips, o, h, w))
        rows = _to_rows(lib, fused)
        wm, b = weight.reshape(o, c).contiguous(), bias.contiguous()
        buf = torch.empty(clips, t + e, h, w, o, dtype=torch.float32, device=fused.device)
        per, st = t * h * w, _stream(fused)
        for i in range(clips):
            if per:
                _lib.check(lib.cffm_linear_bias_fwd(C.c_void_p(rows.data_ptr() + 4 * i * per * c), _ptr(wm), _ptr(b), _ptr(buf[i]), per, o, c, st), lib)
        buf[:, t:].copy_(x2.permute(0, 1, 3, 4, 2))
        ctx.save_for_backward(rows, wm)
        ctx.dims = (clips, t, e)
        ctx.x_plain = fused.is_contiguous()
        return buf.permute(0, 1, 4, 2, 3)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.get()
        rows, wm = ctx.saved_tensors
        clips, t, e = ctx.dims
        n, h, w, c = rows.shape
        o = wm.shape[0]
        g5 = g.permute(0, 1, 3, 4, 2)                                      # [B, T+e, h, w, K] as the loss kernel wrote it
        if not all(g5[i].is_contiguous() for i in range(clips)):
            g5 = g5.contiguous()
        per, st, dev = t * h * w, _stream(rows), rows.device
        # prepare: the results (zero where no stage call will write them), one partial per further clip, the plain-NCHW input gradient
        new = torch.empty if per else torch.zeros
        dx = torch.empty(n, h, w, c, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dwm = new(o, c, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        db = new(o, dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
        tws = [dwm] + [torch.empty_like(dwm) for _ in range(1, clips)] if (dwm is not None and per) else []
        tbs = [db] + [torch.empty_like(db) for _ in range(1, clips)] if (db is not None and per) else []
        dxp = torch.empty(n, c, h, w, dtype=torch.float32, device=dev) if (dx is not None and ctx.x_plain and per) else None
        if per:
            blk = [g5[i, :t] for i in range(clips)]
            with _deferred(lib, st, [rows, wm, g5, dx] + tws + tbs) as sd:
                if dx is not None:
                    for i in range(clips):
                        _lib.check(lib.cffm_linear_bwd_input(_ptr(blk[i]), _ptr(wm), C.c_void_p(dx.data_ptr() + 4 * i * per * c), per, o, c, sd), lib)
                for i in range(clips):
                    xi = C.c_void_p(rows.data_ptr() + 4 * i * per * c)
                    if tws:
                        _lib.check(lib.cffm_linear_bwd_weight(_ptr(blk[i]), xi, _ptr(tws[i]), per, o, c, sd), lib)
                        if i:
                            _lib.check(lib.cffm_add_inplace(_ptr(dwm), _ptr(tws[i]), o * c, sd), lib)
                    if tbs:
                        _lib.check(lib.cffm_colsum(_ptr(blk[i]), per, o, _ptr(tbs[i]), sd), lib)
                        if i:
                            _lib.check(lib.cffm_add_inplace(_ptr(db), _ptr(tbs[i]), o, sd), lib)
        dfused = dx.permute(0, 3, 1, 2) if dx is not None else None
        if dxp is not None:                             # (plain NCHW input: the heads' rows path hands channels-last memory, this is the general case)
            _join_deferred()
            _lib.check(lib.cffm_transpose(_ptr(dx), _ptr(dxp), n, h * w, c, c * h * w, c * h * w, st), lib)
            dfused = dxp
        return dfused, (dwm.view(o, c, 1, 1) if dwm is not None else None), db, g[:, t:], None


def frame_logits_cat(fused, weight, bias, x2, clips):
    """[B, T+e, K, h, w] = cat([conv1x1(fused) per clip, x2], 1): see _FrameLogitsCatFn (o % 4 == 0 and c % 4 == 0 as for conv1x1)"""
    return _FrameLogitsCatFn.apply(fused, weight, bias, x2, int(clips))


def cat_room(x, extra):
    """True when x is what conv1x1(..., clips=B, extra=e) handed out -- the front [B,T,K,h,w] of a [B,T+e,h,w,K] buffer -- or an alias of it
    (detach(): same buffer, offset, shape and strides), with `extra` <= e and the room not yet filled.  By the buffer's entry in _ROOMS, not by
    strides alone: a [:, :T] slice of any rows buffer has the same strides with live data behind it.  Everything else is torch.cat's job."""
    room = _ROOMS.get(x.untyped_storage())
    return room is not None and room[:3] == (x.storage_offset(), x.shape, x.stride()) and 0 < extra <= room[3]


def cat_into(x, x2):
    """torch.cat([x, x2], 1) into the room behind x (cat_room(x, x2.shape[1]) must hold); fills the room, so its entry goes"""
    if x2.dim() != 5 or not cat_room(x, x2.shape[1]) or x2.shape[0] != x.shape[0] or x2.shape[2:] != x.shape[2:]:
        raise _lib.CffmError('cat_into: no room for %s behind %s (ops.cat_room)' % (tuple(x2.shape), tuple(x.shape)))
    del _ROOMS[x.untyped_storage()]
    return _CatIntoFn.apply(x, x2)


# ---------------------------------------------------------------------------------------------- the layer on token rows
class _LayerRowsFn(torch.autograd.Function):
    """BasicLayer3d3 on channels-last token rows: x_rows [B,4,H*W,256] -> the new target frame [B,H*W,256].  Same kernels as
    _LayerFullFn without the four NCHW <-> NHWC transposes (the heads' neighbours of the hot path work on rows too)."""

    @staticmethod
    def forward(ctx, x_rows, h0, w0, depth, *params):
        lib = _lib.get()
        _check_rows(x_rows, h0, w0)
        assert len(params) == NPB * depth
        x_rows = x_rows.contiguous()
        b = x_rows.shape[0]
        g, (key_src, q_dst, inv_ptr, inv_idx) = _layer_geom(lib, b, h0, w0, x_rows.device)
        saved, scratch = _layer_buffers(lib, g, depth, x_rows.device)
        y = torch.empty(b, h0 * w0, 256, dtype=torch.float32, device=x_rows.device)
        _lib.check(lib.cffm_layer_forward_rows(C.byref(g), depth, block_structs(params, depth), _ptr(x_rows), _ptr(y), _ptr(key_src),
                                               _ptr(q_dst), _ptr(saved), _ptr(scratch), _stream(x_rows)), lib)
        ctx.depth, ctx.geom_args = depth, (b, h0, w0)
        ctx.save_for_backward(x_rows, saved, key_src, q_dst, inv_ptr, inv_idx, *params)
        ctx.scratch = scratch
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.get()
        x_rows, saved, key_src, q_dst, inv_ptr, inv_idx, *params = ctx.saved_tensors
        depth = ctx.depth
        b, h0, w0 = ctx.geom_args
        g = make_geom(lib, b, h0, w0)
        dy = dy.contiguous()
        _, grads, _ = _flat_grads(params, dy.device)                   # torch.empty: the library zeroes the alignment gaps
        dx = torch.empty(b, 4, h0 * w0, 256, dtype=torch.float32, device=dy.device)
        _checked_padded(lib, lib.cffm_layer_backward_rows, C.byref(g), depth, block_structs(params, depth), block_structs(grads, depth), _ptr(x_rows),
                                                _ptr(dy), _ptr(dx), _ptr(key_src), _ptr(q_dst), _ptr(inv_ptr), _ptr(inv_idx), _ptr(saved),
                                                _ptr(ctx.scratch), _stream(dy))
        return (dx, None, None, None) + tuple(grads)


def cffm_layer_rows(x_rows, h0, w0, depth, params):
    """x_rows [B,4,H*W,256] (frame-major clip stack, channels-last) -> [B,H*W,256]: the new target frame of the reference's
    BasicLayer3d3 output (frames 0..2 of that output are the input frames)."""
    return _LayerRowsFn.apply(x_rows, h0, w0, depth, *params)


# ---------------------------------------------------------------------------------------------- the layer without a backward
# The inference forward (include/cffm_hip.h, ABI 12): plain functions, nothing recorded, nothing saved.  Same kernels in store-free
# instantiations -- the result equals cffm_layer / cffm_layer_rows bit for bit.  `prepared` holds what depends on the parameters
# alone (layer_prepare); the caller rebuilds it whenever a parameter changes (BasicLayer3d3 keeps one per module, modules.py).
def _check_layer_params(params, depth):
    if len(params) != NPB * depth:
        raise _lib.CffmError('expected %d parameter tensors for depth %d, got %d' % (NPB * depth, depth, len(params)))
    for p in params:
        _require_device(p, 'cffm layer parameter')
        if not p.is_contiguous():
            raise _lib.CffmError('cffm layer parameters must be contiguous float32')


def layer_prepare(depth, params):
    """The parameter-only inputs of the inference forward for these 26 * depth tensors: per block the position-bias fragments, the
    pooling matrix and the forward-form fragment-ordered Linear weights, in one tensor (``cffm_layer_prepare``)."""
    lib = _lib.get()
    _check_layer_params(params, depth)
    dev = params[0].device
    prepared = torch.empty(lib.cffm_layer_prepared_floats(depth), dtype=torch.float32, device=dev)
    _lib.check(lib.cffm_layer_prepare(depth, block_structs(params, depth), _ptr(prepared), _stream(prepared)), lib)
    return prepared


def _infer_buffers(lib, g, depth, prepared, ws, out, out_shape, dev):
    if prepared.dtype != torch.float32 or prepared.numel() < lib.cffm_layer_prepared_floats(depth) or prepared.device != dev:
        raise _lib.CffmError('`prepared` does not belong to a layer of depth %d on %s (ops.layer_prepare)' % (depth, dev))
    need = lib.cffm_layer_infer_ws_floats(C.byref(g))
    if ws is None:
        ws = torch.empty(need, dtype=torch.float32, device=dev)
    elif ws.dtype != torch.float32 or ws.numel() < need or ws.device != dev or not ws.is_contiguous():
        raise _lib.CffmError('inference workspace: %d contiguous fp32 values on %s expected' % (need, dev))
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != tuple(out_shape) or out.device != dev or not out.is_contiguous():
        raise _lib.CffmError('inference output: contiguous fp32 %s on %s expected' % (tuple(out_shape), dev))
    return ws, out


def cffm_layer_infer(x, depth, params, prepared, ws=None, out=None):
    """cffm_layer without autograd: x [B,4,256,H,W] -> [B,4,256,H,W] (frames 0..2 are the input frames).  ``ws`` / ``out``: optional
    caller-owned workspace (``cffm_layer_infer_ws_floats`` floats) and result tensor, e.g. static buffers of a captured graph."""
    lib = _lib.get()
    _check_stack(x)
    if len(params) != NPB * depth:         # (dtype / device / contiguity were checked when `prepared` was built from them)
        raise _lib.CffmError('expected %d parameter tensors for depth %d, got %d' % (NPB * depth, depth, len(params)))
    b, _, _, h0, w0 = x.shape
    x = x.detach().contiguous()
    g, (key_src, q_dst, *_) = _layer_geom(lib, b, h0, w0, x.device)
    ws, out = _infer_buffers(lib, g, depth, prepared, ws, out, (b, 4, 256, h0, w0), x.device)
    _lib.check(lib.cffm_layer_infer_full(C.byref(g), depth, block_structs(params, depth), _ptr(prepared), _ptr(x), _ptr(out), _ptr(key_src),
                                         _ptr(q_dst), _ptr(ws), _stream(x)), lib)
    return out


def cffm_layer_rows_infer(x_rows, h0, w0, depth, params, prepared, ws=None, out=None):
    """cffm_layer_rows without autograd: x_rows [B,4,H*W,256] -> the new target frame [B,H*W,256]."""
    lib = _lib.get()
    _check_rows(x_rows, h0, w0)
    if len(params) != NPB * depth:
        raise _lib.CffmError('expected %d parameter tensors for depth %d, got %d' % (NPB * depth, depth, len(params)))
    x_rows = x_rows.detach().contiguous()
    b = x_rows.shape[0]
    g, (key_src, q_dst, *_) = _layer_geom(lib, b, h0, w0, x_rows.device)
    ws, out = _infer_buffers(lib, g, depth, prepared, ws, out, (b, h0 * w0, 256), x_rows.device)
    _lib.check(lib.cffm_layer_infer_rows(C.byref(g), depth, block_structs(params, depth), _ptr(prepared), _ptr(x_rows), _ptr(out), _ptr(key_src),
                                         _ptr(q_dst), _ptr(ws), _stream(x_rows)), lib)
    return out


def cffm_layer_rows_ring(ring, slots, h0, w0, depth, params, prepared, ws=None, out=None):
    """cffm_layer_rows_infer on four frames where a ring holds them: ring [R,B,h0*w0,256], frame t (the target last) = ring[slots[t]],
    slots a device int32 [4] the kernels read (entries may repeat; one outside 0..R-1 is clamped on the device) -> the new target frame
    [B,h0*w0,256].  Equal, bit for bit, to cffm_layer_rows_infer on ``ring.index_select(0, slots).transpose(0, 1)``.  No argument of the
    library call depends on the table's contents: captured once, the call serves every frame of a video."""
    lib = _lib.get()
    _check_ring(ring, slots, 'cffm_layer_rows_ring')
    if ring.shape[2] != h0 * w0:
        raise _lib.CffmError('cffm_layer_rows_ring: ring slots [B,%d,256] expected, got %s' % (h0 * w0, tuple(ring.shape[1:])))
    if len(params) != NPB * depth:
        raise _lib.CffmError('expected %d parameter tensors for depth %d, got %d' % (NPB * depth, depth, len(params)))
    ring = ring.detach()
    r, b = ring.shape[0], ring.shape[1]
    g, (key_src, q_dst, *_) = _layer_geom(lib, b, h0, w0, ring.device)
    ws, out = _infer_buffers(lib, g, depth, prepared, ws, out, (b, h0 * w0, 256), ring.device)
    img = h0 * w0 * 256
    _lib.check(lib.cffm_layer_infer_rows_ring(C.byref(g), depth, block_structs(params, depth), _ptr(prepared), _ptr(ring), b * img, r, _ptr(slots),
                                              img, _ptr(out), _ptr(key_src), _ptr(q_dst), _ptr(ws), _stream(ring)), lib)
    return out


def cffm_layer_rows_ring_tables(ring, tables, h0, w0, depth, params, prepared, ws=None, out=None):
    """cffm_layer_rows_ring with a clip table per sample: ring [R,h0*w0,256] holds single frames, frame t (the target last) of sample b =
    ring[tables[b, t]], tables a device int32 [B,4] the kernels read (entries may repeat within a sample and across samples; one outside
    0..R-1 is clamped on the device) -> the B new target frames [B,h0*w0,256].  Sample b's rows equal, bit for bit, cffm_layer_rows_ring
    on ``ring.unsqueeze(1)`` with ``tables[b]``.  No argument of the library call depends on the tables' contents."""
    lib = _lib.get()
    _check_frame_ring(ring, tables, (None, 4), 'cffm_layer_rows_ring_tables')
    if ring.shape[1] != h0 * w0:
        raise _lib.CffmError('cffm_layer_rows_ring_tables: ring slots [%d,256] expected, got %s' % (h0 * w0, tuple(ring.shape[1:])))
    if len(params) != NPB * depth:
        raise _lib.CffmError('expected %d parameter tensors for depth %d, got %d' % (NPB * depth, depth, len(params)))
    ring = ring.detach()
    r, b = ring.shape[0], tables.shape[0]
    g, (key_src, q_dst, *_) = _layer_geom(lib, b, h0, w0, ring.device)
    ws, out = _infer_buffers(lib, g, depth, prepared, ws, out, (b, h0 * w0, 256), ring.device)
    _lib.check(lib.cffm_layer_infer_rows_ring_tables(C.byref(g), depth, block_structs(params, depth), _ptr(prepared), _ptr(ring), h0 * w0 * 256, r,
                                                     _ptr(tables), _ptr(out), _ptr(key_src), _ptr(q_dst), _ptr(ws), _stream(ring)), lib)
    return out


# ---------------------------------------------------------------------------------------------- BN + ReLU + 1/8 clip stack
class _BnReluPoolFn(torch.autograd.Function):
    """y [N,256,H,W] (channels-last memory) -> (fused = ReLU(BatchNorm(y)) [N,256,H,W] channels-last, stack = 2x2 average of
    fused as rows [N, H/2*W/2, 256]) -- `linear_fuse`'s norm + activation and the 1/4 -> 1/8 resize of cffm_head.py:119,131-135
    in two passes over the map (statistics, apply) instead of torch's batch_norm + relu + interpolate (+ layout conversions).
    Training mode uses batch statistics (summed over the ranks of `group` when given: SyncBN) and updates the running buffers
    as torch does; eval mode uses the running statistics."""

    @staticmethod
    def forward(ctx, y, weight, bias, running_mean, running_var, training, momentum, eps, want_stack, group, mask):
        lib = _lib.get()
        _require_device(y, 'bn_relu_pool input')
        n, c, h, w = y.shape
        if c != 256 or h % 2 or w % 2:
            raise _lib.CffmError('bn_relu_pool: [N,256,even,even] expected, got %s' % (tuple(y.shape),))
        if mask is not None and (tuple(mask.shape) != (n, 256) or mask.dtype != torch.float32):
            raise _lib.CffmError('bn_relu_pool: the dropout mask is a float32 [N,256] table, got %s' % (tuple(mask.shape),))
        rows = _to_rows(lib, y) if not y.permute(0, 2, 3, 1).is_contiguous() else y.permute(0, 2, 3, 1)
        r, st, dev = n * h * w, _stream(y), y.device
        count = float(r)
        mask = mask.contiguous() if mask is not None else None
        coef = torch.empty(4, 256, dtype=torch.float32, device=dev)     # scale | shift | rstd | -mean * rstd
        if training and group is not None:
            # SyncBN: the statistics cross the process group between the two passes, so the per-channel arithmetic stays in torch
            import torch.distributed as dist
            part = torch.empty(lib.cffm_colstats_records(r), 512, dtype=torch.float32, device=dev)
            _lib.check(lib.cffm_colstats(_ptr(rows), r, _ptr(part), st), lib)
            packed = torch.cat([part.double().sum(0), torch.full((1,), count, dtype=torch.float64, device=dev)])
            dist.all_reduce(packed, group=group if group is not True else None)
            # the global element count stays ON THE DEVICE (a 0-d tensor): no host synchronisation between the two passes, so a
            # head step under SyncBN neither stalls the stream nor breaks a stream capture (`.item()` here did both)
            sums, count = packed[:512], packed[512]
            mean = sums[:256] / count
            var = (sums[256:] / count - mean * mean).clamp_min(0.)
            if running_mean is not None:
                with torch.no_grad():
                    running_mean.mul_(1 - momentum).add_(mean.float() * momentum)
                    running_var.mul_(1 - momentum).add_((var * (count / (count - 1).clamp_min(1.))).float() * momentum)
            rstd = (var + eps).rsqrt()
            coef[0], coef[1] = (weight.double() * rstd).float(), (bias.double() - mean * weight.double() * rstd).float()
            coef[2], coef[3] = rstd.float(), (-mean * rstd).float()
        else:
            # statistics -> scale / shift / running buffers in ONE launch (stock torch: ~25 kernels on 256-element vectors)
            part = None
            if training:
                part = torch.empty(lib.cffm_colstats_records(r), 512, dtype=torch.float32, device=dev)
                _lib.check(lib.cffm_colstats(_ptr(rows), r, _ptr(part), st), lib)
            w_, b_ = weight.detach().contiguous(), bias.detach().contiguous()
            _lib.check(lib.cffm_bn_finalize_fwd(_ptr(part) if training else None, part.shape[0] if training else 0, count, _ptr(w_), _ptr(b_),
                                                _ptr(running_mean) if running_mean is not None else None,
                                                _ptr(running_var) if running_var is not None else None,
                                                float(momentum), float(eps), _ptr(coef), st), lib)
        fused = torch.empty(n, h, w, 256, dtype=torch.float32, device=dev)
        stack = torch.empty(n, (h // 2) * (w // 2), 256, dtype=torch.float32, device=dev) if want_stack else None
        _lib.check(lib.cffm_bn_relu_pool_fwd(_ptr(rows), _ptr(coef[0]), _ptr(coef[1]), _ptr(mask) if mask is not None else None, _ptr(fused),
                                             _ptr(stack) if want_stack else None, n, h, w, st), lib)
        ctx.save_for_backward(rows, coef, weight, mask if mask is not None else torch.empty(0, device=dev))
        ctx.dims, ctx.training, ctx.count, ctx.group = (n, h, w), training, count, group
        out_stack = stack if want_stack else torch.empty(0, device=dev)
        return fused.permute(0, 3, 1, 2), out_stack

    @staticmethod
    def backward(ctx, dfused, dstack):
        lib = _lib.get()
        _join_deferred()          # dfused may come from the deferred branch (frame_logits_cat's backward)
        rows, coef, weight, mask = ctx.saved_tensors
        mask = mask if mask.numel() else None
        n, h, w = ctx.dims
        r, st, dev = n * h * w, _stream(rows), rows.device
        df = None
        if dfused is not None:
            df = dfused.permute(0, 2, 3, 1)
            df = df if df.is_contiguous() else _to_rows(lib, dfused.contiguous())
        ds = dstack.contiguous() if (dstack is not None and dstack.numel()) else None
        g = torch.empty(n, h, w, 256, dtype=torch.float32, device=dev)
        part = torch.empty(lib.cffm_bn_relu_pool_records(n, h, w), 512, dtype=torch.float32, device=dev)
        _lib.check(lib.cffm_bn_relu_pool_bwd1(_ptr(rows), _ptr(coef[0]), _ptr(coef[1]), _ptr(coef[2]), _ptr(coef[3]),
                                              _ptr(mask) if mask is not None else None, _ptr(df) if df is not None else None,
                                              _ptr(ds) if ds is not None else None, _ptr(g), _ptr(part), n, h, w, st), lib)
        out = torch.empty(5, 256, dtype=torch.float32, device=dev)       # dbias | dweight | mean g | mean g*xhat | gamma*rstd
        w_ = weight.detach().contiguous()
        if ctx.training and ctx.group is not None:
            import torch.distributed as dist
            sums = part.double().sum(0)
            out[0], out[1] = sums[:256].float(), sums[256:].float()       # of THIS rank (DDP averages parameter gradients itself)
            sums = sums.clone()
            dist.all_reduce(sums, group=ctx.group if ctx.group is not True else None)
            out[2], out[3] = (sums[:256] / ctx.count).float(), (sums[256:] / ctx.count).float()
            out[4] = w_ * coef[2]
        else:
            _lib.check(lib.cffm_bn_finalize_bwd(_ptr(part), part.shape[0], ctx.count, _ptr(w_), _ptr(coef[2]), 1 if ctx.training else 0,
                                                _ptr(out), st), lib)
        _lib.check(lib.cffm_bn_bwd2(_ptr(g), _ptr(rows), _ptr(coef[2]), _ptr(coef[3]), _ptr(out[4]), _ptr(out[2]), _ptr(out[3]), r, st), lib)
        return g.permute(0, 3, 1, 2), out[1], out[0], None, None, None, None, None, None, None, None


def bn_relu_pool(y, bn, want_stack=True, drop_mask=None):
    """ReLU(bn(y)) and its 2x2-average clip-stack rows; `bn` is the head's BatchNorm2d / SyncBatchNorm module (its parameters,
    running buffers, momentum, eps and training flag are honoured; SyncBatchNorm exchanges the batch statistics over the default
    process group when one is initialised).  `drop_mask` [N,256] (factors 0 or 1/(1-p)): Dropout2d of the first output folded into
    the same pass -- the stack is taken before it, as cffm_head.py:119-131 does."""
    group = None
    if isinstance(bn, torch.nn.SyncBatchNorm) and bn.training:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            group = bn.process_group if bn.process_group is not None else True
    training = bn.training or bn.running_mean is None
    if bn.training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    if bn.momentum is not None:
        momentum = bn.momentum
    elif bn.training and bn.num_batches_tracked is not None:
        momentum = 1.0 / float(bn.num_batches_tracked)      # torch: momentum=None means a cumulative moving average (one host read, as torch does)
    else:
        momentum = 0.0
    fused, stack = _BnReluPoolFn.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, momentum, bn.eps, want_stack, group,
                                       drop_mask)
    return fused, (stack if want_stack else None)


# ---------------------------------------------------------------------------------------------- bilinear resize of token rows
class _RowsResizeFn(torch.autograd.Function):
    """F.interpolate(mode='bilinear', align_corners=False) on token rows: [N,h,w,C] -> [N,H,W,C] (C % 4 == 0).  The gradient is read
    where it lies (maps may be slices of a larger rows buffer), the adjoint is a deterministic gather."""

    @staticmethod
    def forward(ctx, rows, H, W):
        lib = _lib.get()
        _require_device(rows, 'rows_resize input')
        if rows.dim() != 4 or rows.dtype != torch.float32 or rows.shape[3] % 4:
            raise _lib.CffmError('rows_resize: fp32 [N,h,w,C] with C %% 4 == 0 expected, got %s %s' % (tuple(rows.shape), rows.dtype))
        rows = rows.contiguous()
        n, h, w, c = rows.shape
        out = torch.empty(n, H, W, c, dtype=torch.float32, device=rows.device)
        _lib.check(lib.cffm_rows_resize_fwd(_ptr(rows), h * w * c, _ptr(out), H * W * c, n, h, w, H, W, c, _stream(rows)), lib)
        ctx.dims = (n, h, w, H, W, c)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.get()
        n, h, w, H, W, c = ctx.dims
        if not (n == 0 or (dout.stride()[1:] == (W * c, c, 1) and dout.stride(0) >= H * W * c and dout.stride(0) % 4 == 0)):
            dout = dout.contiguous()
        din = torch.empty(n, h, w, c, dtype=torch.float32, device=dout.device)
        _lib.check(lib.cffm_rows_resize_bwd(_ptr(dout), dout.stride(0) if n else H * W * c, _ptr(din), h * w * c, n, h, w, H, W, c,
                                            _stream(dout)), lib)
        return din, None, None


def rows_resize(rows, size):
    """bilinear resize (align_corners=False) of token rows [N,h,w,C] to [N,H,W,C]"""
    return _RowsResizeFn.apply(rows, int(size[0]), int(size[1]))


# ---------------------------------------------------------------------------------------------- resize + cross entropy
class _UpceFn(torch.autograd.Function):
    """sum over pixels of CE(resize(logits)[pixel], label[pixel]) and the number of pixels whose arg-max is the label,
    without the [M,K,H,W] resized logits (csrc/segloss_kernels.h)."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        lib = _lib.get()
        _require_device(logits, 'resize_cross_entropy logits')
        if logits.dim() != 4 or labels.dim() != 3 or labels.shape[0] != logits.shape[0] or labels.dtype != torch.int64:
            raise _lib.CffmError('resize_cross_entropy: logits [M,K,h,w] fp32 and labels [M,H,W] int64 expected, got %s %s / %s %s'
                                 % (tuple(logits.shape), logits.dtype, tuple(labels.shape), labels.dtype))
        if labels.device != logits.device:
            raise _lib.CffmError('resize_cross_entropy: labels on %s, logits on %s' % (labels.device, logits.device))
        logits, labels = logits.contiguous(), labels.contiguous()
        m, k, h, w = logits.shape
        H, W = labels.shape[1:]
        lse = torch.empty(m, H, W, dtype=torch.float32, device=logits.device)
        part = torch.empty(lib.cffm_upce_blocks(m, H, W), 2, dtype=torch.float32, device=logits.device)
        _lib.check(lib.cffm_upce_fwd(_ptr(logits), _ptr(labels), _ptr(lse), _ptr(part), m, k, h, w, H, W, int(ignore_index),
                                     _stream(logits)), lib)
        sums = part.double().sum(0).float()          # [loss sum, hits]: a plain deterministic reduction of the workgroup records
        ctx.save_for_backward(logits, labels, lse)
        ctx.ignore_index = int(ignore_index)
        hits = sums[1].clone()
        ctx.mark_non_differentiable(hits)
        return sums[0].clone(), hits

    @staticmethod
    def backward(ctx, gloss, _ghits):
        lib = _lib.get()
        logits, labels, lse = ctx.saved_tensors
        m, k, h, w = logits.shape
        H, W = labels.shape[1:]
        gs = gloss.to(torch.float32).contiguous()    # device scalar: read by the kernel, never by the host
        dlogits = torch.empty_like(logits)
        _lib.check(lib.cffm_upce_bwd(_ptr(logits), _ptr(labels), _ptr(lse), _ptr(gs), 1.0, _ptr(dlogits), m, k, h, w, H, W,
                                     ctx.ignore_index, _stream(logits)), lib)
        return dlogits, None, None


def resize_cross_entropy(logits, labels, ignore_index=255):
    """(sum of per-pixel cross entropies, number of correctly classified pixels) of `logits` [M,K,h,w] resized bilinearly
    (align_corners=False) to the labels' [M,H,W] resolution -- what decode_head.py:744-835 computes through a materialised
    [M,K,H,W] tensor (resize -> F.cross_entropy(reduction='none', ignore_index) -> sum; accuracy's arg-max == label count).
    Ignored pixels add 0 to both, as in the reference; divide by labels.numel() for its `mean` / percentage."""
    return _UpceFn.apply(logits, labels, ignore_index)


_MAPS_TABLES = {}


def _maps_tables(dev, b, t, label_idx, loss_w, hits_w):
    """device copies of the per-map tables of head_cross_entropy, made once per configuration (a host -> device copy per step would
    also keep the step from being captured in a graph)"""
    key = (str(dev), b, t, tuple(label_idx), tuple(loss_w), tuple(hits_w))
    hit = _MAPS_TABLES.get(key)
    if hit is None:
        if len(_MAPS_TABLES) > 64:
            _MAPS_TABLES.clear()
        hit = (torch.tensor([bi * t + int(i) for bi in range(b) for i in label_idx], dtype=torch.int32, device=dev),
               torch.tensor([float(x) for x in loss_w] * b, dtype=torch.float64, device=dev),
               torch.tensor([float(x) for x in hits_w] * b, dtype=torch.float64, device=dev),
               torch.tensor([float(x) for x in loss_w] * b, dtype=torch.float32, device=dev))      # (the backward's per-map scale)
        _MAPS_TABLES[key] = hit
    return hit


class _UpceMapsFn(torch.autograd.Function):
    """The head's whole loss in one pair of kernels: logits [B,n,K,h,w] (plain memory or token rows [B,n,h,w,K] viewed that way --
    no layout copy either way), labels [B,t,H,W]; map (b, i) is judged on label map (b, label_idx[i]) and enters the loss / the
    hit count with loss_w[i] / hits_w[i] (decode_head.py:744-835: the frame maps at half weight on their own frames, the
    clip-level maps on the last frame, accuracy over the frame maps)."""

    @staticmethod
    def forward(ctx, logits, labels, label_idx, loss_w, hits_w, ignore_index):
        lib = _lib.get()
        _require_device(logits, 'head_cross_entropy logits')
        if logits.dim() != 5 or labels.dim() != 4 or labels.shape[0] != logits.shape[0] or labels.dtype != torch.int64 or \
                logits.dtype != torch.float32 or labels.device != logits.device:
            raise _lib.CffmError('head_cross_entropy: logits [B,n,K,h,w] fp32 and labels [B,t,H,W] int64 on one device expected, got %s %s / %s %s'
                                 % (tuple(logits.shape), logits.dtype, tuple(labels.shape), labels.dtype))
        b, n, k, h, w = logits.shape
        t, H, W = labels.shape[1:]
        if len(label_idx) != n or len(loss_w) != n or len(hits_w) != n or any(not 0 <= int(i) < t for i in label_idx):
            raise _lib.CffmError('head_cross_entropy: one label index (< %d) and two weights per logits map expected' % t)
        st = logits.stride()
        rows = k > 1 and st[2] == 1 and st[4] == k and st[3] == w * k            # token rows [.., h, w, K]
        plain = st[4] == 1 and st[3] == w and st[2] == h * w
        if not (rows or plain) or st[1] < k * h * w or st[0] < n * st[1]:
            logits = logits.contiguous()
            st, rows, plain = logits.stride(), False, True
        labels = labels.contiguous()
        dev, m = logits.device, b * n
        lidx, wl, wh, wl32 = _maps_tables(dev, b, t, label_idx, loss_w, hits_w)
        lse = torch.empty(m, H, W, dtype=torch.float32, device=dev)
        nblk = lib.cffm_upce_blocks(m, H, W)
        part = torch.empty(nblk, 2, dtype=torch.float32, device=dev)
        ks, ps = (1, k) if rows else (h * w, 1)
        _lib.check(lib.cffm_upce_maps_fwd(_ptr(logits), _ptr(labels), _ptr(lidx), _ptr(lse), _ptr(part), m, k, h, w, H, W, int(ignore_index),
                                          n, st[0], st[1], ks, ps, _stream(logits)), lib)
        out = torch.zeros(2, dtype=torch.float32, device=dev) if not m else torch.empty(2, dtype=torch.float32, device=dev)
        if m:       # deterministic record sums and the per-map weighting in one launch (it was ~10 torch kernels: 60 us of a replayed step)
            _lib.check(lib.cffm_upce_maps_finalize(_ptr(part), m, nblk // m, _ptr(wl), _ptr(wh), _ptr(out), _stream(logits)), lib)
        loss, hits = out[0], out[1]
        ctx.save_for_backward(logits, labels, lse, lidx, wl32)
        ctx.geom = (n, ks, ps, int(ignore_index))
        ctx.mark_non_differentiable(hits)
        return loss, hits

    @staticmethod
    def backward(ctx, gloss, _ghits):
        lib = _lib.get()
        logits, labels, lse, lidx, wl = ctx.saved_tensors
        n, ks, ps, ignore_index = ctx.geom
        b, _, k, h, w = logits.shape
        H, W = labels.shape[2:]
        st = logits.stride()
        gs = gloss.to(torch.float32).contiguous()    # device scalar: read by the kernel, never by the host
        dlogits = torch.empty_strided(logits.shape, st, dtype=torch.float32, device=logits.device)
        if b * n and (st[1] != k * h * w or st[0] != n * st[1]):
            dlogits.zero_()                          # (gaps between the maps of a padded buffer)
        _lib.check(lib.cffm_upce_maps_bwd(_ptr(logits), _ptr(labels), _ptr(lidx), _ptr(lse), _ptr(gs), _ptr(wl), 1.0, _ptr(dlogits), b * n, k,
                                          h, w, H, W, ignore_index, n, st[0], st[1], ks, ps, _stream(logits)), lib)
        return dlogits, None, None, None, None, None


def head_cross_entropy(logits, labels, label_idx, loss_w, hits_w, ignore_index=255):
    """(sum_i loss_w[i] * CE-sum of map i, sum_i hits_w[i] * correctly classified pixels of map i) over the n logits maps of every
    clip, each resized bilinearly (align_corners=False) to its label map -- the two `resize -> F.cross_entropy` branches and the
    accuracy of decode_head.py:744-835 in ONE forward and ONE backward kernel, on the logits wherever they lie (plain
    [B,n,K,h,w] or the classifiers' token rows viewed as such): no resized logits, no layout conversion, no gradient assembly."""
    return _UpceMapsFn.apply(logits, labels, tuple(label_idx), tuple(loss_w), tuple(hits_w), ignore_index)


# ---------------------------------------------------------------------------------------------- GTC
GTC_PARAM_KEYS = ('norm1.weight', 'norm1.bias', 'attn.qkv.weight', 'attn.qkv.bias', 'attn.qkv_cluster.weight',
                  'attn.qkv_cluster.bias', 'attn.proj_cluster.weight', 'attn.proj_cluster.bias', 'norm2.weight',
                  'norm2.bias', 'mlp.fc1.weight', 'mlp.fc1.bias', 'mlp.fc2.weight', 'mlp.fc2.bias')


# expected shapes of the 14 parameters (dim 256, mlp_ratio 4: the only CFFM++ prototype block the library is built for)
GTC_PARAM_SHAPES = ((256,), (256,), (768, 256), (768,), (512, 256), (512,), (256, 256), (256,), (256,), (256,), (1024, 256), (1024,),
                    (256, 1024), (256,))
_WS_FILL = None      # tests only: fill value for the block's (otherwise uninitialised) workspace, e.g. NaN


def _gtc_check_params(p, dev):
    """The library takes raw pointers: a mis-ordered, non-fp32 or off-device parameter list would be out-of-bounds device accesses, so
    it is refused here (the per-stage path of rounds 1-4 checked each tensor at its stage call)."""
    if len(p) != len(GTC_PARAM_KEYS):
        raise _lib.CffmError('gtc_block: %d parameters expected (GTC_PARAM_KEYS order), got %d' % (len(GTC_PARAM_KEYS), len(p)))
    for key, shape, t in zip(GTC_PARAM_KEYS, GTC_PARAM_SHAPES, p):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != dev:
            raise _lib.CffmError('gtc_block: parameter %s must be float32 %s on %s, got %s %s on %s'
                                 % (key, shape, dev, t.dtype, tuple(t.shape), t.device))


def _gtc_ptrs(ts):
    """cffm_gtc_params / cffm_gtc_grads from 14 tensors in GTC_PARAM_KEYS order."""
    s = _lib.GtcPtrs()
    for (name, _), t in zip(_lib.GtcPtrs._fields_, ts):
        setattr(s, name, t.data_ptr())
    return s


class _GtcBlockFn(torch.autograd.Function):
    """SwinTransformerBlock_cluster.forward (pvt/swin_transformer_2d.py:605-665), shift 0:
    x [B,T,256], centers [B,K,256] -> [B,T,256].  One library call per direction (cffm_gtc_block_forward / _backward, round 5: the q
    projection as a row-panel GEMM, proj_cluster + residual + norm2 + Mlp as the base block's fused launch, one grouped
    weight-gradient launch); rounds 1-4 sequenced ~33 stage launches here."""

    @staticmethod
    def forward(ctx, x, centers, *p):
        lib = _lib.get()
        _require_device(x, 'gtc input')
        _require_device(centers, 'gtc centers')
        p = [t.detach().contiguous() for t in p]
        _gtc_check_params(p, x.device)
        x, centers = x.contiguous(), centers.contiguous()
        b, t, c = x.shape
        k = centers.shape[1]
        if c != 256 or centers.shape[0] != b or centers.shape[2] != 256 or x.dtype != torch.float32 or centers.dtype != torch.float32:
            raise _lib.CffmError('gtc_block: x [B,T,256] and centers [B,K,256] float32 expected, got %s and %s' % (tuple(x.shape), tuple(centers.shape)))
        n = lib.cffm_gtc_ws_floats(b, t, k)
        if n <= 0:
            raise _lib.CffmError('gtc_block: bad sizes B=%d T=%d K=%d' % (b, t, k))
        ws = torch.empty(n, dtype=torch.float32, device=x.device)
        if _WS_FILL is not None:
            ws.fill_(_WS_FILL)
        out = torch.empty(b, t, c, dtype=torch.float32, device=x.device)
        ps = _gtc_ptrs(p)
        _lib.check(lib.cffm_gtc_block_forward(C.byref(ps), _ptr(x), _ptr(centers), _ptr(out), _ptr(ws), b, t, k, _stream(x)), lib)
        ctx.save_for_backward(x, centers, ws, *p)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.get()
        x, centers, ws = ctx.saved_tensors[:3]
        p = list(ctx.saved_tensors[3:])
        if dout.shape != x.shape or dout.dtype != torch.float32 or dout.device != x.device:
            raise _lib.CffmError('gtc_block backward: float32 gradient of shape %s on %s expected, got %s %s on %s'
                                 % (tuple(x.shape), x.device, dout.dtype, tuple(dout.shape), dout.device))
        dout = dout.contiguous()
        b, t, c = x.shape
        k = centers.shape[1]
        grads = [torch.empty_like(v) for v in p]
        dx, dcenters = torch.empty_like(x), torch.empty_like(centers)
        ps, gs = _gtc_ptrs(p), _gtc_ptrs(grads)
        _lib.check(lib.cffm_gtc_block_backward(C.byref(ps), C.byref(gs), _ptr(x), _ptr(centers), _ptr(dout), _ptr(dx), _ptr(dcenters), _ptr(ws),
                                               b, t, k, _stream(x)), lib)
        return (dx, dcenters) + tuple(grads)


def gtc_block(x, centers, params):
    """params: 14 tensors in GTC_PARAM_KEYS order."""
    return _GtcBlockFn.apply(x, centers, *params)


# ---------------------------------------------------------------------------------------------- prediction (resize, resize, softmax, flip, arg-max)
_FLIPS = {None: 0, False: 0, 'horizontal': 1, 'vertical': 2}


def _predict_layout(logits):
    """(ms_outer, ks, ps) of [B,K,h,w] logits the library can read where they lie, or None: plain memory (cells contiguous) or the heads'
    token rows [B,h,w,K] viewed as [B,K,h,w] (classes contiguous), rows dense either way; the stride of a size-1 dimension says nothing"""
    b, k, h, w = logits.shape
    sb, sk, sh, sw = logits.stride()
    if (w == 1 or sw == 1) and (h == 1 or sh == w) and (k == 1 or sk == h * w):
        return (sb if b > 1 else 0), h * w, 1
    if (k == 1 or sk == 1) and (w == 1 or sw == k) and (h == 1 or sh == w * k):
        return (sb if b > 1 else 0), 1, k
    return None


def predict(logits, size, ori_size=None, flip=None, probs=None, accumulate=False, want_pred=True):
    """Label maps int64 [B,H,W] from logits [B,K,h,w]: bilinear resize (align_corners=False) to `size` (the network input), a second one to
    `ori_size` (None: `size`), softmax over K, flip of the result ('horizontal' / 'vertical'), arg-max -- EncoderDecoder_clips' tail
    (encoder_decoder.py:367-378, 502-572) in ONE kernel of libcffm_hip.so; the resized logits and the probabilities never exist.  The
    logits are read where they lie when the class stride or the pixel stride is 1 (the heads' permuted token-row views: no copy).
    `probs` (fp32 [B,K,H,W], contiguous): also write the softmax probabilities there, or add them with `accumulate` (the sum over
    augmentations of aug_test); with `want_pred=False` only that is done and None is returned.  No autograd."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 4:
        raise _lib.CffmError('predict: logits must be a [B,K,h,w] tensor')
    _require_device(logits, 'predict logits')
    if flip not in _FLIPS:
        raise _lib.CffmError("predict: flip must be None, 'horizontal' or 'vertical', got %r" % (flip,))
    lib = _lib.get()
    logits = logits.detach()
    layout = _predict_layout(logits)
    if layout is None:
        logits = logits.contiguous()
        layout = _predict_layout(logits)
    b, k, h, w = logits.shape
    hm, wm = int(size[0]), int(size[1])
    H, W = (hm, wm) if ori_size is None else (int(ori_size[0]), int(ori_size[1]))
    if probs is not None:
        if probs.dtype != torch.float32 or probs.device != logits.device or tuple(probs.shape) != (b, k, H, W) or not probs.is_contiguous():
            raise _lib.CffmError('predict: probs must be a contiguous fp32 [%d,%d,%d,%d] tensor on %s' % (b, k, H, W, logits.device))
    elif accumulate or not want_pred:
        raise _lib.CffmError('predict: accumulate / want_pred=False need probs')
    ms_outer, ks, ps = layout
    args = (int(bool(accumulate)), b, k, h, w, hm, wm, H, W, _FLIPS[flip], 1, ms_outer, 0, ks, ps, _stream(logits))
    pred = torch.empty((b, H, W), dtype=torch.int64, device=logits.device) if want_pred else None
    _lib.check(lib.cffm_predict(_ptr(logits), _ptr(pred), _ptr(probs), *args), lib)
    return pred


# ---------------------------------------------------------------------------------------------- Mix-FFN middle (depthwise 3x3 + bias + GELU)
class _DwconvGeluFn(torch.autograd.Function):
    """gelu(dwconv3x3(h) + b) on token rows [M, H*W, C] (csrc/mixffn_kernels.h).  Saved: h, weight, bias -- the pre-activation is
    recomputed in the backward, whose workspace (the GELU-scaled gradient + the partial weight-gradient slabs) lives only inside it."""

    @staticmethod
    def forward(ctx, h, weight, bias, H, W):
        lib = _lib.get()
        # every input contiguous BEFORE the stream is looked up or anything is enqueued: a copy made later would be ordered against nothing
        h, weight, bias = h.contiguous(), weight.contiguous(), bias.contiguous()
        m, n, c = h.shape
        out = torch.empty_like(h)
        _lib.check(lib.cffm_dwconv_gelu_fwd(_ptr(h), _ptr(weight), _ptr(bias), _ptr(out), m, H, W, c, _stream(h)), lib)
        ctx.save_for_backward(h, weight, bias)
        ctx.dims = (m, H, W, c)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.get()
        h, weight, bias = ctx.saved_tensors
        m, H, W, c = ctx.dims
        dout = dout.contiguous()
        dh, dw, db = torch.empty_like(h), torch.empty_like(weight), torch.empty_like(bias)
        nbytes = lib.cffm_dwconv_gelu_bwd_workspace_bytes(m, H, W, c)
        if nbytes < 0:
            raise _lib.CffmError('libcffm_hip: %s' % lib.cffm_last_error().decode())
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=h.device)
        _lib.check(lib.cffm_dwconv_gelu_bwd(_ptr(h), _ptr(weight), _ptr(bias), _ptr(dout), _ptr(dh), _ptr(dw), _ptr(db), _ptr(ws), m, H, W, c,
                                            _stream(h)), lib)
        return dh, dw, db, None, None


def dwconv_gelu(h, weight, bias, H, W):
    """MiT's Mix-FFN between fc1 and fc2 (mix_transformer.py:48-55, 358-369) in one pass: h [M, H*W, C] fp32 token rows, weight [C,1,3,3]
    and bias [C] of the depthwise Conv2d(C, C, 3, 1, 1, groups=C) -> gelu(conv(h) + bias) as token rows.  Differentiable in h, weight and
    bias (dw / db bit-reproducible); under no_grad only the forward runs and nothing is saved.  Launches on the current stream."""
    if not isinstance(h, torch.Tensor) or h.dim() != 3:
        raise _lib.CffmError('dwconv_gelu: h must be a [M, H*W, C] tensor')
    for t, what in ((h, 'dwconv_gelu h'), (weight, 'dwconv_gelu weight'), (bias, 'dwconv_gelu bias')):
        _require_device(t, what)
    H, W = int(H), int(W)
    m, n, c = h.shape
    if n != H * W or tuple(weight.shape) != (c, 1, 3, 3) or tuple(bias.shape) != (c,):
        raise _lib.CffmError('dwconv_gelu: h %s with H=%d W=%d needs weight [%d,1,3,3] and bias [%d], got %s / %s'
                             % (tuple(h.shape), H, W, c, c, tuple(weight.shape), tuple(bias.shape)))
    return _DwconvGeluFn.apply(h, weight, bias, H, W)


# ---------------------------------------------------------------------------------------------- spatial-reduction attention core (MiT backbone)
def _sra_forward(lib, q, kv, heads, scale, want_lse):
    """q [B,N,C], kv [B,Nk,2C] contiguous -> (out [B,N,C], lse [B,heads,N] or None)"""
    b, n, c = q.shape
    nk = kv.shape[1]
    out = torch.empty_like(q)
    lse = torch.empty((b, heads, n), dtype=torch.float32, device=q.device) if want_lse else None
    _lib.check(lib.cffm_sra_attn_fwd(_ptr(q), _ptr(kv), _ptr(out), _ptr(lse), b, n, nk, heads, c // heads, scale, _stream(q)), lib)
    return out, lse


def _sra_operand(t):
    """contiguous and 16-byte aligned (a contiguous slice of a larger buffer may start anywhere)"""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _SraAttnFn(torch.autograd.Function):
    """softmax(scale q_h k_h^T) v_h per head on the Linear layers' own layouts (csrc/sra_kernels.h).  Saved: q, kv, out and one
    log-sum-exp per (image, head, query) -- the probabilities are recomputed in the backward, whose workspace (delta + the partial dk / dv
    slabs) lives only inside it."""

    @staticmethod
    def forward(ctx, q, kv, heads, scale):
        lib = _lib.get()
        # every input contiguous BEFORE the stream is looked up or anything is enqueued: a copy made later would be ordered against nothing
        q, kv = _sra_operand(q), _sra_operand(kv)
        out, lse = _sra_forward(lib, q, kv, heads, scale, True)
        ctx.save_for_backward(q, kv, out, lse)
        ctx.heads, ctx.scale = heads, scale
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.get()
        q, kv, out, lse = ctx.saved_tensors
        b, n, c = q.shape
        nk, heads = kv.shape[1], ctx.heads
        dout = _sra_operand(dout)
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        nbytes = lib.cffm_sra_attn_bwd_workspace_bytes(b, n, nk, heads, c // heads)
        if nbytes < 0:
            raise _lib.CffmError('libcffm_hip: %s' % lib.cffm_last_error().decode())
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=q.device)
        _lib.check(lib.cffm_sra_attn_bwd(_ptr(q), _ptr(kv), _ptr(out), _ptr(lse), _ptr(dout), _ptr(dq), _ptr(dkv), _ptr(ws), b, n, nk, heads,
                                         c // heads, ctx.scale, _stream(q)), lib)
        return dq, dkv, None, None


def sra_attention(q, kv, num_heads, scale):
    """The core of MiT's spatial-reduction attention (mix_transformer.py Attention.forward between the q / kv Linear layers and proj) in
    one pass: q [B,N,C] and kv [B,Nk,2C] fp32 as the two Linear layers leave them (head h = columns h*hd .. of q; K = columns h*hd ..,
    V = columns C + h*hd .. of kv; hd = C / num_heads, 32 or 64) -> softmax(scale q_h k_h^T) v_h as [B,N,C] in the reference's
    transpose(1,2).reshape order.  The scores never exist.  Differentiable in q and kv (bit-reproducible); under no_grad, or when neither
    requires grad, only the forward runs, without the log-sum-exp, and nothing is saved.  Launches on the current stream."""
    if not isinstance(q, torch.Tensor) or not isinstance(kv, torch.Tensor) or q.dim() != 3 or kv.dim() != 3:
        raise _lib.CffmError('sra_attention: q must be a [B,N,C] tensor and kv a [B,Nk,2C] tensor')
    _require_device(q, 'sra_attention q')
    _require_device(kv, 'sra_attention kv')
    heads, scale = int(num_heads), float(scale)
    b, n, c = q.shape
    if heads < 1 or c % heads or c // heads not in (32, 64):
        raise _lib.CffmError('sra_attention: C=%d with %d heads: the head size must be 32 or 64' % (c, heads))
    if kv.shape[0] != b or kv.shape[2] != 2 * c or kv.device != q.device:
        raise _lib.CffmError('sra_attention: q %s needs kv [%d,Nk,%d] on %s, got %s on %s'
                             % (tuple(q.shape), b, 2 * c, q.device, tuple(kv.shape), kv.device))
    if n < 1 or kv.shape[1] < 1:
        raise _lib.CffmError('sra_attention: N=%d and Nk=%d must be at least 1' % (n, kv.shape[1]))
    if torch.is_grad_enabled() and (q.requires_grad or kv.requires_grad):
        return _SraAttnFn.apply(q, kv, heads, scale)
    return _sra_forward(_lib.get(), _sra_operand(q.detach()), _sra_operand(kv.detach()), heads, scale, False)[0]


# ---------------------------------------------------------------------------------------------- spatial-reduction conv + LayerNorm (MiT backbone)
# The limits of cffm_sr_ln_fwd / _bwd, a copy of srln_check and SRLN_MAXC in csrc/cffm_hip.hip / srln_kernels.h (stated in
# include/cffm_hip.h): change both together.  tests/test_sr_ln.py::run_refusals walks every limit through both copies.
SR_RATIOS = (2, 4, 8)
SR_MAX_C = 512


def sr_reduce_supported(B, H, W, C, sr_ratio):
    """whether [B, H*W, C] rows with this reduction ratio are inside the limits of the library's kernels"""
    return (sr_ratio in SR_RATIOS and C % 16 == 0 and 16 <= C <= SR_MAX_C and B >= 1 and H >= sr_ratio and W >= sr_ratio
            and B * H * W * C < 2 ** 31)


def _sr_forward(lib, x, weight, bias, ln_weight, ln_bias, H, W, s, eps, want_saved):
    """contiguous, aligned operands -> (out [B,Ho*Wo,C], z or None, stats or None)"""
    b, _, c = x.shape
    nk = (H // s) * (W // s)
    out = torch.empty((b, nk, c), dtype=torch.float32, device=x.device)
    z = torch.empty_like(out) if want_saved else None
    stats = torch.empty((b * nk, 2), dtype=torch.float32, device=x.device) if want_saved else None
    _lib.check(lib.cffm_sr_ln_fwd(_ptr(x), _ptr(weight), _ptr(bias), _ptr(ln_weight), _ptr(ln_bias), _ptr(out), _ptr(z), _ptr(stats),
                                  b, H, W, c, s, eps, _stream(x)), lib)
    return out, z, stats


class _SrReduceFn(torch.autograd.Function):
    """LayerNorm(Conv2d(C, C, s, s)(x as NCHW)) on token rows (csrc/srln_kernels.h).  Saved: x, the weights, and the M = B Ho Wo rows
    before the LayerNorm with their (mean, rstd); the backward's workspace (dz + the partial column sums) lives only inside it."""

    @staticmethod
    def forward(ctx, x, weight, bias, ln_weight, ln_bias, H, W, s, eps):
        lib = _lib.get()
        # every input contiguous BEFORE the stream is looked up or anything is enqueued: a copy made later would be ordered against nothing
        x, weight, bias, ln_weight, ln_bias = (_sra_operand(t) for t in (x, weight, bias, ln_weight, ln_bias))
        out, z, stats = _sr_forward(lib, x, weight, bias, ln_weight, ln_bias, H, W, s, eps, True)
        ctx.save_for_backward(x, weight, ln_weight, z, stats)
        ctx.dims = (H, W, s, eps)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        # (one library call computes all five gradients, also when only some are asked for; those not asked for are dropped)
        lib = _lib.get()
        x, weight, ln_weight, z, stats = ctx.saved_tensors
        H, W, s, eps = ctx.dims
        b, _, c = x.shape
        dout = _sra_operand(dout)
        dx, dw = torch.empty_like(x), torch.empty_like(weight)
        db, dgamma, dbeta = (torch.empty(c, dtype=torch.float32, device=x.device) for _ in range(3))
        nbytes = lib.cffm_sr_ln_bwd_workspace_bytes(b, H, W, c, s)
        if nbytes < 0:
            raise _lib.CffmError('libcffm_hip: %s' % lib.cffm_last_error().decode())
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
        _lib.check(lib.cffm_sr_ln_bwd(_ptr(x), _ptr(weight), _ptr(ln_weight), _ptr(z), _ptr(stats), _ptr(dout), _ptr(dx), _ptr(dw), _ptr(db),
                                      _ptr(dgamma), _ptr(dbeta), _ptr(ws), b, H, W, c, s, eps, _stream(x)), lib)
        return tuple(g if need else None for g, need in zip((dx, dw, db, dgamma, dbeta), ctx.needs_input_grad)) + (None,) * 4


def sr_reduce(x, weight, bias, ln_weight, ln_bias, H, W, sr_ratio, eps=1e-5):
    """The spatial reduction in front of MiT's kv Linear (mix_transformer.py Attention.forward, sr_ratio > 1) in one pass: x [B, H*W, C]
    fp32 token rows, weight [C,C,s,s] and bias [C] of Conv2d(C, C, kernel_size=s, stride=s), ln_weight / ln_bias [C] of the LayerNorm
    -> LayerNorm(conv(x as NCHW)) as token rows [B, (H//s)*(W//s), C].  No NCHW view, no transposes; the weight is read in the Conv2d's
    own layout.  Differentiable in all five tensors (bit-reproducible; the dx of pixel rows / columns beyond the last full window is 0);
    under no_grad, or when nothing requires grad, only the forward runs and nothing is saved.  s in 2, 4, 8; C a multiple of 16, at most
    512; H, W >= s.  Launches on the current stream."""
    ts = (x, weight, bias, ln_weight, ln_bias)
    if not all(isinstance(t, torch.Tensor) for t in ts) or x.dim() != 3:
        raise _lib.CffmError('sr_reduce: x must be a [B, H*W, C] tensor, the weights tensors')
    for t, what in zip(ts, ('x', 'weight', 'bias', 'ln_weight', 'ln_bias')):
        _require_device(t, 'sr_reduce ' + what)
    H, W, s, eps = int(H), int(W), int(sr_ratio), float(eps)
    b, n, c = x.shape
    if n != H * W or tuple(weight.shape) != (c, c, s, s) or any(tuple(t.shape) != (c,) for t in ts[2:]):
        raise _lib.CffmError('sr_reduce: x %s with H=%d W=%d s=%d needs weight [%d,%d,%d,%d] and bias / ln_weight / ln_bias [%d], got %s'
                             % (tuple(x.shape), H, W, s, c, c, s, s, c, [tuple(t.shape) for t in ts[1:]]))
    if any(t.device != x.device for t in ts[1:]):
        raise _lib.CffmError('sr_reduce: all tensors must be on %s' % (x.device,))
    if not sr_reduce_supported(b, H, W, c, s) or not 0 <= eps < float('inf'):
        raise _lib.CffmError('sr_reduce: B=%d H=%d W=%d C=%d s=%d eps=%g outside the limits (s in 2, 4, 8; C a multiple of 16 in 16..%d; '
                             'H, W >= s; B*H*W*C < 2^31; eps finite, >= 0)' % (b, H, W, c, s, eps, SR_MAX_C))
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        return _SrReduceFn.apply(x, weight, bias, ln_weight, ln_bias, H, W, s, eps)
    return _sr_forward(_lib.get(), *(_sra_operand(t.detach()) for t in ts), H, W, s, eps, False)[0]


# ---------------------------------------------------------------------------------------------- LayerNorm of token rows + one MiT stage per call (inference)
# The limits of cffm_ln_rows / cffm_nchw_ln_rows / cffm_ln_rows_nchw and of cffm_mit_stage_infer: copies of mln_check and mit_cfg_check
# in csrc/cffm_hip.hip (stated in include/cffm_hip.h); change both together.  tests/test_mit_stage.py walks them through both copies.
LN_MIN_C, LN_MAX_C = 16, 512


def _infer_only(ts, what):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise _lib.CffmError('%s is inference only: call it under torch.no_grad() or with tensors that do not require grad' % what)


def ln_supported(c, numel):
    """whether rows of width c, numel elements in all, are inside the limits of the LayerNorm calls"""
    return c % 4 == 0 and LN_MIN_C <= c <= LN_MAX_C and 0 < numel < 2 ** 31


def _ln_operands(what, x, weight, bias, c):
    _ln_checked(what, x, weight, bias, c)
    _infer_only((x, weight, bias), what)
    return tuple(_sra_operand(t.detach()) for t in (x, weight, bias))


def _ln_checked(what, x, weight, bias, c):
    for t, name in ((x, 'x'), (weight, 'weight'), (bias, 'bias')):
        if not isinstance(t, torch.Tensor):
            raise _lib.CffmError('%s: %s must be a tensor' % (what, name))
        _require_device(t, '%s %s' % (what, name))
    if tuple(weight.shape) != (c,) or tuple(bias.shape) != (c,) or weight.device != x.device or bias.device != x.device:
        raise _lib.CffmError('%s: weight and bias must be [%d] tensors on %s' % (what, c, x.device))
    if c % 4 or not LN_MIN_C <= c <= LN_MAX_C:
        raise _lib.CffmError('%s: C=%d must be a multiple of 4 in %d..%d' % (what, c, LN_MIN_C, LN_MAX_C))


def _ln_out(what, out, shape, x):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=x.device)
    if out.dtype != torch.float32 or tuple(out.shape) != tuple(shape) or out.device != x.device or not out.is_contiguous():
        raise _lib.CffmError('%s: out must be a contiguous fp32 %s tensor on %s' % (what, tuple(shape), x.device))
    return out


def ln_rows(x, weight, bias, eps=1e-5, out=None):
    """F.layer_norm(x, (C,), weight, bias, eps) of fp32 token rows x [..., C], C a multiple of 4 in 16..512, in one pass with the row in
    registers (``cffm_ln_rows``).  Inference only: it raises when an input requires grad while grad mode is on."""
    if not isinstance(x, torch.Tensor) or x.dim() < 1:
        raise _lib.CffmError('ln_rows: x must be a [..., C] tensor')
    c = x.shape[-1]
    xs, w, b = _ln_operands('ln_rows', x, weight, bias, c)
    if xs.numel() == 0:
        raise _lib.CffmError('ln_rows: x is empty')
    out = _ln_out('ln_rows', out, x.shape, xs)
    lib = _lib.get()
    _lib.check(lib.cffm_ln_rows(_ptr(xs), _ptr(w), _ptr(b), _ptr(out), xs.numel() // c, c, float(eps), _stream(xs)), lib)
    return out


def nchw_ln_rows(x, weight, bias, eps=1e-5, out=None):
    """F.layer_norm(x.flatten(2).transpose(1, 2), (C,), weight, bias, eps) of an fp32 map x [B,C,H,W] -> token rows [B, H*W, C], without the
    transposed copy (``cffm_nchw_ln_rows``).  Inference only."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise _lib.CffmError('nchw_ln_rows: x must be a [B,C,H,W] tensor')
    b_, c, h, w_ = x.shape
    xs, w, b = _ln_operands('nchw_ln_rows', x, weight, bias, c)
    out = _ln_out('nchw_ln_rows', out, (b_, h * w_, c), xs)
    lib = _lib.get()
    _lib.check(lib.cffm_nchw_ln_rows(_ptr(xs), _ptr(w), _ptr(b), _ptr(out), b_, c, h, w_, float(eps), _stream(xs)), lib)
    return out


def ln_rows_nchw(x, weight, bias, H, W, eps=1e-5, out=None):
    """F.layer_norm(x, (C,), weight, bias, eps).reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous() of fp32 token rows x [B, H*W, C] -> the
    map [B,C,H,W] (``cffm_ln_rows_nchw``).  Inference only."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != int(H) * int(W):
        raise _lib.CffmError('ln_rows_nchw: x must be a [B, H*W, C] tensor')
    b_, _, c = x.shape
    xs, w, b = _ln_operands('ln_rows_nchw', x, weight, bias, c)
    out = _ln_out('ln_rows_nchw', out, (b_, c, int(H), int(W)), xs)
    lib = _lib.get()
    _lib.check(lib.cffm_ln_rows_nchw(_ptr(xs), _ptr(w), _ptr(b), _ptr(out), b_, c, int(H), int(W), float(eps), _stream(xs)), lib)
    return out


# ---------------------------------------------------------------------------------------------- the same three LayerNorms, differentiable
_LN_ROWS, _LN_FROM_NCHW, _LN_TO_NCHW = 0, 1, 2


class _LayerNormFn(torch.autograd.Function):
    """The three LayerNorm calls above with their backwards (csrc/mitln_kernels.h).  `form`: rows -> rows (dims = (M, C)), NCHW -> rows,
    rows -> NCHW (dims = (B, C, H, W)).  The forward is the inference call; saved: x, weight, bias -- mean and rstd are recomputed in the
    backward, whose workspace (the dgamma / dbeta records) lives only inside it."""

    @staticmethod
    def forward(ctx, x, weight, bias, form, dims, eps):
        lib = _lib.get()
        # every input contiguous BEFORE the stream is looked up or anything is enqueued: a copy made later would be ordered against nothing
        x, weight, bias = _sra_operand(x), _sra_operand(weight), _sra_operand(bias)
        if form == _LN_ROWS:
            out = torch.empty_like(x)
            rc = lib.cffm_ln_rows(_ptr(x), _ptr(weight), _ptr(bias), _ptr(out), *dims, eps, _stream(x))
        elif form == _LN_FROM_NCHW:
            b, c, h, w = dims
            out = torch.empty((b, h * w, c), dtype=torch.float32, device=x.device)
            rc = lib.cffm_nchw_ln_rows(_ptr(x), _ptr(weight), _ptr(bias), _ptr(out), *dims, eps, _stream(x))
        else:
            b, c, h, w = dims
            out = torch.empty((b, c, h, w), dtype=torch.float32, device=x.device)
            rc = lib.cffm_ln_rows_nchw(_ptr(x), _ptr(weight), _ptr(bias), _ptr(out), *dims, eps, _stream(x))
        _lib.check(rc, lib)
        ctx.save_for_backward(x, weight, bias)
        ctx.form, ctx.dims, ctx.eps = form, dims, eps
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lib = _lib.get()
        x, weight, bias = ctx.saved_tensors
        form, dims, eps = ctx.form, ctx.dims, ctx.eps
        dout = _sra_operand(dout)
        dx, dgamma, dbeta = torch.empty_like(x), torch.empty_like(weight), torch.empty_like(bias)
        if form == _LN_ROWS:
            rows, c, hw = dims[0], dims[1], 1
        else:
            rows, c, hw = dims[0] * dims[2] * dims[3], dims[1], dims[2] * dims[3]
        nbytes = lib.cffm_ln_bwd_workspace_bytes(rows, c, hw)
        if nbytes < 0:
            raise _lib.CffmError('libcffm_hip: %s' % lib.cffm_last_error().decode())
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
        fn = (lib.cffm_ln_rows_bwd, lib.cffm_nchw_ln_rows_bwd, lib.cffm_ln_rows_nchw_bwd)[form]
        _lib.check(fn(_ptr(x), _ptr(weight), _ptr(dout), _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(ws), *dims, eps, _stream(x)), lib)
        return dx, dgamma, dbeta, None, None, None


def layer_norm_rows(x, weight, bias, eps=1e-5):
    """``ln_rows`` with a backward: F.layer_norm(x, (C,), weight, bias, eps) of fp32 token rows x [..., C], C a multiple of 4 in 16..512,
    differentiable in x, weight and bias (``cffm_ln_rows`` / ``cffm_ln_rows_bwd``; dweight / dbias bit-reproducible).  The output has the
    bits of ``ln_rows``; x, weight and bias are all that is saved, and under no_grad nothing is.  Launches on the current stream."""
    if not isinstance(x, torch.Tensor) or x.dim() < 1:
        raise _lib.CffmError('layer_norm_rows: x must be a [..., C] tensor')
    c = x.shape[-1]
    _ln_checked('layer_norm_rows', x, weight, bias, c)
    if x.numel() == 0:
        raise _lib.CffmError('layer_norm_rows: x is empty')
    return _LayerNormFn.apply(x, weight, bias, _LN_ROWS, (x.numel() // c, c), float(eps))


def nchw_layer_norm_rows(x, weight, bias, eps=1e-5):
    """``nchw_ln_rows`` with a backward: F.layer_norm(x.flatten(2).transpose(1, 2), (C,), weight, bias, eps) of an fp32 map x [B,C,H,W] ->
    token rows [B, H*W, C]; neither direction makes a transposed copy (``cffm_nchw_ln_rows`` / ``cffm_nchw_ln_rows_bwd``)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise _lib.CffmError('nchw_layer_norm_rows: x must be a [B,C,H,W] tensor')
    _ln_checked('nchw_layer_norm_rows', x, weight, bias, x.shape[1])
    return _LayerNormFn.apply(x, weight, bias, _LN_FROM_NCHW, tuple(x.shape), float(eps))


def layer_norm_rows_nchw(x, weight, bias, H, W, eps=1e-5):
    """``ln_rows_nchw`` with a backward: F.layer_norm(x, (C,), weight, bias, eps).reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous() of
    fp32 token rows x [B, H*W, C] -> the map [B,C,H,W] (``cffm_ln_rows_nchw`` / ``cffm_ln_rows_nchw_bwd``)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != int(H) * int(W):
        raise _lib.CffmError('layer_norm_rows_nchw: x must be a [B, H*W, C] tensor')
    _ln_checked('layer_norm_rows_nchw', x, weight, bias, x.shape[2])
    return _LayerNormFn.apply(x, weight, bias, _LN_TO_NCHW, (x.shape[0], x.shape[2], int(H), int(W)), float(eps))


# ---------------------------------------------------------------------------------------------- one Linear layer on token rows, differentiable
def linear_rows_supported(in_features, out_features, rows):
    """whether a Linear layer in_features -> out_features on `rows` token rows is inside the limits of cffm_linear_rows_fwd / _bwd"""
    k, n, m = int(in_features), int(out_features), int(rows)
    return k >= 4 and n >= 4 and k % 4 == 0 and n % 4 == 0 and m >= 1 and m * max(n, k) < 2 ** 30 and n * k < 2 ** 30


class _LinearRowsFn(torch.autograd.Function):
    """y = residual + scale[sample] * (x w^T + bias) on token rows and its backward (csrc/gemm_kernels.h: the bf16-split GEMMs with the
    token-row epilogue and the scaled staging of dy).  Saved: x, the weight and the scale -- nothing else; the backward's workspace (the dw
    slabs and the db records) lives only inside it.  The residual's gradient is the incoming gradient itself, not a copy."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, scale, rps):
        lib = _lib.get()
        # every input contiguous BEFORE the stream is looked up or anything is enqueued (as _LayerNormFn.forward)
        x, weight = _sra_operand(x), _sra_operand(weight)
        bias, residual, scale = (None if t is None else _sra_operand(t) for t in (bias, residual, scale))
        n, k = weight.shape
        m = x.numel() // k
        y = torch.empty(tuple(x.shape[:-1]) + (n,), dtype=torch.float32, device=x.device)
        _lib.check(lib.cffm_linear_rows_fwd(_ptr(x), _ptr(weight), _ptr(bias), _ptr(residual), _ptr(scale), _ptr(y), m, n, k, rps, _stream(x)), lib)
        ctx.save_for_backward(x, weight, scale)
        ctx.dims = (m, n, k, rps)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lib = _lib.get()
        x, weight, scale = ctx.saved_tensors
        m, n, k, rps = ctx.dims
        want_dx, want_dw, want_db, want_dr = (bool(v) for v in ctx.needs_input_grad[:4])
        dx = dw = db = None
        if want_dx or want_dw or want_db:
            dy = _sra_operand(dout)
            dx = torch.empty_like(x) if want_dx else None
            dw = torch.empty_like(weight)                   # (the call always forms dw: a layer with a frozen weight is not the hot path)
            db = torch.empty(n, dtype=torch.float32, device=x.device) if want_db else None
            nbytes = lib.cffm_linear_rows_bwd_workspace_bytes(m, n, k, rps, int(want_dx), int(want_db))
            if nbytes < 0:
                raise _lib.CffmError('libcffm_hip: %s' % lib.cffm_last_error().decode())
            ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device) if nbytes else None
            _lib.check(lib.cffm_linear_rows_bwd(_ptr(dy), _ptr(x), _ptr(weight), _ptr(scale), _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws), m, n, k, rps,
                                                _stream(x)), lib)
        return dx, (dw if want_dw else None), db, (dout if want_dr else None), None, None


def linear_rows(x, weight, bias=None, residual=None, scale=None):
    """``residual + scale[sample] * F.linear(x, weight, bias)`` of fp32 token rows x [B, N, Cin] or [M, Cin] -> [..., Cout], one library call
    per direction (``cffm_linear_rows_fwd`` / ``cffm_linear_rows_bwd``): the three-pass bf16-split GEMM of the inference stage call with the
    residual and the per-sample factor in its epilogue.  bias [Cout], residual [..., Cout] and scale [B] (fp32; what DropPath multiplies a
    sample's branch with: 0 or 1 / keep) may each be None.  A sample whose scale is 0 leaves with the bits of its residual.  Differentiable
    in x, weight, bias and residual (not in scale); x gets no gradient formed when it needs none; every gradient is bit-reproducible and the
    residual's gradient is the incoming one, uncopied.  Cin and Cout multiples of 4, rows * max(Cin, Cout) below 2^30.  Launches on the
    current stream."""
    what = 'linear_rows'
    for t, name in ((x, 'x'), (weight, 'weight'), (bias, 'bias'), (residual, 'residual'), (scale, 'scale')):
        if t is None and name not in ('x', 'weight'):
            continue
        if not isinstance(t, torch.Tensor):
            raise _lib.CffmError('%s: %s must be a tensor' % (what, name))
        _require_device(t, '%s %s' % (what, name))
        if t.device != x.device:
            raise _lib.CffmError('%s: %s is on %s, x on %s' % (what, name, t.device, x.device))
    if x.dim() not in (2, 3) or weight.dim() != 2 or x.shape[-1] != weight.shape[1] or x.numel() == 0:
        raise _lib.CffmError('%s: x must be a non-empty [B, N, Cin] or [M, Cin] tensor and weight [Cout, Cin]' % what)
    n, k = weight.shape
    m = x.numel() // k
    if not linear_rows_supported(k, n, m):
        raise _lib.CffmError('%s: Cin=%d and Cout=%d must be multiples of 4 and rows * max(Cin, Cout) = %d below 2^30' % (what, k, n, m * max(n, k)))
    if bias is not None and tuple(bias.shape) != (n,):
        raise _lib.CffmError('%s: bias must be a [%d] tensor' % (what, n))
    if residual is not None and tuple(residual.shape) != tuple(x.shape[:-1]) + (n,):
        raise _lib.CffmError('%s: residual must be a %s tensor' % (what, tuple(x.shape[:-1]) + (n,)))
    rps = m
    if scale is not None:
        samples = scale.numel()
        if scale.dim() != 1 or samples == 0 or (x.dim() == 3 and samples != x.shape[0]) or m % samples:
            raise _lib.CffmError('%s: scale must be a [B] tensor, B = x.shape[0] for a [B, N, Cin] x and a divisor of M for an [M, Cin] x' % what)
        rps = m // samples
        scale = scale.detach()
    return _LinearRowsFn.apply(x, weight, bias, residual, scale, rps)


MIT_HEAD_SIZES = (32, 64)
MIT_SR_RATIOS = (1, 2, 4, 8)


def mit_stage_cfg(shape, blocks, embed_norm, out_norm):
    """cffm_mit_stage_cfg of a stage: `shape` = (B, C, H, W) of the patch-embedding convolution's output, `blocks` the stage's Block
    modules (all of one configuration), the two LayerNorms around them"""
    b, c, h, w = (int(v) for v in shape)
    a, m = blocks[0].attn, blocks[0].mlp
    return _lib.MitStageCfg(B=b, H=h, W=w, C=c, heads=int(a.num_heads), hidden=int(m.fc1.out_features), sr_ratio=int(a.sr_ratio),
                            depth=len(blocks), scale=float(a.scale), eps_embed=float(embed_norm.eps), eps_block=float(blocks[0].norm1.eps),
                            eps_sr=float(a.norm.eps) if a.sr_ratio > 1 else 0.0, eps_out=float(out_norm.eps))


def mit_stage_supported(cfg):
    """whether this stage is inside the limits of cffm_mit_stage_infer"""
    c, heads, s = cfg.C, cfg.heads, cfg.sr_ratio
    m = cfg.B * cfg.H * cfg.W
    eps = (cfg.eps_embed, cfg.eps_block, cfg.eps_sr, cfg.eps_out)
    return (cfg.B >= 1 and cfg.H >= 1 and cfg.W >= 1 and cfg.depth >= 1 and heads >= 1 and c % 16 == 0 and LN_MIN_C <= c <= LN_MAX_C
            and c % heads == 0 and c // heads in MIT_HEAD_SIZES and cfg.hidden >= 4 and cfg.hidden % 4 == 0 and s in MIT_SR_RATIOS
            and cfg.H >= s and cfg.W >= s and cfg.B * heads <= 65535 and m * max(2 * c, cfg.hidden) < 2 ** 30
            and 0 < cfg.scale < float('inf') and all(0 <= e < float('inf') for e in eps))


def mit_stage_tensors(blocks, embed_norm, out_norm):
    """the parameters cffm_mit_stage_infer reads, in the order of cffm_mit_block_params per block, then embed gamma / beta, out gamma /
    beta (None where the module has none: q / kv without bias, no `sr` at sr_ratio 1)"""
    ts = []
    for blk in blocks:
        a, m = blk.attn, blk.mlp
        sr = (a.sr.weight, a.sr.bias, a.norm.weight, a.norm.bias) if a.sr_ratio > 1 else (None,) * 4
        ts += [blk.norm1.weight, blk.norm1.bias, a.q.weight, a.q.bias, a.kv.weight, a.kv.bias, *sr, a.proj.weight, a.proj.bias,
               blk.norm2.weight, blk.norm2.bias, m.fc1.weight, m.fc1.bias, m.dwconv.dwconv.weight, m.dwconv.dwconv.bias, m.fc2.weight, m.fc2.bias]
    return ts + [embed_norm.weight, embed_norm.bias, out_norm.weight, out_norm.bias]


_MIT_FIELDS = [f for f, _ in _lib.MitBlockPtrs._fields_]
_MIT_OPTIONAL = {'q_b', 'kv_b', 'sr_w', 'sr_b', 'srn_g', 'srn_b'}


def mit_stage_infer(conv_out, embed_norm, blocks, out_norm, ws=None, out=None):
    """One MiT stage in eval mode behind its patch embedding's convolution, as one library call (``cffm_mit_stage_infer``): conv_out
    [B,C,H,W] fp32 (``patch_embed.proj``'s output), `embed_norm` = ``patch_embed.norm``, `blocks` = the stage's Block modules, `out_norm` =
    the stage's final LayerNorm -> the stage's NCHW map [B,C,H,W].  The parameters are read where they lie (fp32, contiguous, 16-byte
    aligned; nothing is copied or cached).  ``ws`` / ``out``: optional caller-owned workspace (``cffm_mit_stage_infer_ws_floats`` floats)
    and result, e.g. the static buffers of a captured graph.  Inference only: drop-path, dropout and autograd are not part of it, and it
    raises when an input or a parameter requires grad while grad mode is on.  Launches on the current stream."""
    lib = _lib.get()
    if not isinstance(conv_out, torch.Tensor) or conv_out.dim() != 4:
        raise _lib.CffmError('mit_stage_infer: conv_out must be a [B,C,H,W] tensor')
    _require_device(conv_out, 'mit_stage_infer conv_out')
    blocks = list(blocks)
    if not blocks:
        raise _lib.CffmError('mit_stage_infer: a stage needs at least one block')
    dev = conv_out.device
    tensors = mit_stage_tensors(blocks, embed_norm, out_norm)
    _infer_only([conv_out] + tensors, 'mit_stage_infer')
    n = len(_MIT_FIELDS)
    for i, t in enumerate(tensors):
        name = _MIT_FIELDS[i % n] if i < n * len(blocks) else 'stage norm'
        if t is None:
            if name not in _MIT_OPTIONAL:
                raise _lib.CffmError('mit_stage_infer: parameter %s is missing' % name)
            continue
        _require_device(t, 'mit_stage_infer parameter')
        if t.device != dev or not t.is_contiguous():
            raise _lib.CffmError('mit_stage_infer: parameter %s must be contiguous and on %s' % (name, dev))
    cfg = mit_stage_cfg(conv_out.shape, blocks, embed_norm, out_norm)
    need = lib.cffm_mit_stage_infer_ws_floats(C.byref(cfg))
    if need < 0:
        raise _lib.CffmError('libcffm_hip: %s' % lib.cffm_last_error().decode())
    x = _sra_operand(conv_out.detach())
    if ws is None:
        ws = torch.empty(need, dtype=torch.float32, device=dev)
    elif ws.dtype != torch.float32 or ws.numel() < need or ws.device != dev or not ws.is_contiguous():
        raise _lib.CffmError('mit_stage_infer workspace: %d contiguous fp32 values on %s expected' % (need, dev))
    out = _ln_out('mit_stage_infer', out, x.shape, x)
    structs = (_lib.MitBlockPtrs * len(blocks))()
    for i in range(len(blocks)):
        for f, t in zip(_MIT_FIELDS, tensors[i * n:(i + 1) * n]):
            setattr(structs[i], f, t.data_ptr() if t is not None else None)
    _lib.check(lib.cffm_mit_stage_infer(C.byref(cfg), structs, *(_ptr(t) for t in tensors[-4:]), _ptr(x), _ptr(out), _ptr(ws), _stream(x)), lib)
    return out


# ---------------------------------------------------------------------------------------------- the blocks of one MiT stage per call, differentiable
def mit_blocks_cfg(shape, H, W, blocks):
    """cffm_mit_stage_cfg of cffm_mit_blocks_train_*: `shape` = (B, N, C) of the token rows, `blocks` the stage's Block modules (all of one
    configuration).  eps_embed / eps_out are not read by those calls and stay 0."""
    b, _, c = (int(v) for v in shape)
    a, m = blocks[0].attn, blocks[0].mlp
    return _lib.MitStageCfg(B=b, H=int(H), W=int(W), C=c, heads=int(a.num_heads), hidden=int(m.fc1.out_features), sr_ratio=int(a.sr_ratio),
                            depth=len(blocks), scale=float(a.scale), eps_embed=0.0, eps_block=float(blocks[0].norm1.eps),
                            eps_sr=float(a.norm.eps) if a.sr_ratio > 1 else 0.0, eps_out=0.0)


def mit_blocks_train_supported(cfg):
    """whether the blocks of this stage are inside the limits of cffm_mit_blocks_train_fwd / _bwd: those of cffm_mit_stage_infer"""
    return mit_stage_supported(cfg)


def _mit_block_tensors(blocks):
    """the parameters of the blocks in the order of cffm_mit_block_params, None where a module has none"""
    return mit_stage_tensors(blocks, blocks[0].norm1, blocks[0].norm1)[:-4]


def _mit_block_structs(tensors, depth):
    n = len(_MIT_FIELDS)
    structs = (_lib.MitBlockPtrs * depth)()
    for i in range(depth):
        for f, t in zip(_MIT_FIELDS, tensors[i * n:(i + 1) * n]):
            setattr(structs[i], f, t.data_ptr() if t is not None else None)
    return structs


def _mit_scale_structs(scales, depth):
    """scales: None or depth pairs (attn factor, mlp factor) of [B] tensors or None -> cffm_mit_block_scales[depth] or None"""
    if scales is None or all(t is None for pair in scales for t in pair):
        return None
    structs = (_lib.MitBlockScales * depth)()
    for i, (sa, sm) in enumerate(scales):
        structs[i].scale_attn = sa.data_ptr() if sa is not None else None
        structs[i].scale_mlp = sm.data_ptr() if sm is not None else None
    return structs


def _mit_sized(lib, fn, cfg):
    need = fn(C.byref(cfg))
    if need < 0:
        raise _lib.CffmError('libcffm_hip: %s' % lib.cffm_last_error().decode())
    return need


class _MitBlocksTrainFn(torch.autograd.Function):
    """Every block of one MiT stage, forward and backward, as one library call each (cffm_mit_blocks_train_fwd / _bwd).  Saved: x, the
    parameters, the factors and the library's `saved` buffer (every intermediate of the forward); the backward's workspace lives only
    inside it.  All gradients are formed by the one call, also when only some are asked for; those not asked for are dropped."""

    @staticmethod
    def forward(ctx, x, cfg, scales, *params):
        lib = _lib.get()
        # every input contiguous BEFORE the stream is looked up or anything is enqueued (as _LayerNormFn.forward)
        x = _sra_operand(x)
        params = [None if t is None else _sra_operand(t) for t in params]
        if scales is not None:
            scales = [tuple(None if t is None else _sra_operand(t) for t in pair) for pair in scales]
        y = torch.empty_like(x)
        saved = torch.empty(_mit_sized(lib, lib.cffm_mit_blocks_train_saved_floats, cfg), dtype=torch.float32, device=x.device)
        need = _mit_sized(lib, lib.cffm_mit_blocks_train_fwd_ws_floats, cfg)
        ws = torch.empty(need, dtype=torch.float32, device=x.device) if need else None
        _lib.check(lib.cffm_mit_blocks_train_fwd(C.byref(cfg), _mit_block_structs(params, cfg.depth), _mit_scale_structs(scales, cfg.depth),
                                                 _ptr(x), _ptr(y), _ptr(saved), _ptr(ws), _stream(x)), lib)
        ctx.save_for_backward(x, saved, *params)
        ctx.cfg, ctx.scales = cfg, scales
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lib = _lib.get()
        x, saved, *params = ctx.saved_tensors
        cfg, scales = ctx.cfg, ctx.scales
        dy = _sra_operand(dout)
        dx = torch.empty_like(x)
        grads = [None if t is None else torch.empty_like(t) for t in params]
        ws = torch.empty(_mit_sized(lib, lib.cffm_mit_blocks_train_bwd_ws_floats, cfg), dtype=torch.float32, device=x.device)
        _lib.check(lib.cffm_mit_blocks_train_bwd(C.byref(cfg), _mit_block_structs(params, cfg.depth), _mit_scale_structs(scales, cfg.depth),
                                                 _mit_block_structs(grads, cfg.depth), _ptr(x), _ptr(saved), _ptr(dy), _ptr(dx), _ptr(ws),
                                                 _stream(x)), lib)
        need = ctx.needs_input_grad
        return (dx if need[0] else None, None, None) + tuple(g if n else None for g, n in zip(grads, need[3:]))


def mit_blocks_train(x, blocks, H, W, scales=None):
    """Every block of one MiT stage on token rows, differentiable, as ONE library call per direction (``cffm_mit_blocks_train_fwd`` /
    ``_bwd``): x [B, H*W, C] fp32 (what the patch embedding hands to the first block), `blocks` the stage's Block modules, all of one
    configuration -> what the last block hands to the stage's norm.  The result and every gradient have the bits of the same blocks run op
    by op with ``norm_impl``, ``linear_impl``, ``sr_impl``, ``attn_impl`` and ``dwconv_impl`` = 'hip'.  ``scales``: None, or a [depth, 2, B]
    fp32 tensor -- [i, 0] / [i, 1] the factor DropPath multiplies each sample's attention / Mix-FFN branch of block i with (0 or 1 / keep)
    -- or depth pairs of [B] tensors or None; it is detached and not differentiable.  Differentiable in x and every parameter; the modules'
    dropouts and DropPath modules are NOT applied (the caller draws the factors).  Limits: ``mit_blocks_train_supported``.  Launches on the
    current stream."""
    what = 'mit_blocks_train'
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise _lib.CffmError('%s: x must be a [B, H*W, C] tensor' % what)
    _require_device(x, what + ' x')
    blocks = list(blocks)
    if not blocks:
        raise _lib.CffmError('%s: a stage needs at least one block' % what)
    b, n, c = x.shape
    if n != int(H) * int(W) or x.numel() == 0:
        raise _lib.CffmError('%s: x %s is not [B, %d*%d, C]' % (what, tuple(x.shape), int(H), int(W)))
    tensors = _mit_block_tensors(blocks)
    nf = len(_MIT_FIELDS)
    for i, t in enumerate(tensors):
        name = _MIT_FIELDS[i % nf]
        if t is None:
            if name not in _MIT_OPTIONAL:
                raise _lib.CffmError('%s: parameter %s is missing' % (what, name))
            continue
        _require_device(t, what + ' parameter')
        if t.device != x.device:
            raise _lib.CffmError('%s: parameter %s must be on %s' % (what, name, x.device))
    if scales is not None:
        if isinstance(scales, torch.Tensor):
            if tuple(scales.shape) != (len(blocks), 2, b):
                raise _lib.CffmError('%s: scales must be a [%d, 2, %d] tensor' % (what, len(blocks), b))
            _require_device(scales, what + ' scales')
            scales = scales.detach().contiguous()
            scales = [(scales[i, 0], scales[i, 1]) for i in range(len(blocks))]
        else:
            scales = [tuple(pair) for pair in scales]
            if len(scales) != len(blocks) or any(len(pair) != 2 for pair in scales):
                raise _lib.CffmError('%s: scales must hold one (attention, Mix-FFN) pair per block' % what)
            for t in (t for pair in scales for t in pair if t is not None):
                _require_device(t, what + ' scales')
                if tuple(t.shape) != (b,) or t.device != x.device:
                    raise _lib.CffmError('%s: a factor must be a [%d] tensor on %s' % (what, b, x.device))
            scales = [tuple(None if t is None else t.detach() for t in pair) for pair in scales]
        if any(t is not None and t.device != x.device for pair in scales for t in pair):
            raise _lib.CffmError('%s: scales must be on %s' % (what, x.device))
    return _MitBlocksTrainFn.apply(x, mit_blocks_cfg(x.shape, H, W, blocks), scales, *tensors)


# ---------------------------------------------------------------------------------------------- the overlapping patch embedding + n stages per call (inference)
# The limits of cffm_patch_embed_fwd: a copy of pemb_check in csrc/cffm_hip.hip (stated in include/cffm_hip.h); change both together.
PEMB_KERNELS = ((7, 4), (3, 2))


def patch_embed_out_hw(proj, h, w):
    """the output size of a Conv2d `proj` on an h x w map"""
    return tuple((s + 2 * proj.padding[d] - proj.dilation[d] * (proj.kernel_size[d] - 1) - 1) // proj.stride[d] + 1 for d, s in ((0, h), (1, w)))


def patch_embed_supported(proj, shape):
    """whether the Conv2d `proj` on an fp32 input of `shape` = (B, Cin, H, W) is inside the limits of cffm_patch_embed_fwd (the module's
    configuration and the sizes; where its tensors lie is the caller's to check)"""
    if type(proj) is not torch.nn.Conv2d or len(shape) != 4:
        return False
    b, cin, h, w = (int(v) for v in shape)
    k, s = proj.kernel_size[0], proj.stride[0]
    if (tuple(proj.kernel_size) != (k, k) or tuple(proj.stride) != (s, s) or (k, s) not in PEMB_KERNELS or proj.padding != (k // 2, k // 2)
            or tuple(proj.dilation) != (1, 1) or proj.groups != 1 or proj.bias is None or proj.padding_mode != 'zeros' or proj.in_channels != cin):
        return False
    cout = proj.out_channels
    if not (1 <= cin <= 4 if k == 7 else (cin % 4 == 0 and 4 <= cin <= 512)) or cout % 16 or not LN_MIN_C <= cout <= LN_MAX_C:
        return False
    if b < 1 or h < 1 or w < 1:
        return False
    ho, wo = patch_embed_out_hw(proj, h, w)
    return b * cin * h * w < 2 ** 31 and b * ho * wo * cout < 2 ** 31


def _pemb_operands(what, x, proj, norm, infer_only=True):
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise _lib.CffmError('%s: x must be a [B,Cin,H,W] tensor' % what)
    if type(proj) is not torch.nn.Conv2d or proj.bias is None or norm.weight is None or norm.bias is None:
        raise _lib.CffmError('%s: a Conv2d with a bias and a LayerNorm with weight and bias expected' % what)
    ts = (x, proj.weight, proj.bias, norm.weight, norm.bias)
    for t in ts:
        _require_device(t, what)
        if t.device != x.device:
            raise _lib.CffmError('%s: every tensor must be on %s' % (what, x.device))
    if infer_only:
        _infer_only(ts, what)
    if (tuple(proj.kernel_size) != (proj.kernel_size[0],) * 2 or tuple(proj.stride) != (proj.stride[0],) * 2 or tuple(proj.dilation) != (1, 1)
            or proj.groups != 1 or proj.padding != (proj.kernel_size[0] // 2,) * 2 or proj.padding_mode != 'zeros'
            or proj.in_channels != x.shape[1] or tuple(norm.normalized_shape) != (proj.out_channels,)):
        raise _lib.CffmError('%s: a square Conv2d(Cin, Cout, k, stride, padding=k // 2) without dilation or groups, on x [B,Cin,H,W], and '
                             'LayerNorm(Cout) expected' % what)
    return tuple(_sra_operand(t.detach()) for t in ts) if infer_only else ts


def patch_embed(x, proj, norm, out=None):
    """``OverlapPatchEmbed.forward`` in eval mode as one kernel (``cffm_patch_embed_fwd``): norm(proj(x).flatten(2).transpose(1, 2)) of an
    fp32 map x [B,Cin,H,W] -> (token rows [B, Ho*Wo, Cout], Ho, Wo).  `proj`: Conv2d(Cin, Cout, k, stride, padding=k // 2) with (k, stride) =
    (7, 4) or (3, 2) and a bias, `norm`: LayerNorm(Cout); both are read where they lie.  The products are three-pass bf16-split (the
    accuracy class of the library's Linear GEMMs); the same bits on every call.  Inference only: it raises when an input or a parameter
    requires grad while grad mode is on."""
    xs, w, b, g, beta = _pemb_operands('patch_embed', x, proj, norm)
    bsz, cin, h, wd = xs.shape
    ho, wo = patch_embed_out_hw(proj, h, wd)
    cout = proj.out_channels
    out = _ln_out('patch_embed', out, (bsz, max(ho, 0) * max(wo, 0), cout), xs)
    lib = _lib.get()
    _lib.check(lib.cffm_patch_embed_fwd(_ptr(xs), _ptr(w), _ptr(b), _ptr(g), _ptr(beta), _ptr(out), bsz, cin, h, wd, cout,
                                        int(proj.kernel_size[0]), int(proj.stride[0]), float(norm.eps), _stream(xs)), lib)
    return out, ho, wo


class _PatchEmbedFn(torch.autograd.Function):
    """``patch_embed`` with its backward (csrc/pembed_kernels.h).  The forward is the inference kernel's instantiation that also stores z, the
    pre-LayerNorm rows; saved: x, the weight, gamma and z -- mean and rstd are recomputed in the backward, whose workspace (dz, the LayerNorm
    records, the dw slabs, the transposed weight) lives only inside it."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, k, stride, eps):
        lib = _lib.get()
        # every input contiguous BEFORE the stream is looked up or anything is enqueued (as _LayerNormFn.forward)
        x, weight, bias, gamma, beta = (_sra_operand(t) for t in (x, weight, bias, gamma, beta))
        bsz, cin, h, w = x.shape
        cout = weight.shape[0]
        ho, wo = ((v + 2 * (k // 2) - k) // stride + 1 for v in (h, w))
        out = torch.empty((bsz, max(ho, 0) * max(wo, 0), cout), dtype=torch.float32, device=x.device)
        z = torch.empty_like(out)
        _lib.check(lib.cffm_patch_embed_fwd_train(_ptr(x), _ptr(weight), _ptr(bias), _ptr(gamma), _ptr(beta), _ptr(out), _ptr(z), bsz, cin, h, w,
                                                  cout, k, stride, eps, _stream(x)), lib)
        ctx.save_for_backward(x, weight, gamma, z)
        ctx.conv = (k, stride, eps)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lib = _lib.get()
        x, weight, gamma, z = ctx.saved_tensors
        k, stride, eps = ctx.conv
        dout = _sra_operand(dout)
        bsz, cin, h, w = x.shape
        cout = weight.shape[0]
        want_dx = bool(ctx.needs_input_grad[0])
        dx = torch.empty_like(x) if want_dx else None
        dw = torch.empty_like(weight)
        db, dgamma, dbeta = (torch.empty(cout, dtype=torch.float32, device=x.device) for _ in range(3))
        nbytes = lib.cffm_patch_embed_bwd_workspace_bytes(bsz, cin, h, w, cout, k, stride, int(want_dx))
        if nbytes < 0:
            raise _lib.CffmError('libcffm_hip: %s' % lib.cffm_last_error().decode())
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
        _lib.check(lib.cffm_patch_embed_bwd(_ptr(x), _ptr(weight), _ptr(gamma), _ptr(z), _ptr(dout), _ptr(dx), _ptr(dw), _ptr(db), _ptr(dgamma),
                                            _ptr(dbeta), _ptr(ws), bsz, cin, h, w, cout, k, stride, eps, _stream(x)), lib)
        return dx, dw, db, dgamma, dbeta, None, None, None


def overlap_patch_embed(x, proj, norm):
    """``patch_embed`` with a backward: norm(proj(x).flatten(2).transpose(1, 2)) of an fp32 map x [B,Cin,H,W] -> (token rows [B, Ho*Wo, Cout],
    Ho, Wo), differentiable in x ((k, stride) = (3, 2) only), proj.weight, proj.bias, norm.weight and norm.bias (``cffm_patch_embed_fwd_train``
    / ``cffm_patch_embed_bwd``; every gradient bit-reproducible).  The rows have the bits of ``patch_embed``; x, the weight, norm.weight and
    the pre-LayerNorm rows are all that is saved.  Under no_grad, or with nothing that requires grad, it IS ``patch_embed``.  A 7 x 7
    embedding whose x requires grad raises: that input gradient is not built.  Launches on the current stream."""
    what = 'overlap_patch_embed'
    ts = _pemb_operands(what, x, proj, norm, infer_only=False)
    if not (torch.is_grad_enabled() and any(t.requires_grad for t in ts)):
        return patch_embed(x, proj, norm)
    k, stride = int(proj.kernel_size[0]), int(proj.stride[0])
    if (k, stride) not in PEMB_KERNELS:
        raise _lib.CffmError('%s: (k, stride) = (%d, %d) is neither (7, 4) nor (3, 2)' % (what, k, stride))
    if k != 3 and x.requires_grad:
        raise _lib.CffmError('%s: the input gradient exists for (k, stride) = (3, 2) only; x must not require grad' % what)
    ho, wo = patch_embed_out_hw(proj, x.shape[2], x.shape[3])
    return _PatchEmbedFn.apply(x, proj.weight, proj.bias, norm.weight, norm.bias, k, stride, float(norm.eps)), ho, wo


def mit_stages(shape, stages):
    """(the cffm_mit_stage array of `stages` on an input of `shape` = (B, Cin, H, W), the objects it points into, the output shapes);
    `stages`: (patch_embed, blocks, out_norm) per stage, patch_embed with .proj and .norm"""
    b, cin, h, w = (int(v) for v in shape)
    arr, keep, shapes = (_lib.MitStage * len(stages))(), [], []
    n = len(_MIT_FIELDS)
    for i, (pe, blocks, out_norm) in enumerate(stages):
        blocks = list(blocks)
        if not blocks:
            raise _lib.CffmError('mit_infer: a stage needs at least one block')
        ho, wo = patch_embed_out_hw(pe.proj, h, w)
        cout = int(pe.proj.out_channels)
        tensors = mit_stage_tensors(blocks, pe.norm, out_norm)
        structs = (_lib.MitBlockPtrs * len(blocks))()
        for j in range(len(blocks)):
            for f, t in zip(_MIT_FIELDS, tensors[j * n:(j + 1) * n]):
                setattr(structs[j], f, t.data_ptr() if t is not None else None)
        s = arr[i]
        s.cfg = mit_stage_cfg((b, cout, ho, wo), blocks, pe.norm, out_norm)
        s.Cin, s.Hin, s.Win, s.k, s.stride = cin, h, w, int(pe.proj.kernel_size[0]), int(pe.proj.stride[0])
        s.conv_w, s.conv_b = pe.proj.weight.data_ptr(), pe.proj.bias.data_ptr() if pe.proj.bias is not None else None
        s.embed_g, s.embed_b, s.out_g, s.out_b = (t.data_ptr() if t is not None else None for t in tensors[-4:])
        s.blocks = structs
        keep.append((structs, tensors))
        shapes.append((b, cout, ho, wo))
        cin, h, w = cout, ho, wo
    return arr, keep, shapes


def mit_infer(x, stages, ws=None, outs=None):
    """n = 1..4 consecutive MiT stages in eval mode, patch embeddings included, as ONE library call (``cffm_mit_infer``): x [B,Cin,H,W] fp32
    -> the list of the stages' NCHW maps.  `stages`: (patch_embed, blocks, out_norm) per stage -- an OverlapPatchEmbed (``.proj``,
    ``.norm``), the stage's Block modules, its final LayerNorm; every parameter is read where it lies (fp32, contiguous, 16-byte aligned).
    ``ws`` / ``outs``: optional caller-owned workspace (``cffm_mit_infer_ws_floats`` floats: the largest stage's, not the sum) and results,
    e.g. the static buffers of a captured graph.  Everything goes to the current stream as a single chain.  Inference only: it raises when
    an input or a parameter requires grad while grad mode is on."""
    lib = _lib.get()
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise _lib.CffmError('mit_infer: x must be a [B,Cin,H,W] tensor')
    _require_device(x, 'mit_infer x')
    stages = [(pe, list(blocks), norm) for pe, blocks, norm in stages]
    if not 1 <= len(stages) <= 4:
        raise _lib.CffmError('mit_infer: 1..4 stages expected, got %d' % len(stages))
    dev = x.device
    every = [x]
    for pe, blocks, norm in stages:
        if type(pe.proj) is not torch.nn.Conv2d or pe.proj.bias is None:
            raise _lib.CffmError('mit_infer: patch_embed.proj must be a Conv2d with a bias')
        ts = [pe.proj.weight, pe.proj.bias] + (mit_stage_tensors(blocks, pe.norm, norm) if blocks else [])
        for t in ts:
            if t is None:
                continue
            _require_device(t, 'mit_infer parameter')
            if t.device != dev or not t.is_contiguous():
                raise _lib.CffmError('mit_infer: every parameter must be contiguous and on %s' % dev)
        every += ts
    _infer_only(every, 'mit_infer')
    xs = _sra_operand(x.detach())
    arr, keep, shapes = mit_stages(xs.shape, stages)
    need = lib.cffm_mit_infer_ws_floats(arr, len(stages))
    if need < 0:
        raise _lib.CffmError('libcffm_hip: %s' % lib.cffm_last_error().decode())
    if ws is None:
        ws = torch.empty(need, dtype=torch.float32, device=dev)
    elif ws.dtype != torch.float32 or ws.numel() < need or ws.device != dev or not ws.is_contiguous():
        raise _lib.CffmError('mit_infer workspace: %d contiguous fp32 values on %s expected' % (need, dev))
    if outs is None:
        outs = [None] * len(stages)
    if len(outs) != len(stages):
        raise _lib.CffmError('mit_infer: %d outputs expected' % len(stages))
    outs = [_ln_out('mit_infer', o, s, xs) for o, s in zip(outs, shapes)]
    ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    _lib.check(lib.cffm_mit_infer(arr, len(stages), _ptr(xs), ptrs, _ptr(ws), _stream(xs)), lib)
    del keep
    return outs
