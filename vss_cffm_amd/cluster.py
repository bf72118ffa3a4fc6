"""k-means on token rows in libcffm_hip.so (include/cffm_hip.h ABI 13: cffm_kmeans): the prototype-generating stage of CFFM++.

One library call enqueues every iteration on the caller's stream (no host round trip: it can be captured into a HIP graph).  Semantics
are those of ``head._kmeans``: euclidean Lloyd iterations, a fixed iteration count, a centre that attracts no point keeps its value.
"""
import ctypes as C

import torch

from . import _lib
from .ops import _ptr, _stream


def kmeans_workspace(n, k, device):
    """the transient workspace of one ``kmeans`` call on [n,256] rows with k centres (uint8)"""
    lib = _lib.get()
    nbytes = lib.cffm_kmeans_workspace_bytes(n, k)
    if nbytes < 0:
        raise _lib.CffmError('libcffm_hip: %s' % lib.cffm_last_error().decode())
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def kmeans(x, k, iters=10, init=None, ws=None):
    """x [N,256] or [B,N,256] (fp32, contiguous) -> (centers [k,256] fp32, labels [N] int32, counts [k] int32), each with a leading B for
    a batched x.  ``init`` ([k,256] / [B,k,256]) gives the initial centres; None draws ``x[torch.randperm(N, device=x.device)[:k]]`` per
    clip, as ``head._kmeans`` does.  labels / counts are those of the last assignment made (against the centres that entered the last
    iteration).  ``ws``: a workspace from ``kmeans_workspace`` to reuse (e.g. under graph capture).  No autograd."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3):
        raise _lib.CffmError('kmeans: x must be a [N,256] or [B,N,256] tensor')
    if _lib._override is None and not x.is_cuda:
        raise _lib.CffmError('kmeans: runs only on the GPU (got a %s tensor); there is no CPU fallback' % x.device)
    if x.dtype != torch.float32:
        raise _lib.CffmError('kmeans: fp32 expected, got %s' % x.dtype)
    if not x.is_contiguous():
        raise _lib.CffmError('kmeans: x must be contiguous')
    if x.shape[-1] != 256:
        raise _lib.CffmError('kmeans: 256 channels expected, got %d' % x.shape[-1])
    lib = _lib.get()
    batched = x.dim() == 3
    xb = x.detach() if batched else x.detach().unsqueeze(0)
    b, n = xb.shape[:2]
    k, iters = int(k), int(iters)
    if lib.cffm_kmeans_workspace_bytes(n, k) < 0 or iters < 1:      # K outside 1..128, N < K, iters < 1: the library's own message
        _lib.check(lib.cffm_kmeans(None, n, k, iters, None, None, None, None, None), lib)
    if init is None:
        centers = torch.stack([xb[i][torch.randperm(n, device=x.device)[:k]] for i in range(b)])
    else:
        centers = init.detach().to(device=x.device, dtype=torch.float32).reshape(b, k, 256).clone()
    centers = centers.contiguous()
    labels = torch.empty((b, n), dtype=torch.int32, device=x.device)
    counts = torch.empty((b, k), dtype=torch.int32, device=x.device)
    if ws is None:
        ws = kmeans_workspace(n, k, x.device)
    elif ws.dtype != torch.uint8 or ws.numel() < lib.cffm_kmeans_workspace_bytes(n, k) or ws.device != x.device:
        raise _lib.CffmError('kmeans: workspace too small (kmeans_workspace(n, k, device))')
    for i in range(b):             # (the clips share the workspace: stream order keeps them apart)
        _lib.check(lib.cffm_kmeans(_ptr(xb[i]), n, k, iters, _ptr(centers[i]), _ptr(labels[i]), _ptr(counts[i]), _ptr(ws), _stream(x)), lib)
    if batched:
        return centers, labels, counts
    return centers[0], labels[0], counts[0]
