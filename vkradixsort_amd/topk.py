"""Top-k selection: the k smallest or largest keys of every segment and their positions by radix select (vrs_topk_segments).

topk_segments works on Buffers of a GPUContext; topk is torch.topk(x, k, dim=-1) of a 1-D or 2-D int32 / float32 tensor in the IEEE
total order; torch_topk is the drop-in: sort's nine dtypes, any shape, dim and strides, torch's order.  Both on torch's current stream.
"""
from __future__ import annotations

import ctypes

from . import capi
from ._torch import aligned, buffers, context_for, positions_to_int64, row_offsets
from .capi import VrsError
from .sort import _dtype_code

_KEY_TYPES = {"u32": capi.VRS_TOPK_U32, "i32": capi.VRS_TOPK_I32, "f32": capi.VRS_TOPK_F32}


def scratch_bytes(num_elements: int, num_segments: int, k: int, largest: bool = False, sorted: bool = True) -> int:
    """Bytes of scratch vrs_topk_segments needs for this shape (no device)."""
    flags = (capi.VRS_TOPK_LARGEST if largest else 0) | (capi.VRS_TOPK_SORTED if sorted else 0)
    return capi.query_u64("vrs_topk_scratch_bytes", num_elements, num_segments, k, flags)


def topk_segments(ctx, keys, offsets, num_elements: int, num_segments: int, k: int, out_keys, out_indices=None, scratch=None,
                  key_type: str = "u32", largest: bool = False, sorted: bool = True) -> None:
    """For every segment i = keys[offsets[i], offsets[i+1]) the min(k, length) smallest (largest=True: largest) keys, ties lowest index
    first, into out_keys[i*k ...] and their positions within the segment into out_indices[i*k ...]; slots past the segment's length get
    0xFFFFFFFF.  sorted=True: in that order, else in some order.  key_type "u32", "i32" or "f32" fixes how the bit patterns compare.
    scratch: a Buffer of at least scratch_bytes(...) bytes.  Stream-ordered on the context's stream."""
    if key_type not in _KEY_TYPES:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"key_type must be one of {sorted(_KEY_TYPES)}")
    if scratch is None:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "topk_segments needs a scratch Buffer of scratch_bytes(...) bytes")
    flags = (capi.VRS_TOPK_LARGEST if largest else 0) | (capi.VRS_TOPK_SORTED if sorted else 0)
    ctx.check(ctx.lib.vrs_topk_segments(ctx.handle, keys.handle, num_elements, offsets.handle, num_segments, k, _KEY_TYPES[key_type], flags,
                                        out_keys.handle, out_indices.handle if out_indices is not None else None, scratch.handle))


def topk_stats(ctx) -> dict:
    """Segments the context's top-k calls gave each tier so far (cumulative)."""
    c = [ctypes.c_uint64() for _ in range(3)]
    ctx.check(ctx.lib.vrs_topk_stats(ctx.handle, *(ctypes.byref(v) for v in c)))
    return {"lds": c[0].value, "block": c[1].value, "grid": c[2].value}


def topk(x, k: int, dim: int = -1, largest: bool = True, sorted: bool = True):
    """torch.topk(x, k, dim=-1, largest, sorted) of a contiguous 1-D or 2-D int32 or float32 tensor on a GPU: one call for all rows.

    Returns (values, indices), indices int64 positions within the row.  Ties are broken by the lower index, so the result is that of
    a stable sort of each row, sliced; torch.topk equals it on rows without ties.  Floats compare by the IEEE-754 total order:
    -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN (a NaN with its sign bit set is the smallest key, one without it the largest;
    -0.0 is below +0.0), where torch treats every NaN as the largest value and -0.0 equal to +0.0.  torch_topk is the function that
    follows torch there, and takes every dtype of sort, any dim and any strides."""
    import torch

    if not x.is_cuda:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "topk takes a tensor on a GPU")
    if x.dim() not in (1, 2) or not x.is_contiguous():
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "topk takes a contiguous 1-D or 2-D tensor")
    if dim not in (-1, x.dim() - 1):
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "topk selects along the last dimension only")
    if x.dtype == torch.int32:
        key_type = capi.VRS_TOPK_I32
    elif x.dtype == torch.float32:
        key_type = capi.VRS_TOPK_F32
    else:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"topk takes int32 or float32, not {x.dtype}")
    rows, length = (1, x.shape[0]) if x.dim() == 1 else tuple(x.shape)
    if k < 0 or k > length:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"k = {k} is outside [0, {length}]")
    n = rows * length
    if n >= 1 << 32 or rows * k >= 1 << 32:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "topk takes fewer than 2^32 elements")
    shape = (k,) if x.dim() == 1 else (rows, k)
    device = x.device
    values = torch.empty(shape, dtype=x.dtype, device=device)
    idx = torch.empty(shape, dtype=torch.int32, device=device)
    if k == 0 or rows == 0:
        return values, idx.long()
    ctx = context_for(device)
    flags = (capi.VRS_TOPK_LARGEST if largest else 0) | (capi.VRS_TOPK_SORTED if sorted else 0)
    scratch = torch.empty(max(scratch_bytes(n, rows, k, largest, sorted), 4), dtype=torch.uint8, device=device)
    with buffers(ctx, x, row_offsets(rows, length, device), values, idx, scratch) as (keys, offsets, out_keys, out_idx, scr):
        ctx.check(ctx.lib.vrs_topk_segments(ctx.handle, keys, n, offsets, rows, k, key_type, flags, out_keys, out_idx, scr))
    return values, positions_to_int64(idx, length)


def torch_topk(x, k: int, dim: int = -1, largest: bool = True, sorted: bool = True):
    """torch.topk(x, k, dim, largest, sorted) of a tensor on a GPU (int8, uint8, int16, int32, int64, float16, bfloat16, float32 or
    float64, any shape and strides, fewer than 2^32 elements): a torch.return_types.topk (values, int64 indices) -- the k largest
    (largest=False: smallest) elements of every row along dim in torch's order: NaNs the largest, -0.0 and +0.0 equal, ties lowest index
    first.  Values and indices equal torch.sort(x, dim, descending=largest, stable=True) sliced to k, bit for bit (a NaN keeps its
    payload, a zero its sign); sorted=False: the same set in some order.  torch.topk equals it on rows without ties.  k outside
    [0, the row's length]: RuntimeError."""
    import torch

    if not isinstance(x, torch.Tensor):
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "topk takes a tensor")
    code = _dtype_code(torch, x.dtype, "topk")
    nd = max(x.dim(), 1)
    if not -nd <= dim < nd:
        raise IndexError(f"Dimension out of range (expected to be in range of [{-nd}, {nd - 1}], but got {dim})")
    dim %= nd
    length = x.shape[dim] if x.dim() else 1
    if not 0 <= k <= length:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "selected index k out of range")
    if not x.is_cuda:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "topk takes a tensor on a GPU")
    if x.numel() >= 1 << 32:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "topk takes fewer than 2^32 elements")
    device = x.device
    if x.dim() == 0:  # (as torch: a 0-d tensor is its own answer for k of 0 and of 1, its index 0)
        return torch.return_types.topk((x.clone(), torch.zeros((), dtype=torch.int64, device=device)))
    lead = x.shape[:dim] + x.shape[dim + 1:]  # (the rows' shape: movedim(dim, -1) without its last dim)
    rows = 1
    for s in lead:
        rows *= s
    values = torch.empty(rows * k, dtype=x.dtype, device=device)
    idx = torch.empty(rows * k, dtype=torch.int32, device=device)
    if k and rows:
        xt = aligned(x.movedim(dim, -1).contiguous())  # (a contiguous tensor along its last dim is not copied, unless off a 4-byte boundary)
        n = rows * length
        wide = x.dtype in (torch.int64, torch.float64)
        flags = (capi.VRS_TOPK_LARGEST if largest else 0) | (capi.VRS_TOPK_SORTED if sorted else 0) | (capi.VRS_TOPK_RANK64 if wide else 0)
        ctx = context_for(device)
        scratch = torch.empty(max(capi.query_u64("vrs_topk_scratch_bytes", n, rows, k, flags), 8), dtype=torch.uint8, device=device)
        with buffers(ctx, xt, row_offsets(rows, length, device), values, idx, scratch) as (keys, offsets, out_keys, out_idx, scr):
            ctx.check(ctx.lib.vrs_topk_segments(ctx.handle, keys, n, offsets, rows, k, capi.VRS_TOPK_DTYPE(code), flags, out_keys, out_idx, scr))
    shape = tuple(lead) + (k,)
    out_v, out_i = values.view(shape).movedim(-1, dim), positions_to_int64(idx, length).view(shape).movedim(-1, dim)
    return torch.return_types.topk((out_v, out_i))
