"""torch.kthvalue, torch.median and torch.nanmedian drop-ins: one entry of every row's sorted order by a one-rank radix select
(vrs_select_segments), without sorting the row.

select_segments works on Buffers of a GPUContext; kthvalue, median and nanmedian take torch tensors of sort's nine dtypes, any shape, dim
and strides, on torch's current stream.  Values equal torch's; the indices are those of the stable order (where torch leaves the index
of a tie unspecified).
"""
from __future__ import annotations

import ctypes

from . import capi
from ._torch import aligned, buffers, context_for, positions_to_int64, row_offsets
from .capi import VrsError
from .sort import _dtype_code

_MODES = {"kth": capi.VRS_SELECT_KTH, "median": capi.VRS_SELECT_MEDIAN, "nanmedian": capi.VRS_SELECT_NANMEDIAN}
TIER_NAMES = {capi.VRS_SELECT_LDS: "lds", capi.VRS_SELECT_BLOCK: "block", capi.VRS_SELECT_GRID: "grid"}


def select_scratch_bytes(num_elements: int, num_segments: int, dtype: int) -> int:
    """Bytes of scratch vrs_select_segments needs for this shape and dtype (a capi.VRS_SORT_* code); no device."""
    return capi.query_u64("vrs_select_scratch_bytes", num_elements, num_segments, dtype)


def select_segments(ctx, src, offsets, num_elements: int, num_segments: int, dtype: int, out_values, out_indices=None, scratch=None,
                    mode: str = "kth", k: int = 1, descending: bool = False) -> None:
    """For every segment i = src[offsets[i], offsets[i+1]) of elements of `dtype` (a capi.VRS_SORT_* code) entry j of its stable
    ascending (descending=True: descending) order in torch's order: the element's own bits into out_values[i] and its position within
    the segment into out_indices[i] (uint32; 0xFFFFFFFF and zero bits for a segment without such an entry).  mode "kth": j = k - 1;
    "median": the lower median, the first NaN when the segment has one; "nanmedian": the lower median of the non-NaN elements.
    scratch: a Buffer of at least select_scratch_bytes(...) bytes.  Stream-ordered on the context's stream."""
    if mode not in _MODES:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"mode must be one of {sorted(_MODES)}")
    if scratch is None:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "select_segments needs a scratch Buffer of select_scratch_bytes(...) bytes")
    flags = capi.VRS_SELECT_DESCENDING if descending else 0
    ctx.check(ctx.lib.vrs_select_segments(ctx.handle, src.handle, num_elements, offsets.handle, num_segments, dtype, _MODES[mode], k, flags,
                                          out_values.handle, out_indices.handle if out_indices is not None else None, scratch.handle))


def select_stats(ctx) -> dict:
    """Segments the context's selections gave each tier so far, and the grid-tier segments that compacted (cumulative)."""
    c = [ctypes.c_uint64() for _ in range(4)]
    ctx.check(ctx.lib.vrs_select_stats(ctx.handle, *(ctypes.byref(v) for v in c)))
    return {"lds": c[0].value, "block": c[1].value, "grid": c[2].value, "compacted": c[3].value}


def _check(torch, name, x, dim, k=None):
    """What is refused before any device work, in torch's order: the dtype, the dim, an empty reduction dim, k.  Returns (dtype code, dim)."""
    if not isinstance(x, torch.Tensor):
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes a tensor")
    code = _dtype_code(torch, x.dtype, name)
    nd = max(x.dim(), 1)
    if not -nd <= dim < nd:
        raise IndexError(f"Dimension out of range (expected to be in range of [{-nd}, {nd - 1}], but got {dim})")
    dim %= nd
    length = x.shape[dim] if x.dim() else 1
    if length == 0:
        raise IndexError(f"{name}(): Expected reduction dim {dim} to have non-zero size.")
    if k is not None and not 1 <= k <= length:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name}(): selected number k out of range for dimension {dim}")
    if not x.is_cuda:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes a tensor on a GPU")
    if x.numel() >= 1 << 32:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes fewer than 2^32 elements")
    return code, dim


def _along(x, code: int, dim: int, keepdim: bool, mode: int, k: int):
    """(values, int64 indices) of the selection along dim of a checked tensor: one segment per row of movedim(dim, -1)."""
    import torch

    device = x.device
    if x.dim() == 0:  # (as torch: a 0-d tensor is its own answer, its index 0)
        return x.clone(), torch.zeros((), dtype=torch.int64, device=device)
    xt = aligned(x.movedim(dim, -1).contiguous())  # (a contiguous tensor reduced along its last dim is not copied, unless off a 4-byte boundary)
    length = xt.shape[-1]
    n = xt.numel()
    rows = n // length
    values = torch.empty(rows, dtype=x.dtype, device=device)
    idx = torch.empty(rows, dtype=torch.int32, device=device)
    if rows:
        ctx = context_for(device)
        scratch = torch.empty(max(select_scratch_bytes(n, rows, code), 8), dtype=torch.uint8, device=device)
        with buffers(ctx, xt, row_offsets(rows, length, device), values, idx, scratch) as (src, offsets, out_v, out_i, scr):
            ctx.check(ctx.lib.vrs_select_segments(ctx.handle, src, n, offsets, rows, code, mode, k, 0, out_v, out_i, scr))
    shape = xt.shape[:-1]
    out_v, out_i = values.view(shape), positions_to_int64(idx, length).view(shape)
    return (out_v.unsqueeze(dim), out_i.unsqueeze(dim)) if keepdim else (out_v, out_i)


def kthvalue(x, k: int, dim: int = -1, keepdim: bool = False):
    """torch.kthvalue(x, k, dim, keepdim) of a tensor on a GPU (int8, uint8, int16, int32, int64, float16, bfloat16, float32 or float64,
    any shape and strides, fewer than 2^32 elements): a torch.return_types.kthvalue (values, int64 indices) -- the k-th smallest element
    of every row along dim (1 <= k <= the row's length, else RuntimeError), NaNs the largest, -0.0 and +0.0 equal.  Values equal
    torch's; indices are those of the stable order: of equal elements the one at position k - 1 of torch.sort(x, dim, stable=True),
    where torch leaves the index of a tie unspecified."""
    import torch

    code, dim = _check(torch, "kthvalue", x, dim, k)
    return torch.return_types.kthvalue(_along(x, code, dim, keepdim, capi.VRS_SELECT_KTH, k))


def _median(name: str, x, dim, keepdim: bool):
    import torch

    mode = _MODES[name]
    if dim is not None:
        code, dim = _check(torch, name, x, dim)
        return getattr(torch.return_types, name)(_along(x, code, dim, keepdim, mode, 0))
    if isinstance(x, torch.Tensor) and x.numel() == 0:  # (as torch: NaN; it answers an integer tensor with no defined value, this refuses)
        _dtype_code(torch, x.dtype, name)
        if not x.dtype.is_floating_point:
            raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} of an empty integer tensor has no value")
        return torch.full((), float("nan"), dtype=x.dtype, device=x.device)
    flat = x.reshape(-1) if isinstance(x, torch.Tensor) else x
    code, _ = _check(torch, name, flat, 0)
    return _along(flat, code, 0, False, mode, 0)[0]


def median(x, dim=None, keepdim: bool = False):
    """torch.median of a tensor on a GPU (the dtypes, shapes and sizes of kthvalue).  median(x): the lower median of all elements as a
    0-d tensor (NaN for an empty float tensor).  median(x, dim, keepdim): a torch.return_types.median (values, int64 indices) along dim
    (a dim of size 0: IndexError).  A row with any NaN answers NaN.  Values equal torch's; indices are those of the stable order: the
    element at position (L - 1) // 2 of torch.sort(x, dim, stable=True), the first NaN of a row that has one -- where torch leaves the
    index of a tie unspecified (torch on the CPU answers the second of two NaNs)."""
    return _median("median", x, dim, keepdim)


def nanmedian(x, dim=None, keepdim: bool = False):
    """torch.nanmedian of a tensor on a GPU: median(x, dim, keepdim) over the elements of every row that are not NaN; a row of NaNs alone
    answers NaN (its first).  Integer dtypes: the same as median.  Values equal torch's; indices are those of the stable order."""
    return _median("nanmedian", x, dim, keepdim)
