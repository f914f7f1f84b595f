"""torch.sort and torch.argsort drop-ins: any dim, ascending or descending, nine dtypes, equal to torch's stable sort bit for bit.

Three steps on torch's current stream: vrs_sort_rank_keys maps every element to its rank in torch's order (and its position in the row),
a stable segmented sort sorts each row's ranks (vrs_sort_segments_(pairs_)u32 / _u64; one row: the one-call sort), and vrs_sort_restore
writes the values back from the sorted ranks and the int64 indices from the positions.
"""
from __future__ import annotations

from . import capi
from ._torch import aligned, buffers, context_for, row_offsets
from .capi import VrsError


def _dtype_code(torch, dtype, name: str = "sort"):
    codes = {torch.int8: capi.VRS_SORT_INT8, torch.uint8: capi.VRS_SORT_UINT8, torch.int16: capi.VRS_SORT_INT16,
             torch.int32: capi.VRS_SORT_INT32, torch.int64: capi.VRS_SORT_INT64, torch.float16: capi.VRS_SORT_FLOAT16,
             torch.bfloat16: capi.VRS_SORT_BFLOAT16, torch.float32: capi.VRS_SORT_FLOAT32, torch.float64: capi.VRS_SORT_FLOAT64}
    if dtype not in codes:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes int8, uint8, int16, int32, int64, float16, bfloat16, float32 or "
                                                        f"float64, not {dtype}")
    return codes[dtype]


def _run(x, dim: int, descending: bool, want_values: bool, want_indices: bool):
    """(values or None, int64 indices or None) of the stable sort of x along dim."""
    import torch

    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "sort takes a tensor on a GPU")
    code = _dtype_code(torch, x.dtype)
    nd = max(x.dim(), 1)
    if not -nd <= dim < nd:
        raise IndexError(f"Dimension out of range (expected to be in range of [{-nd}, {nd - 1}], but got {dim})")
    n = x.numel()
    if n >= 1 << 32:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "sort takes fewer than 2^32 elements")
    device = x.device
    if x.dim() == 0 or n == 0:  # (as torch: a 0-d tensor is its own sort, its index 0)
        return (x.clone() if want_values else None), (torch.zeros(x.shape, dtype=torch.int64, device=device) if want_indices else None)
    dim %= x.dim()
    xt = aligned(x.movedim(dim, -1).contiguous())  # (a contiguous tensor sorted along its last dim is not copied, unless off a 4-byte boundary)
    L = xt.shape[-1]
    rows = n // L
    is_float = x.dtype.is_floating_point
    wide = x.dtype in (torch.int64, torch.float64)
    with_pos = want_indices or is_float  # the indices, or the exact bits of a float's ±0.0 and NaN (an integer's values alone: bare keys)
    rdt = torch.int64 if wide else torch.int32
    flags = capi.VRS_SORT_DESCENDING if descending else 0
    ranks, ranks_tmp = torch.empty(n, dtype=rdt, device=device), torch.empty(n, dtype=rdt, device=device)
    pos = torch.empty(n if with_pos else 0, dtype=torch.int32, device=device)
    pos_tmp = torch.empty_like(pos)
    values = torch.empty(n if want_values else 0, dtype=x.dtype, device=device)
    indices = torch.empty(n if want_indices else 0, dtype=torch.int64, device=device)
    offsets = row_offsets(rows, L, device) if rows > 1 and L > 1 else None
    ctx = context_for(device)
    lib = ctx.lib
    with buffers(ctx, xt, ranks, ranks_tmp, pos, pos_tmp, values, indices, offsets) as (src, rk, rk_tmp, ps, ps_tmp, vals, idx, offs):
        ctx.check(lib.vrs_sort_rank_keys(ctx.handle, src, n, L, code, flags, rk, ps))
        if L > 1:
            w = "u64" if wide else "u32"
            if rows == 1:
                if with_pos:
                    ctx.check(getattr(lib, f"vrs_sort_pairs_{w}")(ctx.handle, rk, rk_tmp, ps, ps_tmp, n))
                else:
                    ctx.check(getattr(lib, f"vrs_sort_keys_{w}")(ctx.handle, rk, rk_tmp, n))
            elif with_pos:
                ctx.check(getattr(lib, f"vrs_sort_segments_pairs_{w}")(ctx.handle, rk, rk_tmp, ps, ps_tmp, n, offs, rows))
            else:
                ctx.check(getattr(lib, f"vrs_sort_segments_{w}")(ctx.handle, rk, rk_tmp, n, offs, rows))
        ctx.check(lib.vrs_sort_restore(ctx.handle, src, rk, ps, n, L, code, flags, vals, idx))
    shape = xt.shape
    out_v = values.view(shape).movedim(-1, dim) if want_values else None
    out_i = indices.view(shape).movedim(-1, dim) if want_indices else None
    return out_v, out_i


def sort(x, dim: int = -1, descending: bool = False, stable: bool = False):
    """torch.sort(x, dim, descending, stable) of a tensor on a GPU (int8, uint8, int16, int32, int64, float16, bfloat16, float32 or
    float64, any shape and strides, fewer than 2^32 elements): a torch.return_types.sort (values, int64 indices) equal to
    torch.sort(x, dim, descending, stable=True) bit for bit -- NaNs last (first when descending), -0.0 and +0.0 equal, equal keys in
    input order.  The result is always stable, which is a valid answer to stable=False."""
    import torch

    return torch.return_types.sort(_run(x, dim, descending, True, True))


def sort_values(x, dim: int = -1, descending: bool = False):
    """sort(x, dim, descending).values without the indices: integers are then sorted as bare keys (no position payload)."""
    return _run(x, dim, descending, True, False)[0]


def argsort(x, dim: int = -1, descending: bool = False, stable: bool = False):
    """torch.argsort(x, dim, descending, stable) of a tensor on a GPU: the int64 indices of sort(x, dim, descending), without writing
    the values."""
    return _run(x, dim, descending, False, True)[1]
