"""torch.mode drop-in: the most frequent value of every row along a dim and an index where it sits, nine dtypes, any dim.

Three steps on torch's current stream, none of which waits for the device: vrs_sort_rank_keys maps every element to its rank in torch's
order (no positions), a sort of bare keys sorts each row's ranks (vrs_sort_segments_u32 / _u64; one row: vrs_sort_keys_u32 / _u64), and
vrs_sort_restore with VRS_SORT_MODE finds the longest run of every sorted row and, reading the input once more, the last place the
run's value sits.  No position payload goes through the sort: mode wants one index per row, not one per element.
"""
from __future__ import annotations

from . import capi
from ._torch import aligned, buffers, context_for, row_offsets
from .capi import VrsError
from .sort import _dtype_code


def mode(x, dim: int = -1, keepdim: bool = False):
    """torch.mode(x, dim, keepdim) of a tensor on a GPU (int8, uint8, int16, int32, int64, float16, bfloat16, float32 or float64, any
    shape and strides, fewer than 2^32 elements): a torch.return_types.mode (values, int64 indices).

    values: the most frequent value of every row along dim, the smallest of them where several are equally frequent -- equal to
    torch.mode's on the CPU for NaN-free input (torch's GPU mode answers any of the most frequent values).  indices: a valid occurrence, x.gather(dim, indices) == values; here always the LAST one, where
    torch's choice is unspecified.  -0.0 and +0.0 count as one value and all NaNs as one value, the largest, as in this package's sort,
    kthvalue and median; the value returned carries the bits of the element at the index (a zero's sign, a NaN's payload)."""
    import torch

    if not isinstance(x, torch.Tensor):
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "mode takes a tensor on a GPU")
    # what the arguments alone decide comes first, the device last: these refusals are the same on every machine
    code = _dtype_code(torch, x.dtype, "mode")
    nd = max(x.dim(), 1)
    if not -nd <= dim < nd:
        raise IndexError(f"Dimension out of range (expected to be in range of [{-nd}, {nd - 1}], but got {dim})")
    if x.dim() and x.shape[dim] == 0:  # an empty reduced dim: torch's own refusal, by torch itself (an empty CPU tensor of this shape)
        torch.mode(torch.empty(x.shape, dtype=x.dtype), dim, keepdim)
        raise IndexError(f"mode(): Expected reduction dim {dim} to have non-zero size.")
    if not x.is_cuda:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "mode takes a tensor on a GPU")
    n = x.numel()
    if n >= 1 << 32:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "mode takes fewer than 2^32 elements")
    device = x.device
    if x.dim() == 0:  # (as torch: a 0-d tensor answers itself, its index 0)
        return torch.return_types.mode((x.clone(), torch.zeros((), dtype=torch.int64, device=device)))
    dim %= x.dim()
    xt = aligned(x.movedim(dim, -1).contiguous())
    L = xt.shape[-1]
    rows = n // L
    out_shape = xt.shape[:-1]
    values = torch.empty(out_shape, dtype=x.dtype, device=device)
    indices = torch.empty(out_shape, dtype=torch.int64, device=device)
    if n:
        wide = x.dtype in (torch.int64, torch.float64)
        rdt = torch.int64 if wide else torch.int32
        ranks = torch.empty(n, dtype=rdt, device=device)
        ranks_tmp = torch.empty(n if L > 1 else 0, dtype=rdt, device=device)
        scratch = torch.empty(rows, dtype=torch.int64, device=device)
        offsets = row_offsets(rows, L, device) if rows > 1 and L > 1 else None
        ctx = context_for(device)
        lib = ctx.lib
        with buffers(ctx, xt, ranks, ranks_tmp, scratch, values, indices, offsets) as (src, rk, rk_tmp, scr, vals, idx, offs):
            ctx.check(lib.vrs_sort_rank_keys(ctx.handle, src, n, L, code, 0, rk, None))
            if L > 1:
                w = "u64" if wide else "u32"
                if rows == 1:
                    ctx.check(getattr(lib, f"vrs_sort_keys_{w}")(ctx.handle, rk, rk_tmp, n))
                else:
                    ctx.check(getattr(lib, f"vrs_sort_segments_{w}")(ctx.handle, rk, rk_tmp, n, offs, rows))
            ctx.check(lib.vrs_sort_restore(ctx.handle, src, rk, scr, n, L, code, capi.VRS_SORT_MODE, vals, idx))
    if keepdim:
        values, indices = values.unsqueeze(dim), indices.unsqueeze(dim)
    return torch.return_types.mode((values, indices))
