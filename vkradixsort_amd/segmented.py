"""Segmented sorts: many independent segments of one buffer sorted by one call (vrs_sort_segments_u32 / vrs_sort_segments_pairs_u32).

sort_segments works on Buffers of a GPUContext; sort_rows is the torch.sort(x, dim=-1, stable=True) of a 2-D int32 / float32 tensor,
on torch's current stream.
"""
from __future__ import annotations

import ctypes

from . import capi
from ._torch import buffers, context_for, positions_to_int64, row_offsets
from .capi import VrsError


def sort_segments(ctx, keys, keys_tmp, offsets, num_elements: int, num_segments: int, values=None, values_tmp=None) -> None:
    """Sorts segment i = keys[offsets[i], offsets[i+1]) for every i < num_segments, ascending, in place (uint32 keys).  With values /
    values_tmp the payloads follow their keys and equal keys keep their input order.  keys_tmp / values_tmp are scratch of
    num_elements entries.  Stream-ordered on the context's stream."""
    lib = ctx.lib
    if values is None and values_tmp is None:
        ctx.check(lib.vrs_sort_segments_u32(ctx.handle, keys.handle, keys_tmp.handle, num_elements, offsets.handle, num_segments))
        return
    if values is None or values_tmp is None:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "values and values_tmp go together")
    ctx.check(lib.vrs_sort_segments_pairs_u32(ctx.handle, keys.handle, keys_tmp.handle, values.handle, values_tmp.handle, num_elements,
                                              offsets.handle, num_segments))


def segmented_stats(ctx) -> dict:
    """Segments the context's segmented sorts gave each tier so far (cumulative)."""
    c = [ctypes.c_uint64() for _ in range(4)]
    ctx.check(ctx.lib.vrs_segmented_stats(ctx.handle, *(ctypes.byref(v) for v in c)))
    return {"wave": c[0].value, "block": c[1].value, "global": c[2].value, "one_call": c[3].value}


def sort_rows(x, return_indices: bool = False):
    """Every row of a contiguous 2-D int32 or float32 tensor on a GPU sorted ascending, one call for all rows.

    Returns the sorted tensor, or (values, indices) with return_indices=True; indices are int64 positions within the row, as
    torch.sort's.  The result equals torch.sort(x, dim=-1, stable=True) for inputs without NaN and without -0.0.  For those two the
    library sorts by the IEEE-754 total order: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN (a NaN with its sign bit set first,
    one without it last; -0.0 before +0.0), where torch puts every NaN last and keeps -0.0 and +0.0 in input order."""
    import torch

    if x.dim() != 2 or not x.is_contiguous() or not x.is_cuda:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "sort_rows takes a contiguous 2-D tensor on a GPU")
    if x.dtype == torch.int32:
        to_keys, from_keys = capi.VRS_KEYS_INT32, capi.VRS_KEYS_INT32
    elif x.dtype == torch.float32:
        to_keys, from_keys = capi.VRS_KEYS_FLOAT32_TO_SORTABLE, capi.VRS_KEYS_SORTABLE_TO_FLOAT32
    else:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"sort_rows takes int32 or float32, not {x.dtype}")
    rows, length = x.shape
    n = rows * length
    if n >= 1 << 32:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "sort_rows takes fewer than 2^32 elements")
    device = x.device
    out = x.clone()
    idx = torch.arange(length, dtype=torch.int32, device=device).repeat(rows) if return_indices else None
    if n == 0:
        return (out, torch.zeros_like(out, dtype=torch.int64)) if return_indices else out
    ctx = context_for(device)
    idx_tmp = torch.empty_like(idx) if return_indices else None
    with buffers(ctx, out, torch.empty_like(out), row_offsets(rows, length, device), idx, idx_tmp) as h:
        keys, keys_tmp, offsets, vals, vals_tmp = h
        ctx.check(ctx.lib.vrs_transform_keys(ctx.handle, keys, n, to_keys))
        if return_indices:
            ctx.check(ctx.lib.vrs_sort_segments_pairs_u32(ctx.handle, keys, keys_tmp, vals, vals_tmp, n, offsets, rows))
        else:
            ctx.check(ctx.lib.vrs_sort_segments_u32(ctx.handle, keys, keys_tmp, n, offsets, rows))
        ctx.check(ctx.lib.vrs_transform_keys(ctx.handle, keys, n, from_keys))
    return (out, positions_to_int64(idx.view(rows, length), length)) if return_indices else out
