"""torch.searchsorted and torch.bucketize drop-ins: where each value of `input` goes in a sorted sequence (vrs_search_sorted).

One call on torch's current stream.  The library picks a tier from the shape (vrs_search_plan): boundaries that fit a workgroup's LDS
are searched there, 1- and 2-byte dtypes with many queries through a table of every bit pattern's answer, long sequences with many
queries through a sampled index built by the call, everything else by a plain binary search in global memory.
"""
from __future__ import annotations

import ctypes

from . import capi
from ._torch import aligned, buffers, context_for
from .capi import VrsError
from .sort import _dtype_code

TIER_NAMES = {capi.VRS_SEARCH_LDS: "lds", capi.VRS_SEARCH_TABLE: "table", capi.VRS_SEARCH_DIRECT: "direct", capi.VRS_SEARCH_INDEXED: "indexed"}


def _refuse(message: str):
    raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, message)


def search_stats(ctx) -> dict:
    """Calls the context's searches ran in each tier so far (cumulative; counted on the host)."""
    c = [ctypes.c_uint64() for _ in range(4)]
    ctx.check(ctx.lib.vrs_search_stats(ctx.handle, *(ctypes.byref(v) for v in c)))
    return {name: c[tier].value for tier, name in TIER_NAMES.items()}


def searchsorted(sorted_sequence, input, *, out_int32: bool = False, right: bool = False, side=None, sorter=None):
    """torch.searchsorted(sorted_sequence, input, out_int32=, right=, side=, sorter=) of tensors on a GPU: for every value v of `input`
    the number of elements b of its row of `sorted_sequence` with b < v (right / side='right': b <= v), int64 unless out_int32, in the
    shape of `input`.

    Nine dtypes (int8, uint8, int16, int32, int64, float16, bfloat16, float32, float64) in torch.sort's order: -0.0 equals +0.0 and
    every NaN equals every other NaN and is above +inf.  Equal to numpy.searchsorted always and to torch.searchsorted whenever the
    sequence holds no NaN (NaN values of `input` get the sequence's length, or the first NaN's position from the left); with NaNs in
    the sequence torch's answer depends on which midpoints its binary search visits ([1, 2, 3, nan, nan] and 4.0: torch 5, here and
    numpy 3).  A sequence that is not ascending gives some position within [0, length] per value, as torch.
    Shapes as torch: a 1-D sequence with an input of any shape (a Python number too), or a sequence and an input that differ in
    their last dimension only.  `sorter`: int64 indices of the sequence's shape that sort it along its last dimension.  An input of
    another dtype (or a number) is promoted with the sequence as torch does (torch.result_type, then .to()); non-contiguous tensors
    and 1- or 2-byte views that start off a 4-byte boundary are made contiguous and aligned first (one copy).  Refusals are VrsError and come before any device work."""
    import torch

    if not isinstance(sorted_sequence, torch.Tensor):
        _refuse("searchsorted takes a tensor as sorted_sequence")
    if side is not None:
        if side not in ("left", "right"):
            _refuse(f"side must be 'left' or 'right', not {side!r}")
        if side == "left" and right:
            _refuse("side='left' and right=True contradict each other")
        right = side == "right"
    seq = sorted_sequence
    if seq.dim() == 0:
        _refuse("sorted_sequence must have at least one dimension")
    scalar = not isinstance(input, torch.Tensor)
    if scalar:
        if isinstance(input, bool) or not isinstance(input, (int, float)):
            _refuse("input must be a tensor or a Python number")
        if seq.dim() != 1:
            _refuse("a Python number searches a 1-D sorted_sequence only")
    elif seq.dim() != 1 and (seq.dim() != input.dim() or seq.shape[:-1] != input.shape[:-1]):
        _refuse(f"sorted_sequence must be 1-D or match input in every dimension but the last: {tuple(seq.shape)} and {tuple(input.shape)}")
    if sorter is not None:
        if not isinstance(sorter, torch.Tensor) or sorter.dtype != torch.int64:
            _refuse("sorter must be an int64 tensor")
        if sorter.shape != seq.shape:
            _refuse(f"sorter must have sorted_sequence's shape: {tuple(sorter.shape)} and {tuple(seq.shape)}")
    common = torch.result_type(seq, input)
    code = _dtype_code(torch, common)  # (refuses a promoted dtype outside the nine)
    if not seq.is_cuda or (not scalar and not input.is_cuda) or (sorter is not None and not sorter.is_cuda):
        _refuse("searchsorted takes tensors on a GPU")
    device = seq.device
    if (not scalar and input.device != device) or (sorter is not None and sorter.device != device):
        _refuse("sorted_sequence, input and sorter must be on one device")
    if seq.numel() >= 1 << 32 or (not scalar and input.numel() >= 1 << 32):
        _refuse("searchsorted takes fewer than 2^32 elements on either side")
    values = torch.tensor(input, dtype=common, device=device) if scalar else input
    seq_c, values_c = aligned(seq.to(common).contiguous()), aligned(values.to(common).contiguous())
    sorter_c = sorter.contiguous() if sorter is not None else None
    out = torch.empty(values_c.shape, dtype=torch.int32 if out_int32 else torch.int64, device=device)
    nq, nb = values_c.numel(), seq_c.numel()
    if nq == 0:
        return out
    m = seq_c.shape[-1]
    q_len = nq if seq_c.dim() == 1 else values_c.shape[-1]
    flags = (capi.VRS_SEARCH_RIGHT if right else 0) | (0 if out_int32 else capi.VRS_SEARCH_OUT_INT64)
    ctx = context_for(device)
    lib = ctx.lib
    tier, need = ctypes.c_int(), ctypes.c_uint64()
    ctx.check(lib.vrs_search_plan(ctx.handle, nb, m, nq, q_len, code, int(sorter_c is not None), ctypes.byref(tier), ctypes.byref(need)))
    scratch = torch.empty(need.value, dtype=torch.uint8, device=device) if need.value else None
    with buffers(ctx, seq_c, values_c, sorter_c, out, scratch) as (bnd, qry, srt, res, scr):
        ctx.check(lib.vrs_search_sorted(ctx.handle, bnd, nb, m, qry, nq, q_len, code, flags, srt, res, scr))
    return out


def bucketize(input, boundaries, *, out_int32: bool = False, right: bool = False):
    """torch.bucketize(input, boundaries, out_int32=, right=): searchsorted(boundaries, input, ...) for 1-D boundaries."""
    import torch

    if not isinstance(boundaries, torch.Tensor) or boundaries.dim() != 1:
        _refuse("bucketize takes 1-D boundaries")
    return searchsorted(boundaries, input, out_int32=out_int32, right=right)
