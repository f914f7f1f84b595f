"""torch.repeat_interleave drop-in: run-length decode (the identity form of vrs_search_sorted).

The inverse of run_length_encode / unique_consecutive(return_counts=True): counts back to one entry per element, which is also the CSR
row expansion and the batch vector of a ragged batch.  Three steps on torch's current stream:
    ends  = cumsum(repeats)                    the library's scan, to int64
    index = the identity search of `ends`      vrs_search_sorted(queries = NULL, VRS_SEARCH_RIGHT): output j is the number of run ends
                                               <= j, which is the run of output j.  A merge: the ends are read once and the indices
                                               written once, no arange is made and nothing is searched per output.
    out   = input.index_select(dim, index)     torch plumbing: vrs_search_sorted has no operand that could carry values through the
                                               search, so the rows are gathered by torch from the indices.
Without output_size the call reads (min, total) of `repeats` from the device once, as torch reads the total; with output_size it reads
nothing and never waits for the device.
"""
from __future__ import annotations

from . import capi
from ._torch import buffers, context_for
from .capi import VrsError
from .scan import cumsum


def _refuse(message: str):
    raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, message)


def _run_index(repeats, output_size):
    """The one-argument form for a checked 1-D int32 / int64 `repeats` on a GPU: the run of every output, in repeats' dtype."""
    import torch

    m, device = repeats.numel(), repeats.device
    if m == 0:
        return torch.empty_like(repeats, memory_format=torch.contiguous_format)
    if m >= 1 << 32:
        _refuse("repeat_interleave takes fewer than 2^32 repeats")
    ends = cumsum(repeats, 0)  # int64 (int32 repeats are widened by the scan's load)
    if output_size is None:
        lowest, total = torch.stack((repeats.min().to(torch.int64), ends[-1])).tolist()  # the call's one host read
        if lowest < 0:
            raise RuntimeError("repeats can not be negative")
    else:
        total = output_size
    if total >= 1 << 32:
        _refuse("repeat_interleave gives fewer than 2^32 elements")
    index = torch.empty(total, dtype=repeats.dtype, device=device)
    if total == 0:
        return index
    flags = capi.VRS_SEARCH_RIGHT | (capi.VRS_SEARCH_OUT_INT64 if repeats.dtype == torch.int64 else 0)
    ctx = context_for(device)
    with buffers(ctx, ends, index) as (bnd, res):
        ctx.check(ctx.lib.vrs_search_sorted(ctx.handle, bnd, m, m, None, total, total, capi.VRS_SORT_INT64, flags, None, res, None))
    if output_size is not None:
        # outputs past the true total (a caller's error, as in torch on a GPU) count every end: m.  One op keeps them inside the input.
        index.clamp_(max=m - 1)
    return index


def repeat_interleave(input, repeats=None, dim=None, *, output_size=None):
    """torch.repeat_interleave(input, repeats=None, dim=None, *, output_size=None) of tensors on a GPU, equal to torch's CPU result in
    values, shape and dtype.

    repeat_interleave(repeats): the index of each output's run -- [1, 0, 2] gives [0, 2, 2] -- in repeats' dtype (int32 or int64, 1-D).
    repeat_interleave(input, repeats, dim): element i along dim (of the flattened input without dim) repeated repeats[i] times; `repeats`
    a Python int (views and one copy by torch, no kernel of this library), or an int32 / int64 tensor that is 0-d, has one element
    (both broadcast) or input.size(dim) elements.  `input` may have any dtype and strides; its bits are copied (a NaN keeps its payload).
    output_size: the total, when the caller knows it; the call then reads nothing from the device.  A wrong output_size is the caller's
    error, as in torch on a GPU: outputs past the true total repeat the last element, none is read out of range.
    A negative repeat (found by the host read, so without output_size), a repeats of another dtype, shape or length: RuntimeError, as
    torch.  CPU tensors, and totals of 2^32 or more: VrsError."""
    import torch

    if not isinstance(input, torch.Tensor):
        raise TypeError("repeat_interleave takes a tensor as input")
    if output_size is not None and (isinstance(output_size, bool) or not isinstance(output_size, int) or output_size < 0):
        raise TypeError("output_size must be a non-negative int")
    if repeats is None:  # the one-argument form: input is the repeats
        if dim is not None:
            raise TypeError("repeat_interleave(repeats) takes no dim")
        if input.dim() != 1:
            raise RuntimeError("repeat_interleave only accept 1D vector as repeat")
        if input.dtype not in (torch.int32, torch.int64):
            raise RuntimeError("repeats has to be Long or Int tensor")
        if not input.is_cuda:
            _refuse("repeat_interleave takes tensors on a GPU")
        return _run_index(input, output_size)
    if dim is not None:
        nd = max(input.dim(), 1)
        if isinstance(dim, bool) or not isinstance(dim, int):
            raise TypeError("dim must be an int")
        if not -nd <= dim < nd:
            raise IndexError(f"Dimension out of range (expected to be in range of [{-nd}, {nd - 1}], but got {dim})")
    if isinstance(repeats, torch.Tensor):
        if repeats.dim() > 1:
            raise RuntimeError("repeats must be 0-dim or 1-dim tensor")
        if repeats.dtype not in (torch.int32, torch.int64):
            raise RuntimeError("repeats has to be Long or Int tensor")
    elif isinstance(repeats, bool) or not isinstance(repeats, int):
        raise TypeError("repeats must be an int or a tensor")
    elif repeats < 0:
        raise RuntimeError("Repeats must be non-negative")
    if not input.is_cuda or (isinstance(repeats, torch.Tensor) and not repeats.is_cuda):
        _refuse("repeat_interleave takes tensors on a GPU")
    if isinstance(repeats, torch.Tensor) and repeats.device != input.device:
        _refuse("repeat_interleave takes tensors on one device")
    src = input.flatten() if dim is None else (input.unsqueeze(0) if input.dim() == 0 else input)
    d = 0 if dim is None else dim % src.dim()
    size = src.shape[d]
    if not isinstance(repeats, torch.Tensor):
        if output_size is not None and output_size != size * repeats:
            raise RuntimeError(f"repeat_interleave: Invalid output_size, expected {size * repeats} but got {output_size}")
        shape = list(src.shape)
        shape[d] = size * repeats
        out = src.unsqueeze(d + 1).expand(*src.shape[:d + 1], repeats, *src.shape[d + 1:]).reshape(shape)
        return out.clone() if out.data_ptr() == src.data_ptr() and out.numel() else out  # (never a view of the input)
    if repeats.numel() == 1:  # 0-d or one element: every element that many times
        repeats = repeats.reshape(1).expand(size)
    elif repeats.shape[0] != size:
        raise RuntimeError(f"repeats must have the same size as input along dim, but got repeats.size(0) = {repeats.shape[0]} "
                           f"and input.size({d}) = {size}")
    return src.index_select(d, _run_index(repeats, output_size))
