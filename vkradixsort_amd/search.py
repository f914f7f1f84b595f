"""torch.searchsorted, torch.bucketize and torch.isin drop-ins: where each value of `input` goes in a sorted sequence, and whether it
is there at all (vrs_search_sorted and its membership form).

One call on torch's current stream.  The library picks a tier from the shape (vrs_search_plan): boundaries that fit a workgroup's LDS
are searched there, 1- and 2-byte dtypes with many queries through a table of every bit pattern's answer, long sequences with many
queries through a sampled index built by the call, everything else by a plain binary search in global memory.
"""
from __future__ import annotations

import ctypes

from . import capi
from ._torch import aligned, buffers, context_for
from .capi import VrsError
from .sort import _dtype_code, sort_values

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


def isin(elements, test_elements, *, assume_unique: bool = False, invert: bool = False):
    """torch.isin(elements, test_elements, assume_unique=, invert=) of tensors on a GPU: a torch.bool tensor of elements' shape, True
    where the element equals some test element (invert: where it equals none); equal to torch.isin on the CPU bit for bit.

    Two steps on torch's current stream: this library's sort of the flattened test set (values only), then one vrs_search_sorted call
    in its membership form (VRS_SEARCH_MEMBER, with VRS_SEARCH_MEMBER_INVERT for invert=True) that writes the bool result itself -- no
    index tensor, no gather, no logical_not.  The tier and the scratch are those vrs_search_plan reports for the shapes.
    Either argument may be a Python number, not both; a number as `elements` gives a 0-dim result.  Both sides are converted to
    torch.result_type(elements, test_elements) as torch does, which must be one of the nine dtypes of sort; bool raises torch's own
    RuntimeError.  -0.0 equals +0.0, and a NaN equals nothing, a NaN among the test elements included.  assume_unique is accepted and
    changes nothing: duplicates among the test elements never change membership.  An empty `elements` or an empty test set launches
    nothing.  Refusals (CPU tensors, two devices, 2^32 or more elements on either side, other dtypes) are VrsError and come before any
    device work."""
    import torch

    tensors = [t for t in (elements, test_elements) if isinstance(t, torch.Tensor)]
    if not tensors:
        _refuse("isin takes a tensor as elements or as test_elements")
    for t in (elements, test_elements):
        if not isinstance(t, (torch.Tensor, bool, int, float)):
            _refuse("elements and test_elements must be tensors or Python numbers")
    if any(t.dtype == torch.bool if isinstance(t, torch.Tensor) else isinstance(t, bool) for t in (elements, test_elements)):
        raise RuntimeError("Unsupported input type encountered for isin(): Bool")  # (torch's refusal of a bool on either side, in its words)
    common = torch.result_type(elements, test_elements)
    code = _dtype_code(torch, common, "isin")  # (refuses a promoted dtype outside the nine)
    if not all(t.is_cuda for t in tensors):
        _refuse("isin takes tensors on a GPU")
    device = tensors[0].device
    if tensors[-1].device != device:
        _refuse("elements and test_elements must be on one device")
    if any(t.numel() >= 1 << 32 for t in tensors):
        _refuse("isin takes fewer than 2^32 elements on either side")
    as_tensor = lambda t: t if isinstance(t, torch.Tensor) else torch.tensor(t, dtype=common, device=device)  # noqa: E731
    queries = aligned(as_tensor(elements).to(common).contiguous())
    tests = as_tensor(test_elements).to(common).reshape(-1)
    nq, m = queries.numel(), tests.numel()
    if nq == 0:
        return torch.empty(queries.shape, dtype=torch.bool, device=device)
    if m == 0:
        return torch.full(queries.shape, bool(invert), dtype=torch.bool, device=device)
    bounds = aligned(sort_values(tests))
    out = torch.empty(queries.shape, dtype=torch.bool, device=device)
    flags = capi.VRS_SEARCH_MEMBER | (capi.VRS_SEARCH_MEMBER_INVERT if invert else 0)
    ctx = context_for(device)
    lib = ctx.lib
    tier, need = ctypes.c_int(), ctypes.c_uint64()
    ctx.check(lib.vrs_search_plan(ctx.handle, m, m, nq, nq, code, 0, ctypes.byref(tier), ctypes.byref(need)))
    scratch = torch.empty(need.value, dtype=torch.uint8, device=device) if need.value else None
    with buffers(ctx, bounds, queries, out, scratch) as (bnd, qry, res, scr):
        ctx.check(lib.vrs_search_sorted(ctx.handle, bnd, m, m, qry, nq, nq, code, flags, None, res, scr))
    return out


def bucketize(input, boundaries, *, out_int32: bool = False, right: bool = False):
    """torch.bucketize(input, boundaries, out_int32=, right=): searchsorted(boundaries, input, ...) for 1-D boundaries."""
    import torch

    if not isinstance(boundaries, torch.Tensor) or boundaries.dim() != 1:
        _refuse("bucketize takes 1-D boundaries")
    return searchsorted(boundaries, input, out_int32=out_int32, right=right)
