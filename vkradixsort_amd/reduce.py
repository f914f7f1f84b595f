"""torch.segment_reduce, index_add, index_reduce and scatter_reduce drop-ins with reproducible results (vrs_segment_reduce).

Rows that share a destination are reduced in one fixed order (include/vkradixsort_amd_ops.h "K13"): the same input gives the same bits on
every run, where torch's float atomics differ in the last bits from run to run.  The index forms sort (index, position) pairs by
destination with the stable one-call sort, find every destination's range in the sorted indices with one search, and reduce the
gathered rows range by range; nothing is added with a float atomic.  float16 and bfloat16 values are accumulated in float32 and rounded
once; a float sum that is zero is +0.0.
"""
from __future__ import annotations

import ctypes
import math

from . import capi
from ._torch import aligned, buffers, context_for
from .binning import _on_gpu
from .capi import VrsError
from .sort import _dtype_code

MAP_NAMES = {capi.VRS_REDUCE_MAP_LANE: "lane", capi.VRS_REDUCE_MAP_ROWS: "rows", capi.VRS_REDUCE_MAP_COLUMNS: "columns"}
_OPS = {"sum": capi.VRS_REDUCE_SUM, "mean": capi.VRS_REDUCE_SUM, "prod": capi.VRS_REDUCE_PROD, "min": capi.VRS_REDUCE_MIN, "max": capi.VRS_REDUCE_MAX,
        "amin": capi.VRS_REDUCE_MIN, "amax": capi.VRS_REDUCE_MAX}
_DTYPES = ("int32", "int64", "float16", "bfloat16", "float32", "float64")


def _refuse(message: str):
    raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, message)


def reduce_stats(ctx) -> dict:
    """Chunks the context's reductions gave each lane map so far and the most levels a segment took (cumulative; waits for the stream)."""
    c = [ctypes.c_uint64() for _ in range(4)]
    ctx.check(ctx.lib.vrs_segment_reduce_stats(ctx.handle, *(ctypes.byref(v) for v in c)))
    stats = {name: c[m].value for m, name in MAP_NAMES.items()}
    stats["max_levels"] = c[3].value
    return stats


def _check_dtype(name: str, dtype):
    if str(dtype).replace("torch.", "") not in _DTYPES:
        _refuse(f"{name} takes int32, int64, float16, bfloat16, float32 or float64, not {dtype}")


def _as_u32(bounds):
    """int64 bounds below 2^32 as uint32 bit patterns in an int32 tensor"""
    import torch

    return ((bounds + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)


def _reduce_rows(values, order, offsets, num_segments: int, op: int, init):
    """vrs_segment_reduce of the contiguous [n, C] `values` (rows taken through the int32 `order` when given) over the num_segments + 1
    int32 `offsets`, on top of the [num_segments, C] `init` when given: a new [num_segments, C] tensor."""
    import torch

    n, C = values.shape
    if n >= 1 << 32 or num_segments >= 1 << 32 or C >= 1 << 32:
        _refuse("a reduction takes fewer than 2^32 rows, columns and segments")
    device = values.device
    values, init = aligned(values), aligned(init) if init is not None else None
    out = torch.empty((num_segments, C), dtype=values.dtype, device=device)
    if num_segments == 0 or C == 0:
        return out
    code = _dtype_code(torch, values.dtype)
    ctx = context_for(device)
    lib = ctx.lib
    chunk_rows = ctx.tuned(capi.VRS_TUNE_REDUCE_CHUNK_ROWS)
    need = capi.query_u64("vrs_segment_reduce_scratch_bytes", n, C, num_segments, code, chunk_rows)
    scratch = torch.empty(need, dtype=torch.uint8, device=device)
    with buffers(ctx, values, order, offsets, init, out, scratch) as (val, ordr, offs, ini, res, scr):
        ctx.check(lib.vrs_segment_reduce(ctx.handle, val, n, C, code, ordr, offs, num_segments, op, ini, res, scr))
    return out


def segment_reduce(data, reduce: str, *, lengths=None, offsets=None, axis: int = 0, unsafe: bool = False, initial=None):
    """torch.segment_reduce(data, reduce, lengths= | offsets=, axis=0, unsafe=False, initial=None) of an N-D tensor on a GPU along axis 0,
    for 1-D lengths or offsets: `sum`, `mean`, `max`, `min` or `prod` of every segment of rows, in a fixed order.

    As torch's CPU version: a segment without rows answers `initial`, or without it 0 (sum), 1 (prod), -inf (max), +inf (min), NaN
    (mean); `mean` is (initial + sum) / length; max and min propagate NaN; unless `unsafe`, negative lengths and lengths that do not
    sum to data.shape[0] raise (one host read).  Unlike torch it also takes int32 and int64 data: their sums and products wrap, their
    empty max / min segments answer the type's minimum / maximum, their mean is floored and 0 for an empty segment.
    Non-contiguous data is made contiguous first.  Refusals are VrsError and come before any device work."""
    import torch

    if not isinstance(data, torch.Tensor):
        _refuse("segment_reduce takes a tensor")
    if reduce not in ("sum", "mean", "max", "min", "prod"):
        _refuse(f"segment_reduce takes sum, mean, max, min or prod, not {reduce!r}")
    if (lengths is None) == (offsets is None):
        _refuse("segment_reduce takes either lengths or offsets")
    bounds = lengths if lengths is not None else offsets
    if not isinstance(bounds, torch.Tensor) or bounds.dim() != 1 or bounds.dtype not in (torch.int32, torch.int64):
        _refuse("lengths / offsets must be a 1-D int32 or int64 tensor")
    if offsets is not None and offsets.numel() == 0:
        _refuse("offsets holds one bound or more")
    if data.dim() == 0:
        _refuse("segment_reduce takes data of one dimension or more")
    if axis not in (0, -data.dim()):
        _refuse("segment_reduce reduces along axis 0 only")
    _check_dtype("segment_reduce", data.dtype)
    _on_gpu("segment_reduce", data, bounds)
    n = data.shape[0]
    lens = bounds.long() if lengths is not None else torch.diff(bounds.long())
    if not unsafe and lens.numel():
        smallest, total = torch.stack((lens.min(), lens.sum())).tolist()
        if smallest < 0:
            raise RuntimeError("lengths contains negative value!")
        if total != n:
            raise RuntimeError("Expected all rows of lengths along axis to sum to data.size(lengths.dim()-1) when !unsafe.")
    if lengths is not None:
        ends = torch.cumsum(lens, 0)
        offs = torch.cat((torch.zeros(1, dtype=torch.int64, device=data.device), ends))
    else:
        offs = bounds.long()
    num_segments = offs.numel() - 1
    rest = tuple(data.shape[1:])
    values = data.contiguous().view(n, math.prod(rest))
    init = None
    if initial is not None:
        init = torch.full((num_segments, values.shape[1]), initial, dtype=data.dtype, device=data.device)
    out = _reduce_rows(values, None, _as_u32(offs.clamp(0, (1 << 32) - 1)), num_segments, _OPS[reduce], init)
    if reduce == "mean":
        count = lens.clamp(min=0).view(-1, 1)
        if data.dtype.is_floating_point:
            empty = torch.full_like(out, math.nan) if initial is None else out
            out = torch.where(count > 0, out / count.clamp(min=1).to(out.dtype), empty)
        else:
            out = torch.div(out, count.clamp(min=1).to(out.dtype), rounding_mode="floor")
    return out.view((num_segments,) + rest)


def _by_destination(name: str, input, dim: int, index, source, reduce: str, include_self: bool, alpha=1):
    """out = input with every row source[i] reduced into row index[i] along dim: sort by destination, find the ranges, reduce them."""
    import torch

    from .search import searchsorted

    if not all(isinstance(t, torch.Tensor) for t in (input, index, source)):
        _refuse(f"{name} takes tensors")
    if input.dim() == 0 or source.dim() != input.dim():
        _refuse(f"{name} takes an input of one dimension or more and a source of as many")
    nd = input.dim()
    if not -nd <= dim < nd:
        raise IndexError(f"Dimension out of range (expected to be in range of [{-nd}, {nd - 1}], but got {dim})")
    dim %= nd
    if index.dim() != 1 or index.dtype not in (torch.int32, torch.int64):
        _refuse(f"{name} takes a 1-D int32 or int64 index")
    if source.dtype != input.dtype:
        _refuse(f"{name}: source must have the input's dtype")
    _check_dtype(name, input.dtype)
    if index.numel() != source.shape[dim] or any(source.shape[d] != input.shape[d] for d in range(nd) if d != dim):
        _refuse(f"{name}: source must have index.numel() entries along dim and the input's shape elsewhere")
    _on_gpu(name, input, index, source)
    M, n = input.shape[dim], index.numel()
    if M >= 1 << 31 or n >= 1 << 32:
        _refuse(f"{name} takes fewer than 2^31 destinations and 2^32 contributions")
    if n == 0 or input.numel() == 0:
        return input.clone()
    smallest, largest = torch.stack(torch.aminmax(index)).tolist()
    if smallest < 0 or largest >= M:
        raise IndexError("index out of range in self")
    device = input.device
    base = input.movedim(dim, 0).contiguous()
    rows = source.movedim(dim, 0).contiguous().view(n, input.numel() // M)
    if alpha != 1:
        rows = rows * alpha
    # (index, position) sorted by index, stable: the positions of one destination stay ascending
    keys, keys_tmp = index.to(torch.int32, copy=True).contiguous(), torch.empty(n, dtype=torch.int32, device=device)
    pos, pos_tmp = torch.arange(n, dtype=torch.int32, device=device), torch.empty(n, dtype=torch.int32, device=device)
    ctx = context_for(device)
    with buffers(ctx, keys, keys_tmp, pos, pos_tmp) as (k, kt, p, pt):
        ctx.check(ctx.lib.vrs_sort_pairs_u32(ctx.handle, k, kt, p, pt, n))
    offsets = searchsorted(keys, torch.arange(M + 1, dtype=torch.int32, device=device), out_int32=True)
    init = base.view(M, input.numel() // M) if include_self else None
    out = _reduce_rows(rows, pos, offsets, M, _OPS[reduce], init)
    count = (offsets[1:] - offsets[:-1]).view(M, 1)
    if reduce == "mean":
        total = count + (1 if include_self else 0)
        if input.dtype.is_floating_point:
            out = out / total.clamp(min=1).to(out.dtype)
        else:
            out = torch.div(out, total.clamp(min=1).to(out.dtype), rounding_mode="floor")
    if not include_self:
        out = torch.where(count > 0, out, base.view(M, input.numel() // M))
    return out.view(base.shape).movedim(0, dim)


def index_add(input, dim: int, index, source, *, alpha=1):
    """torch.index_add(input, dim, index, source, alpha=1) on a GPU, out of place, for int32, int64, float16, bfloat16, float32 and
    float64: out = input, plus alpha * source[i] added to row index[i] along dim -- the rows of one destination in the order of i, by
    the fixed order of vrs_segment_reduce, so two runs give the same bits.  alpha != 1 multiplies the source first (one pass).
    An index outside [0, input.shape[dim]) raises IndexError (one torch.aminmax and one host read)."""
    return _by_destination("index_add", input, dim, index, source, "sum", True, alpha)


def index_reduce(input, dim: int, index, source, reduce: str, *, include_self: bool = True):
    """torch.index_reduce(input, dim, index, source, reduce, include_self=True) on a GPU, out of place: `prod`, `mean`, `amax` or
    `amin`.  mean is the sum divided by the number of contributions (plus one with include_self), floored for integers as torch floors;
    without include_self a destination no index names keeps its input."""
    if reduce not in ("prod", "mean", "amax", "amin"):
        _refuse(f"index_reduce takes prod, mean, amax or amin, not {reduce!r}")
    return _by_destination("index_reduce", input, dim, index, source, reduce, bool(include_self))


def scatter_reduce(input, dim: int, index, src, reduce: str, *, include_self: bool = True):
    """torch.scatter_reduce(input, dim, index, src, reduce, include_self=True) for 1-D tensors on a GPU, out of place: `sum`, `prod`,
    `mean`, `amax` or `amin`; the first index.numel() entries of src are used, as torch.  N-D tensors raise NotImplementedError in this
    first form."""
    import torch

    if reduce not in ("sum", "prod", "mean", "amax", "amin"):
        _refuse(f"scatter_reduce takes sum, prod, mean, amax or amin, not {reduce!r}")
    if not all(isinstance(t, torch.Tensor) for t in (input, index, src)):
        _refuse("scatter_reduce takes tensors")
    if input.dim() != 1 or index.dim() != 1 or src.dim() != 1:
        raise NotImplementedError("scatter_reduce takes 1-D tensors in this first form")
    if dim not in (0, -1):
        raise IndexError(f"Dimension out of range (expected to be in range of [-1, 0], but got {dim})")
    if index.numel() > src.numel():
        _refuse("scatter_reduce: index may not be longer than src")
    return _by_destination("scatter_reduce", input, 0, index, src[:index.numel()], reduce, bool(include_self))
