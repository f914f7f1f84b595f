"""torch.bincount, torch.histc and torch.histogram drop-ins: how many elements (or how much weight) fall into each bin (vrs_bin_count).

One counting call on torch's current stream.  The library picks a tier from the number of bins (vrs_bin_count_plan): counters that fit
a workgroup's LDS are kept there and flushed once, larger tables take every add as a global atomic.  Counts are accumulated as
integers and converted once, so a float count is the correctly rounded count (torch's float atomics stop growing at 2^24 in float32);
weighted sums are float atomics in no specified order, as torch's are.
"""
from __future__ import annotations

import ctypes
import math

from . import capi
from ._torch import aligned, buffers, context_for
from .capi import VrsError
from .search import bucketize
from .sort import _dtype_code

TIER_NAMES = {capi.VRS_BINCOUNT_LDS: "lds", capi.VRS_BINCOUNT_GLOBAL: "global"}
_INDEX_DTYPES = ("uint8", "int8", "int16", "int32", "int64")
_LINEAR_DTYPES = ("float16", "bfloat16", "float32", "float64")


def _refuse(message: str):
    raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, message)


def bincount_stats(ctx) -> dict:
    """Calls the context's counts ran in each tier so far (cumulative; counted on the host)."""
    c = [ctypes.c_uint64() for _ in range(2)]
    ctx.check(ctx.lib.vrs_bin_count_stats(ctx.handle, *(ctypes.byref(v) for v in c)))
    return {name: c[tier].value for tier, name in TIER_NAMES.items()}


def _count(values, mode: int, lo: float, hi: float, num_bins: int, weights, out_dtype):
    """vrs_bin_count of the contiguous 1-D `values` (and `weights`) into a new tensor of num_bins entries of out_dtype."""
    import torch

    if values.numel() >= 1 << 32:
        _refuse("a count takes fewer than 2^32 elements")
    if not 1 <= num_bins < 1 << 32:
        _refuse(f"a count takes 1 to 2^32 - 1 bins, not {num_bins}")
    device = values.device
    values, weights = aligned(values), aligned(weights) if weights is not None else None
    w_code = _dtype_code(torch, weights.dtype) if weights is not None else capi.VRS_BIN_NO_WEIGHTS
    out = torch.empty(num_bins, dtype=out_dtype, device=device)
    ctx = context_for(device)
    lib = ctx.lib
    tier, need = ctypes.c_int(), ctypes.c_uint64()
    ctx.check(lib.vrs_bin_count_plan(ctx.handle, num_bins, w_code, _dtype_code(torch, out_dtype), ctypes.byref(tier), ctypes.byref(need)))
    scratch = torch.empty(need.value, dtype=torch.uint8, device=device)
    with buffers(ctx, values, weights, out, scratch) as (val, wgt, res, scr):
        ctx.check(lib.vrs_bin_count(ctx.handle, val, values.numel(), _dtype_code(torch, values.dtype), mode, lo, hi, num_bins, wgt, w_code,
                                    _dtype_code(torch, out_dtype), res, None, scr))
    return out


def _on_gpu(name: str, *tensors):
    device = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            _refuse(f"{name} takes tensors on a GPU")
        if device is not None and t.device != device:
            _refuse(f"{name} takes tensors on one device")
        device = t.device


def bincount(input, weights=None, minlength: int = 0):
    """torch.bincount(input, weights=None, minlength=0) of a 1-D uint8 / int8 / int16 / int32 / int64 tensor on a GPU: out[v] = the
    number of elements equal to v (the sum of their weights), for v up to max(input.max(), minlength - 1).

    int64 without weights; with float32 or float64 weights their dtype, with weights of any other dtype float64 (they are
    .double()ed, as torch does).  The size comes from one torch.aminmax and one host read (torch waits for the device there too); a
    negative element raises with torch's message.  An empty input gives minlength zeros (of the weights' dtype when there are
    weights; torch gives int64 there).  The elements are read in their own width.
    Non-contiguous tensors and 1- or 2-byte views that start off a 4-byte boundary are made contiguous and aligned first (one
    copy).  Refusals are VrsError and come before any device work."""
    import torch

    if not isinstance(input, torch.Tensor) or (weights is not None and not isinstance(weights, torch.Tensor)):
        _refuse("bincount takes tensors")
    if input.dim() != 1:
        _refuse("bincount only supports 1-d non-negative integral inputs.")
    if str(input.dtype).replace("torch.", "") not in _INDEX_DTYPES:
        _refuse(f"bincount takes uint8, int8, int16, int32 or int64, not {input.dtype}")
    if not isinstance(minlength, int) or isinstance(minlength, bool) or minlength < 0:
        _refuse("minlength should be >= 0")
    if weights is not None and weights.shape != input.shape:
        _refuse("weights should be 1-d and have the same length as input")
    _on_gpu("bincount", input, weights)
    if weights is not None and weights.dtype not in (torch.float32, torch.float64):
        weights = weights.double()
    out_dtype = torch.int64 if weights is None else weights.dtype
    if input.numel() == 0:
        return torch.zeros(minlength, dtype=out_dtype, device=input.device)
    smallest, largest = torch.stack(torch.aminmax(input)).tolist()
    if smallest < 0:
        _refuse("bincount only supports 1-d non-negative integral inputs.")
    return _count(input.contiguous(), capi.VRS_BIN_INDEX, 0.0, 0.0, max(largest + 1, minlength),
                  weights.contiguous() if weights is not None else None, out_dtype)


def histc(input, bins: int = 100, min=0, max=0):
    """torch.histc(input, bins=100, min=0, max=0) of a float16 / bfloat16 / float32 / float64 tensor of any shape on a GPU: `bins`
    counts in the input's dtype over [min, max], by torch's rule evaluated in float32 (float64 for float64):
        bin = (int)((x - min) * bins / (max - min)),   bin == bins goes to the last bin;   x < min, x > max and NaN are not counted.
    min == max: the range is the data's minimum and maximum (one torch.aminmax and one host read), widened by 1 each way if those are
    equal too; a range that is not finite raises, as torch.  With an explicit range the call does not wait for the device.
    Unlike torch's float32 result, which is a sum of float ones and stops growing at 2^24, each count here is accumulated as an integer
    and rounded to the dtype once.  Refusals are VrsError and come before any device work."""
    import torch

    if not isinstance(input, torch.Tensor):
        _refuse("histc takes a tensor")
    if str(input.dtype).replace("torch.", "") not in _LINEAR_DTYPES:
        _refuse(f"histc takes float16, bfloat16, float32 or float64, not {input.dtype}")
    if not isinstance(bins, int) or isinstance(bins, bool) or bins <= 0:
        _refuse("bins must be > 0")
    lo, hi = float(min), float(max)
    if lo > hi:
        _refuse("max must be larger than min")
    if lo != hi and not (math.isfinite(lo) and math.isfinite(hi)):
        _refuse(f"range of [{lo}, {hi}] is not finite")
    _on_gpu("histc", input)
    if input.numel() == 0 and lo == hi:
        return torch.zeros(bins, dtype=input.dtype, device=input.device)
    if lo == hi:
        lo, hi = torch.stack(torch.aminmax(input)).tolist()
    if not (math.isfinite(lo) and math.isfinite(hi)):
        _refuse(f"range of [{lo}, {hi}] is not finite")
    if lo == hi:
        lo, hi = lo - 1.0, hi + 1.0
    return _count(input.contiguous().view(-1), capi.VRS_BIN_LINEAR, lo, hi, bins, None, input.dtype)


def histogram(input, bins, *, range=None, weight=None, density: bool = False):
    """torch.histogram(input, bins, *, range=None, weight=None, density=False) of a float32 / float64 tensor on a GPU, where torch has
    no implementation: (hist, bin_edges), both of the input's dtype.

    An int `bins`: bin_edges = torch.linspace(lo, hi, bins + 1) with (lo, hi) = `range`, or the data's minimum and maximum (one
    torch.aminmax and one host read; widened by 0.5 each way when they are equal, (0, 1) for an empty input; as torch).  A 1-D tensor
    `bins`: that tensor is bin_edges (ascending; not checked).  An element x falls into bin i when edges[i] <= x < edges[i + 1], the last
    bin also takes x == edges[-1]; elements outside the edges and NaN are not counted.  `weight`: a tensor of the input's shape and dtype.
    This is the first form, a composition: bucketize over the edges, two elementwise passes (- 1, and the last edge by torch.where),
    then one counting call in index mode, whose skip rule drops everything outside.  density=True divides by hist.sum() * diff(edges)
    with torch ops.  Refusals are VrsError and come before any device work."""
    import torch

    if not isinstance(input, torch.Tensor) or (weight is not None and not isinstance(weight, torch.Tensor)):
        _refuse("histogram takes tensors")
    if input.dtype not in (torch.float32, torch.float64):
        _refuse(f"histogram takes float32 or float64, not {input.dtype}")
    if weight is not None and (weight.shape != input.shape or weight.dtype != input.dtype):
        _refuse("weight must have the input's shape and dtype")
    edges_given = isinstance(bins, torch.Tensor)
    if edges_given:
        if bins.dim() != 1 or bins.numel() < 2 or bins.dtype != input.dtype:
            _refuse("bins must be an int or a 1-D tensor of two or more edges of the input's dtype")
    elif not isinstance(bins, int) or isinstance(bins, bool) or bins <= 0:
        _refuse("bins must be > 0")
    if range is not None:
        if edges_given:
            _refuse("range goes with an int bins only")
        lo, hi = (float(v) for v in range)
        if not (math.isfinite(lo) and math.isfinite(hi)):
            _refuse(f"range of [{lo}, {hi}] is not finite")
        if lo > hi:
            _refuse("max must be larger than min")
    _on_gpu("histogram", input, weight, bins if edges_given else None)
    x = input.contiguous().view(-1)
    if edges_given:
        edges = bins.contiguous()
    else:
        if range is None:
            lo, hi = torch.stack(torch.aminmax(x)).tolist() if x.numel() else (0.0, 1.0)
            if not (math.isfinite(lo) and math.isfinite(hi)):
                _refuse(f"range of [{lo}, {hi}] is not finite")
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5
        edges = torch.linspace(lo, hi, bins + 1, dtype=input.dtype, device=input.device)
    num_bins = edges.numel() - 1
    if x.numel() == 0:
        hist = torch.zeros(num_bins, dtype=input.dtype, device=input.device)
    else:
        at = bucketize(x, edges, right=True, out_int32=True) - 1
        at = torch.where(x == edges[-1], num_bins - 1, at)
        hist = _count(at, capi.VRS_BIN_INDEX, 0.0, 0.0, num_bins, weight.contiguous().view(-1) if weight is not None else None, input.dtype)
    if density:
        hist = hist / (hist.sum() * torch.diff(edges))
    return hist, edges
