"""torch.cumsum, cumprod, cummax and cummin drop-ins with a fixed order (vrs_scan_rows).

A contiguous tensor is viewed as [S, L, C] around `dim` and scanned where it lies, every column on its own: no transposed copy for a dim
other than the last.  Sums and products are combined in one fixed order (include/vkradixsort_amd_ops.h "K14"), a function of the length
along dim, the width behind it, the dtype and VRS_TUNE_SCAN_TILE_ROWS alone: the same input gives the same bits on every run, which
torch.cumsum on a GPU does not promise.  float16 and bfloat16 are accumulated in float32 and rounded once per output; a float sum starts
at +0.0, so cumsum of [-0.0] is +0.0 (torch's CPU answer too).  cummax and cummin equal torch's CPU results bit for bit, indices included.

Not offered: exclusive and reverse scans, out=, logcumsumexp (its exp / log cannot be held bit-equal between host and device), complex
dtypes and ragged segments.  A tensor that is not contiguous is made contiguous first.
"""
from __future__ import annotations

import ctypes
import math

from . import capi
from ._torch import aligned, buffers, context_for
from .binning import _on_gpu
from .capi import VrsError
from .sort import _dtype_code

TIER_NAMES = {capi.VRS_SCAN_TILE: "tile", capi.VRS_SCAN_THREE_LAUNCH: "three_launch", capi.VRS_SCAN_SINGLE_PASS: "single_pass"}
_KERNEL_OUT = ("int32", "int64", "float16", "bfloat16", "float32", "float64")  # what SUM and PROD write
_WIDENED = ("int8", "uint8", "int16", "int32")                                   # what they read into int64


def _refuse(message: str):
    raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, message)


def _name(dtype) -> str:
    return str(dtype).replace("torch.", "")


def scan_stats(ctx) -> dict:
    """Calls the context's scans gave each tier so far, and the status words a waiting wave of the single pass computed itself
    (cumulative; waits for the stream)."""
    c = [ctypes.c_uint64() for _ in range(4)]
    ctx.check(ctx.lib.vrs_scan_stats(ctx.handle, *(ctypes.byref(v) for v in c)))
    stats = {name: c[t].value for t, name in TIER_NAMES.items()}
    stats["takeovers"] = c[3].value
    return stats


def _check(name: str, x, dim: int, coded: bool = False) -> int:
    """What is refused before any device work: the dtype first (coded: one the kernel has a code for, bool as uint8), then the device, the dim."""
    import torch

    if not isinstance(x, torch.Tensor):
        _refuse(f"{name} takes a tensor")
    if x.dtype.is_complex:
        _refuse(f"{name} takes no complex dtype")
    if coded:
        _dtype_code(torch, torch.uint8 if x.dtype == torch.bool else x.dtype, name)
    _on_gpu(name, x)
    nd = max(x.dim(), 1)
    if not isinstance(dim, int) or not -nd <= dim < nd:
        raise IndexError(f"Dimension out of range (expected to be in range of [{-nd}, {nd - 1}], but got {dim})")
    return dim % nd


def _scan_rows(src, dim: int, op: int, out_dtype):
    """vrs_scan_rows of `src` along dim: (out of out_dtype, int64 indices or None), both of src's shape."""
    import torch

    pairs = op in (capi.VRS_SCAN_MAX, capi.VRS_SCAN_MIN)
    device = src.device
    out = torch.empty(src.shape, dtype=out_dtype, device=device)
    idx = torch.empty(src.shape, dtype=torch.int64, device=device) if pairs else None
    if src.numel() == 0:
        return out, idx
    shape = tuple(src.shape) or (1,)
    S, L, C = math.prod(shape[:dim]), shape[dim], math.prod(shape[dim + 1:])
    if S * L >= 1 << 32 or C >= 1 << 32:
        _refuse("a scan takes fewer than 2^32 rows in all and fewer than 2^32 columns")
    src = aligned(src.contiguous())
    code, out_code = _dtype_code(torch, src.dtype, "scan"), _dtype_code(torch, out_dtype, "scan")
    ctx = context_for(device)
    tile_rows, min_rows = ctx.tuned(capi.VRS_TUNE_SCAN_TILE_ROWS), ctx.tuned(capi.VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS)
    need = capi.query_u64("vrs_scan_scratch_bytes", S, L, C, code, out_code, op, tile_rows, min_rows)
    scratch = torch.empty(need, dtype=torch.uint8, device=device)
    with buffers(ctx, src, out, idx, scratch) as (val, res, ind, scr):
        ctx.check(ctx.lib.vrs_scan_rows(ctx.handle, val, S, L, C, code, out_code, op, res, ind, scr))
    return out, idx


def _arith(name: str, x, dim: int, op: int, dtype):
    import torch

    dim = _check(name, x, dim)
    target = dtype if dtype is not None else (x.dtype if x.dtype.is_floating_point else torch.int64)
    if not isinstance(target, torch.dtype) or target.is_complex:
        _refuse(f"{name} takes a real torch.dtype")
    if _name(target) in _KERNEL_OUT:
        direct = x.dtype == target or (target == torch.int64 and _name(x.dtype) in _WIDENED)
        return _scan_rows(x if direct else x.to(target), dim, op, target)[0]
    # a dtype= the kernel does not write: convert first, scan in int64 (narrow integers wrap alike) or float32, convert back
    src = x.to(target)
    if target.is_floating_point:
        return _scan_rows(src.to(torch.float32), dim, op, torch.float32)[0].to(target)
    if _name(target) not in _WIDENED:
        src = src.to(torch.int64)
    return _scan_rows(src, dim, op, torch.int64)[0].to(target)


def cumsum(x, dim: int, *, dtype=None):
    """torch.cumsum(x, dim, dtype=None) on a GPU, in a fixed order: any shape, any dim.  An integer or bool input without dtype= gives
    int64, as torch (int8, uint8, int16 and int32 are widened by the kernel's load, anything else by one .to()); integer sums wrap."""
    return _arith("cumsum", x, dim, capi.VRS_SCAN_SUM, dtype)


def cumprod(x, dim: int, *, dtype=None):
    """torch.cumprod(x, dim, dtype=None) on a GPU, in a fixed order; dtypes as cumsum."""
    return _arith("cumprod", x, dim, capi.VRS_SCAN_PROD, dtype)


def _pairs(name: str, x, dim: int, op: int):
    import torch

    dim = _check(name, x, dim, coded=True)
    src = x.to(torch.uint8) if x.dtype == torch.bool else x
    values, indices = _scan_rows(src, dim, op, src.dtype)
    return getattr(torch.return_types, name)((values.to(x.dtype), indices))


def cummax(x, dim: int):
    """torch.cummax(x, dim) on a GPU: (values, int64 indices), equal to torch's CPU result bit for bit -- ties take the later index, a
    NaN stays and the index follows the latest NaN."""
    return _pairs("cummax", x, dim, capi.VRS_SCAN_MAX)


def cummin(x, dim: int):
    """torch.cummin(x, dim) on a GPU: (values, int64 indices), as cummax."""
    return _pairs("cummin", x, dim, capi.VRS_SCAN_MIN)
