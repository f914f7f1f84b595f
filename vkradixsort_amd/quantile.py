"""torch.quantile and torch.nanquantile drop-ins: the neighbouring order statistics of every q by a multi-rank radix select
(vrs_quantile_segments), without sorting the row, and torch's interpolation between them.

quantile_segments works on Buffers of a GPUContext; quantile and nanquantile take float32 / float64 torch tensors of any shape, dim and
strides, on torch's current stream.  A q that asks for more than 16 order statistics per row (9 or more q with "linear" or "midpoint",
17 or more with the others) sorts the rows with this library's sort instead and gathers.  The values of the order statistics are rebuilt
from their ranks: +0.0 for either zero.
"""
from __future__ import annotations

import ctypes

from . import capi
from ._torch import aligned, buffers, context_for, row_offsets
from .capi import VrsError

INTERPOLATIONS = {"linear": capi.VRS_QUANTILE_LINEAR, "lower": capi.VRS_QUANTILE_LOWER, "higher": capi.VRS_QUANTILE_HIGHER,
                  "midpoint": capi.VRS_QUANTILE_MIDPOINT, "nearest": capi.VRS_QUANTILE_NEAREST}


def _sides(interpolation: str) -> int:
    return 2 if interpolation in ("linear", "midpoint") else 1


def quantile_scratch_bytes(num_elements: int, num_segments: int, dtype: int) -> int:
    """Bytes of scratch vrs_quantile_segments needs for this shape and dtype (capi.VRS_SORT_FLOAT32 / FLOAT64); no device."""
    return capi.query_u64("vrs_quantile_scratch_bytes", num_elements, num_segments, dtype)


def quantile_segments(ctx, src, offsets, num_elements: int, num_segments: int, dtype: int, q, out_values, out_lower=None, out_upper=None,
                      out_weight=None, scratch=None, interpolation: str = "linear", ignore_nan: bool = False) -> None:
    """For every segment i = src[offsets[i], offsets[i+1]) of float32 / float64 elements (`dtype`: a capi.VRS_SORT_* code) and every q[j]
    (a sequence of Python floats in [0, 1]): the quantile into out_values[i, j] and, where given, the two order statistics it lies between
    and the weight into out_lower, out_upper and out_weight -- each [num_segments, len(q)] elements of the dtype; NaN everywhere for a
    segment without an answer (empty; any NaN, or with ignore_nan NaNs alone).  scratch: a Buffer of at least quantile_scratch_bytes(...)
    bytes.  Stream-ordered on the context's stream."""
    if interpolation not in INTERPOLATIONS:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"interpolation must be one of {sorted(INTERPOLATIONS)}")
    if scratch is None:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "quantile_segments needs a scratch Buffer of quantile_scratch_bytes(...) bytes")
    qs = (ctypes.c_double * max(len(q), 1))(*[float(v) for v in q])
    handle = lambda b: b.handle if b is not None else None  # noqa: E731
    ctx.check(ctx.lib.vrs_quantile_segments(ctx.handle, src.handle, num_elements, offsets.handle, num_segments, dtype, qs, len(q),
                                            INTERPOLATIONS[interpolation], capi.VRS_QUANTILE_IGNORE_NAN if ignore_nan else 0,
                                            out_values.handle, handle(out_lower), handle(out_upper), handle(out_weight), scratch.handle))


def quantile_stats(ctx) -> dict:
    """Segments the context's quantile calls gave each tier so far, and the grid-tier segments that sieved (cumulative)."""
    c = [ctypes.c_uint64() for _ in range(4)]
    ctx.check(ctx.lib.vrs_quantile_stats(ctx.handle, *(ctypes.byref(v) for v in c)))
    return {"lds": c[0].value, "block": c[1].value, "grid": c[2].value, "sieved": c[3].value}


def _select_rows(xt, code: int, qs, interpolation: str, ignore_nan: bool):
    """[rows, Q] quantiles of the rows of a contiguous 2-d tensor by vrs_quantile_segments."""
    import torch

    rows, length = xt.shape
    n = xt.numel()
    device = xt.device
    out = torch.empty((rows, len(qs)), dtype=xt.dtype, device=device)
    ctx = context_for(device)
    scratch = torch.empty(max(quantile_scratch_bytes(n, rows, code), 8), dtype=torch.uint8, device=device)
    arr = (ctypes.c_double * len(qs))(*qs)
    with buffers(ctx, xt, row_offsets(rows, length, device), out, scratch) as (src, offsets, out_v, scr):
        ctx.check(ctx.lib.vrs_quantile_segments(ctx.handle, src, n, offsets, rows, code, arr, len(qs), INTERPOLATIONS[interpolation],
                                                capi.VRS_QUANTILE_IGNORE_NAN if ignore_nan else 0, out_v, None, None, None, scr))
    return out


def _sort_rows(xt, qs, interpolation: str, ignore_nan: bool):
    """[rows, Q] quantiles of the rows of a contiguous 2-d tensor by this library's sort, a gather and the rule and interpolation of
    vrs_quantile_segments in torch operations (each rounded on its own): the same bits as _select_rows."""
    import torch

    from .sort import sort_values

    rows, length = xt.shape
    dt = xt.dtype
    srt = sort_values(xt, -1)  # (NaNs last)
    nans = torch.isnan(srt).sum(-1)
    live = length - nans if ignore_nan else torch.full_like(nans, length)
    valid = (live > 0) if ignore_nan else (nans == 0)
    last = (live - 1).clamp(min=0)
    r = torch.tensor(qs, dtype=dt, device=xt.device)[None, :] * last.to(dt)[:, None]
    if interpolation == "lower":
        r = r.floor()
    elif interpolation == "higher":
        r = r.ceil()
    elif interpolation == "nearest":
        r = r.round()  # (half to even)
    below = r.floor()
    cap = last.to(dt)[:, None]
    lo = torch.minimum(below, cap).long().minimum(last[:, None])
    a = srt.gather(-1, lo) + 0.0  # (+ 0.0: -0.0 becomes +0.0, as the selection answers)
    if _sides(interpolation) == 2:
        hi = torch.minimum(r.ceil(), cap).long().minimum(last[:, None])
        b = srt.gather(-1, hi) + 0.0
        w = torch.full_like(r, 0.5) if interpolation == "midpoint" else r - below
        d = b - a
        v = torch.where(w < 0.5, a + w * d, b - d * (1 - w))
    else:
        v = a
    nan = torch.full((), float("nan"), dtype=dt, device=xt.device)
    return torch.where(valid[:, None] & ~torch.isnan(v), v, nan)


def _quantile(name: str, x, q, dim, keepdim: bool, interpolation: str, ignore_nan: bool):
    import torch

    if not isinstance(x, torch.Tensor):
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes a tensor")
    # what torch refuses, in its order and its words (it says quantile() for both functions)
    if x.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("quantile() input tensor must be either float or double dtype")
    if isinstance(q, torch.Tensor):
        if q.dtype != x.dtype:
            raise RuntimeError("quantile() q tensor must be same dtype as the input tensor")
        if q.dim() > 1:
            raise RuntimeError("quantile() q must be a scalar or 1D tensor")
        scalar_q = q.dim() == 0
        qs = [float(v) for v in q.reshape(-1).tolist()]  # (read to the host once)
        if not all(0.0 <= v <= 1.0 for v in qs):
            raise RuntimeError("quantile() q values must be in the range [0, 1]")
    else:
        scalar_q = True
        qs = [float(q)]
        if not 0.0 <= qs[0] <= 1.0:
            raise RuntimeError(f"quantile() q must be in the range [0, 1] but got {qs[0]:g}")
    if interpolation not in INTERPOLATIONS:
        raise RuntimeError(f"quantile() interpolation must be one of linear, lower, higher, midpoint or nearest, but got {interpolation}")
    if x.numel() == 0:
        raise RuntimeError("quantile() input tensor must be non-empty")
    if dim is not None:
        nd = max(x.dim(), 1)
        if not -nd <= dim < nd:
            raise IndexError(f"Dimension out of range (expected to be in range of [{-nd}, {nd - 1}], but got {dim})")
        dim %= nd
    if not x.is_cuda:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes a tensor on a GPU")
    if x.numel() >= 1 << 32:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes fewer than 2^32 elements")
    if dim is None:
        kept = (1,) * x.dim()
        x, dim = x.reshape(-1), 0
    else:
        kept = None
    if x.dim() == 0:
        x = x.reshape(1)
        squeeze0 = True
    else:
        squeeze0 = False
    moved = x.movedim(dim, -1)
    reduced = tuple(moved.shape[:-1])
    xt = aligned(moved.reshape(-1, moved.shape[-1]).contiguous())
    code = capi.VRS_SORT_FLOAT64 if x.dtype == torch.float64 else capi.VRS_SORT_FLOAT32
    if not qs:
        out = torch.empty((xt.shape[0], 0), dtype=x.dtype, device=x.device)
    elif len(qs) * _sides(interpolation) > capi.VRS_QUANTILE_MAX_TARGETS:
        out = _sort_rows(xt, qs, interpolation, ignore_nan)
    else:
        out = _select_rows(xt, code, qs, interpolation, ignore_nan)
    out = out.reshape(*reduced, len(qs)).movedim(-1, 0)  # (Q, *reduced)
    if keepdim:
        if kept is not None:
            out = out.reshape(len(qs), *kept)
        elif not squeeze0:
            out = out.unsqueeze(dim + 1)
    return out[0] if scalar_q else out


def quantile(x, q, dim=None, keepdim: bool = False, *, interpolation: str = "linear"):
    """torch.quantile(x, q, dim, keepdim, interpolation=...) of a float32 / float64 tensor on a GPU (any shape and strides, fewer than
    2^32 elements).  q: a Python float, or a 0-d / 1-d tensor of x's dtype (read to the host once), in [0, 1].  A scalar q answers the
    reduced shape, a 1-d q (Q, *reduced); dim=None reduces all elements.  A row with any NaN answers NaN.  Differences from torch: an
    order statistic that is a zero is +0.0 whatever its sign was; a NaN answered is the quiet NaN; inputs of more than 2^24 elements
    are answered (torch refuses them)."""
    return _quantile("quantile", x, q, dim, keepdim, interpolation, False)


def nanquantile(x, q, dim=None, keepdim: bool = False, *, interpolation: str = "linear"):
    """torch.nanquantile: quantile over the elements of every row that are not NaN; a row of NaNs alone answers NaN."""
    return _quantile("nanquantile", x, q, dim, keepdim, interpolation, True)
