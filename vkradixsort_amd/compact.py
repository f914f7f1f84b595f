"""torch.nonzero, argwhere, where(condition), count_nonzero, masked_select and masked_scatter drop-ins, and x[mask] / index_put for a mask
over the leading dims (mask_index, mask_index_put): ordered stream compaction (vrs_compact_count + vrs_compact_emit).

The flags are read in their own dtype (bool and the nine dtypes of the sort drop-ins; no `x != 0` pass), counted per tile, the counts
scanned, and the survivors written in input order: positions, coordinates, gathered values, or the scatter form.  Outputs are integers
and copied bits, so every function equals torch's CPU result bit for bit; -0.0 is zero, NaNs are nonzero, NaN payloads survive a copy.
nonzero, masked_select and masked_scatter read the count R on the host once, as torch does; count_nonzero does not.

Not offered: stable partition, out=, in-place masked_scatter_ / masked_fill, count_nonzero over a dim, three-argument where, complex
dtypes, 2^32 elements or more.  A tensor that is not contiguous (a broadcast mask too) is made contiguous first.
"""
from __future__ import annotations

import ctypes

from . import capi
from ._torch import aligned, buffers, context_for
from .binning import _on_gpu
from .capi import VrsError


def _refuse(message: str):
    raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, message)


def _flag_code(torch, dtype, name: str) -> int:
    codes = {torch.int8: capi.VRS_SORT_INT8, torch.uint8: capi.VRS_SORT_UINT8, torch.int16: capi.VRS_SORT_INT16,
             torch.int32: capi.VRS_SORT_INT32, torch.int64: capi.VRS_SORT_INT64, torch.float16: capi.VRS_SORT_FLOAT16,
             torch.bfloat16: capi.VRS_SORT_BFLOAT16, torch.float32: capi.VRS_SORT_FLOAT32, torch.float64: capi.VRS_SORT_FLOAT64,
             torch.bool: capi.VRS_COMPACT_BOOL}
    if dtype not in codes:
        _refuse(f"{name} takes bool, int8, uint8, int16, int32, int64, float16, bfloat16, float32 or float64, not {dtype}")
    return codes[dtype]


def compact_stats(ctx) -> dict:
    """Count calls, emit calls and the elements the count calls were given on this context so far (cumulative)."""
    c = [ctypes.c_uint64() for _ in range(3)]
    ctx.check(ctx.lib.vrs_compact_stats(ctx.handle, *(ctypes.byref(v) for v in c)))
    return {"count_calls": c[0].value, "emit_calls": c[1].value, "elements": c[2].value}


def _tensor(name: str, x):
    import torch

    if not isinstance(x, torch.Tensor):
        _refuse(f"{name} takes a tensor")
    if x.dtype.is_complex:
        _refuse(f"{name} takes no complex dtype")
    return torch


class _Counted:
    """The flags of one call after count and carries: the context, the scratch the emit reads, and R when it was asked for."""

    def __init__(self, name: str, flags, *, host: bool, device_count=None):
        import torch

        n = flags.numel()
        if n >= 1 << 32:
            _refuse(f"{name} takes fewer than 2^32 elements")
        self.flags = aligned(flags.contiguous()).reshape(-1)
        self.n, self.code = n, _flag_code(torch, flags.dtype, name)
        self.ctx = context_for(flags.device)
        tile = self.ctx.tuned(capi.VRS_TUNE_COMPACT_TILE_ELEMS)
        need = capi.query_u64("vrs_compact_scratch_bytes", n, tile)
        self.scratch = torch.empty(need, dtype=torch.uint8, device=flags.device)
        got = ctypes.c_uint64()
        with buffers(self.ctx, self.flags, self.scratch, device_count) as (f, s, c):
            self.ctx.check(self.ctx.lib.vrs_compact_count(self.ctx.handle, f, n, self.code, s, c, ctypes.byref(got) if host else None))
        self.R = got.value if host else None

    def emit(self, *, flat=None, coords=None, layout=capi.VRS_COMPACT_ROWS, shape=(), gather=None, gather_out=None, scatter=None,
             row_elems=0, value_bytes=None):
        """vrs_compact_emit into the given tensors; scatter = (input, source, out).  row_elems >= 2: the row form, every flag a row of
        that many elements of value_bytes (the tensors' element size unless given)."""
        o = capi.CompactOutputs()
        o.num_selected, o.row_elems = self.R, row_elems
        inp, src, out = scatter or (None, None, None)
        value = gather if gather is not None else inp
        with buffers(self.ctx, self.flags, self.scratch, flat, coords, gather, gather_out, inp, src, out) as (f, s, *handles):
            fl, co, gv, go, si, ss, so = (h.value if h is not None else None for h in handles)  # (a structure's field takes the address)
            o.flat, o.coords, o.coords_layout = fl, co, layout
            if coords is not None:
                o.ndim = len(shape)
                o.shape = (ctypes.c_uint32 * 8)(*shape)
            o.gather_values, o.gather_out = gv, go
            o.value_bytes = value_bytes or (value.element_size() if value is not None else 0)
            o.scatter_input, o.scatter_source, o.scatter_out = si, ss, so
            self.ctx.check(self.ctx.lib.vrs_compact_emit(self.ctx.handle, f, self.n, self.code, s, ctypes.byref(o)))


def _strides(shape):
    out, stride = [], 1
    for size in reversed(shape):
        out.append(stride)
        stride *= size
    return out[::-1]


def _coordinates(name: str, x, columns: bool):
    """The survivors' coordinates as int64 [ndim, R] (columns) or [R, ndim]; x has one dim or more."""
    import torch

    shape = tuple(x.shape)
    ndim, device = len(shape), x.device
    if x.numel() == 0:
        return torch.empty((ndim, 0) if columns else (0, ndim), dtype=torch.int64, device=device)
    counted = _Counted(name, x, host=True)
    R = counted.R
    if ndim <= capi.COMPACT_MAX_DIMS:
        out = torch.empty((ndim, R) if columns else (R, ndim), dtype=torch.int64, device=device)
        if R and ndim == 1:  # (one dim: the coordinates are the flat positions, in either layout)
            counted.emit(flat=out.reshape(-1))
        elif R:
            counted.emit(coords=out, layout=capi.VRS_COMPACT_COLUMNS if columns else capi.VRS_COMPACT_ROWS, shape=shape)
        return out
    # more dims than the kernel decomposes: its flat positions, taken apart by torch
    flat = torch.empty(R, dtype=torch.int64, device=device)
    if R:
        counted.emit(flat=flat)
    cols = [(flat // stride) % size for stride, size in zip(_strides(shape), shape)]
    return torch.stack(cols, 0 if columns else 1)


def nonzero(x, *, as_tuple: bool = False):
    """torch.nonzero(x, as_tuple=False) on a GPU: the coordinates of the nonzero elements in row-major order, int64 [R, ndim], or with
    as_tuple one contiguous 1-D tensor per dim.  A 0-dim tensor gives [R, 0], and with as_tuple counts as 1-D, as torch."""
    _tensor("nonzero", x)
    _on_gpu("nonzero", x)
    if as_tuple:
        return tuple(_coordinates("nonzero", x.reshape(1) if x.dim() == 0 else x, True).unbind(0))
    if x.dim() == 0:
        return _coordinates("nonzero", x.reshape(1), False)[:, :0]
    return _coordinates("nonzero", x, False)


def argwhere(x):
    """torch.argwhere(x) on a GPU: nonzero(x)."""
    _tensor("argwhere", x)
    _on_gpu("argwhere", x)
    return nonzero(x)


def where(condition):
    """torch.where(condition), the one-argument form, on a GPU: nonzero(condition, as_tuple=True)."""
    _tensor("where", condition)
    _on_gpu("where", condition)
    return nonzero(condition, as_tuple=True)


def count_nonzero(x):
    """torch.count_nonzero(x) over the whole tensor on a GPU: a 0-dim int64 tensor on the device, without a host read."""
    torch = _tensor("count_nonzero", x)
    _on_gpu("count_nonzero", x)
    if x.numel() == 0:
        return torch.zeros((), dtype=torch.int64, device=x.device)
    out = torch.empty(1, dtype=torch.int64, device=x.device)
    _Counted("count_nonzero", x, host=False, device_count=out)
    return out.reshape(())


def _masked(name: str, x, mask):
    """x and mask checked and broadcast against each other."""
    torch = _tensor(name, x)
    if not isinstance(mask, torch.Tensor):
        _refuse(f"{name} takes a tensor mask")
    if mask.dtype != torch.bool:
        raise RuntimeError(f"{name}: expected BoolTensor for mask")
    if x.element_size() not in (1, 2, 4, 8):
        _refuse(f"{name} takes elements of 1, 2, 4 or 8 bytes")
    x, mask = torch.broadcast_tensors(x, mask)  # (RuntimeError when the shapes do not broadcast, as torch)
    _on_gpu(name, x, mask)
    return torch, x, mask


def masked_select(x, mask):
    """torch.masked_select(x, mask) on a GPU (what x[mask] becomes): the elements of x where the bool mask is set, in row-major order of
    the broadcast shape, as a 1-D tensor of x's dtype.  Values are copied as bits."""
    torch, x, mask = _masked("masked_select", x, mask)
    if x.numel() == 0:
        return torch.empty(0, dtype=x.dtype, device=x.device)
    counted = _Counted("masked_select", mask, host=True)
    out = torch.empty(counted.R, dtype=x.dtype, device=x.device)
    if counted.R:
        counted.emit(gather=aligned(x.contiguous()).reshape(-1), gather_out=out)
    return out


def masked_scatter(x, mask, source):
    """torch.masked_scatter(x, mask, source) on a GPU, out of place: a copy of x (broadcast against the bool mask) whose elements under a
    set mask are source's elements in order.  RuntimeError when source has fewer elements than the mask has set, as torch on the CPU."""
    torch, x, mask = _masked("masked_scatter", x, mask)
    if not isinstance(source, torch.Tensor):
        _refuse("masked_scatter takes a tensor source")
    if source.dtype != x.dtype:
        raise RuntimeError(f"masked_scatter: expected self and source to have same dtypes but got {x.dtype} and {source.dtype}")
    _on_gpu("masked_scatter", x, source)
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    if x.numel() == 0:
        return out
    counted = _Counted("masked_scatter", mask, host=True)
    if source.numel() < counted.R:
        raise RuntimeError(f"masked_scatter: source has {source.numel()} elements, the mask sets {counted.R}")
    src = aligned(source.contiguous()).reshape(-1)
    counted.emit(scatter=(aligned(x.contiguous()).reshape(-1), src, out.reshape(-1)))
    return out


# ---------------------------------------------------------------------------------------------- a mask over the leading dims: rows

def _row_mask(name: str, x, mask):
    """x and a bool mask over x's leading dims, refused as torch's indexing refuses them: (torch, the shape of one row)."""
    import torch

    if not isinstance(x, torch.Tensor) or not isinstance(mask, torch.Tensor):
        _refuse(f"{name} takes tensors")
    if mask.dtype != torch.bool:
        raise IndexError(f"{name}: the mask is a bool tensor, not {mask.dtype} (indexing by integer tensors is not offered)")
    if mask.dim() > x.dim() or tuple(mask.shape) != tuple(x.shape[:mask.dim()]):
        raise IndexError(f"{name}: the shape of the mask {list(mask.shape)} does not match the leading dims of the indexed tensor "
                         f"{list(x.shape)}")
    if x.element_size() not in (1, 2, 4, 8, 16):
        _refuse(f"{name} takes elements of 1, 2, 4, 8 or 16 bytes")
    return torch, tuple(x.shape[mask.dim():])


def _row_width(name: str, x, tail):
    """(value_bytes, row_elems) of one row of x: bits are copied, so an element of 16 bytes goes in as two of 8."""
    value_bytes = min(x.element_size(), 8)
    row_elems = x.element_size() // value_bytes
    for size in tail:
        row_elems *= size
    if row_elems >= 1 << 32:
        _refuse(f"{name} takes rows of fewer than 2^32 elements")
    return value_bytes, row_elems


def mask_index(x, mask):
    """x[mask] on a GPU for a bool mask over x's leading dims (mask.shape == x.shape[:mask.dim()]): the rows of x under a set flag, in
    order, as [R, *x.shape[mask.dim():]].  Every flag moves a whole row as dense words; a mask of x's own shape takes the element kernels, as masked_select.
    Bits are copied (any dtype of 1, 2, 4, 8 or 16 bytes).  IndexError for a mask that is not bool or whose shape does not match, as
    torch.  One host read of R, as torch makes.  Not offered: a mask over other dims (x[:, mask]), integer-tensor indices."""
    torch, tail = _row_mask("mask_index", x, mask)
    _on_gpu("mask_index", x, mask)
    if mask.numel() == 0:
        return torch.empty((0, *tail), dtype=x.dtype, device=x.device)
    counted = _Counted("mask_index", mask, host=True)
    out = torch.empty((counted.R, *tail), dtype=x.dtype, device=x.device)
    if out.numel():
        value_bytes, row_elems = _row_width("mask_index", x, tail)
        counted.emit(gather=aligned(x.contiguous()).reshape(-1), gather_out=out.reshape(-1), row_elems=row_elems, value_bytes=value_bytes)
    return out


def mask_index_put(x, mask, values, accumulate: bool = False):
    """torch.index_put(x, (mask,), values) on a GPU, out of place, for a bool mask over x's leading dims: a copy of x whose rows under a
    set flag are the rows of values in order.  values of exactly [R, *x.shape[mask.dim():]] and contiguous is read where it lies;
    anything else that broadcasts to that shape is expanded first, and what does not is a RuntimeError.  Not offered: accumulate=True,
    the in-place x[mask] = values."""
    torch, tail = _row_mask("mask_index_put", x, mask)
    if accumulate:
        _refuse("mask_index_put takes no accumulate=True")
    if not isinstance(values, torch.Tensor):
        values = torch.as_tensor(values, dtype=x.dtype, device=x.device)
    if values.dtype != x.dtype:
        raise RuntimeError(f"mask_index_put: expected self and values to have same dtypes but got {x.dtype} and {values.dtype}")
    shape = tuple(values.shape)
    if len(shape) > len(tail) + 1 or any(v not in (1, t) for v, t in zip(reversed(shape), reversed(tail))):
        raise RuntimeError(f"mask_index_put: values of shape {list(shape)} do not broadcast to [R, {', '.join(map(str, tail))}]")
    _on_gpu("mask_index_put", x, mask, values)
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    if x.numel() == 0:
        return out
    counted = _Counted("mask_index_put", mask, host=True)
    target = (counted.R, *tail)
    if len(shape) == len(target) and shape[0] not in (1, counted.R):
        raise RuntimeError(f"mask_index_put: values of shape {list(shape)} do not broadcast to {list(target)}")
    if shape != target or not values.is_contiguous():
        values = values.expand(target).contiguous()
    value_bytes, row_elems = _row_width("mask_index_put", x, tail)
    counted.emit(scatter=(aligned(x.contiguous()).reshape(-1), aligned(values).reshape(-1), out.reshape(-1)),
                 row_elems=row_elems, value_bytes=value_bytes)
    return out
