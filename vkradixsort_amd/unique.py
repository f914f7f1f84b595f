"""Run-length encoding and unique: maximal runs of equal consecutive keys (vrs_run_length_encode) and the distinct keys of a buffer by
the stable one-call sort plus that encode (vrs_unique).

run_length_encode and unique_keys work on Buffers of a GPUContext; unique and unique_consecutive are torch.unique /
torch.unique_consecutive of an int32, int64, float32 or float64 tensor on a GPU, on torch's current stream.  With columns=C >= 2 (the
Buffer level) or dim=d (the torch level) the elements are rows of C words: the row form of the two calls, VRS_UNIQUE_COLUMNS(C).
"""
from __future__ import annotations

from . import capi
from ._torch import buffers, context_for, positions_to_int64
from .capi import VrsError

_KEY_TYPES = {"u32": capi.VRS_UNIQUE_U32, "i32": capi.VRS_UNIQUE_I32, "f32": capi.VRS_UNIQUE_F32,
              "u64": capi.VRS_UNIQUE_U64, "i64": capi.VRS_UNIQUE_I64, "f64": capi.VRS_UNIQUE_F64}


def _columns(columns: int) -> int:
    """what `columns` adds to key_type / key_bytes: nothing for the word form (0 or 1 column)"""
    if columns < 0 or columns >= 1 << 23:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "columns must be in [0, 2^23)")
    return capi.VRS_UNIQUE_COLUMNS(columns) if columns >= 2 else 0


def rle_scratch_bytes(num_elements: int, key_bytes: int = 4, counts: bool = False, columns: int = 1) -> int:
    """Bytes of scratch vrs_run_length_encode needs (no device); counts=True when out_counts is given without out_offsets.
    columns >= 2: the row form (num_elements rows of `columns` words)."""
    return capi.query_u64("vrs_run_length_encode_scratch_bytes", num_elements, key_bytes | _columns(columns), capi.VRS_RLE_COUNTS if counts else 0)


def unique_scratch_bytes(num_elements: int, key_type: str = "u32", inverse: bool = False, counts: bool = False, columns: int = 1) -> int:
    """Bytes of scratch vrs_unique needs for these outputs (no device).  columns >= 2: the row form (num_elements rows)."""
    if key_type not in _KEY_TYPES:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"key_type must be one of {sorted(_KEY_TYPES)}")
    flags = (capi.VRS_UNIQUE_INVERSE if inverse else 0) | (capi.VRS_UNIQUE_COUNTS if counts else 0)
    return capi.query_u64("vrs_unique_scratch_bytes", num_elements, _KEY_TYPES[key_type] | _columns(columns), flags)


def _h(b):
    return b.handle if b is not None else None


def run_length_encode(ctx, keys, num_elements: int, out_num_runs, scratch, key_bytes: int = 4, out_keys=None, out_offsets=None,
                      out_counts=None, out_run_ids=None, columns: int = 1) -> None:
    """The maximal runs of bit-identical consecutive keys of `keys` (4- or 8-byte keys, any order): out_keys[j], out_offsets[j] (and
    out_offsets[R] = n), out_counts[j] per run, out_run_ids[i] per element, out_num_runs[0] = R.  Any out_* may be None.  scratch: a
    Buffer of at least rle_scratch_bytes(...) bytes.  Stream-ordered on the context's stream.  columns >= 2: the row form -- num_elements
    rows of `columns` words row-major, runs of bit-identical rows, out_keys the R rows."""
    if scratch is None:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "run_length_encode needs a scratch Buffer of rle_scratch_bytes(...) bytes")
    ctx.check(ctx.lib.vrs_run_length_encode(ctx.handle, keys.handle, num_elements, key_bytes | _columns(columns), _h(out_keys), _h(out_offsets),
                                            _h(out_counts), _h(out_run_ids), out_num_runs.handle, scratch.handle))


def unique_keys(ctx, keys, num_elements: int, out_keys, out_num_runs, scratch, key_type: str = "u32", out_counts=None,
                out_inverse=None, columns: int = 1) -> None:
    """The distinct keys of `keys` in ascending order of key_type ("u32", "i32", "f32", "u64", "i64", "f64"; floats by the IEEE-754
    total order, equality of bit patterns) into out_keys, their occurrences into out_counts, the index of each element's key into
    out_inverse, R into out_num_runs[0].  scratch: a Buffer of at least unique_scratch_bytes(...) bytes.  Stream-ordered; may wait for
    the inner sort's plan, never for the sort.  columns >= 2: the row form -- num_elements rows of `columns` words row-major, the distinct
    rows in lexicographic order of the words' ranks."""
    if key_type not in _KEY_TYPES:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"key_type must be one of {sorted(_KEY_TYPES)}")
    if scratch is None:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "unique_keys needs a scratch Buffer of unique_scratch_bytes(...) bytes")
    ctx.check(ctx.lib.vrs_unique(ctx.handle, keys.handle, num_elements, _KEY_TYPES[key_type] | _columns(columns), out_keys.handle,
                                 _h(out_counts), _h(out_inverse), out_num_runs.handle, scratch.handle))


def _check_tensor(torch, x, name: str, dim):
    """the key type of x, and dim normalised (None stays None); with a dim, the refusals name it"""
    if dim is not None:
        nd = x.dim()
        if not isinstance(dim, int) or isinstance(dim, bool):
            raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name}: dim must be None or one int, not {dim!r}")
        if nd == 0:
            raise IndexError(f"Dimension specified as {dim} but tensor has no dimensions")
        if not -nd <= dim < nd:
            raise IndexError(f"Dimension out of range (expected to be in range of [{-nd}, {nd - 1}], but got {dim})")
        dim %= nd
        name = f"{name}(dim={dim})"
    if not x.is_cuda:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes a tensor on a GPU")
    if dim is None and not x.is_contiguous():
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes a contiguous tensor")
    types = {torch.int32: "i32", torch.int64: "i64", torch.float32: "f32", torch.float64: "f64"}
    if x.dtype not in types:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes int32, int64, float32 or float64, not {x.dtype}")
    if x.numel() >= 1 << 32:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes fewer than 2^32 elements")
    return types[x.dtype], dim


def _result(values, inverse, counts, return_inverse: bool, return_counts: bool):
    out = (values,) + ((inverse,) if return_inverse else ()) + ((counts,) if return_counts else ())
    return out[0] if len(out) == 1 else out


def _run(torch, x, return_inverse: bool, return_counts: bool, consecutive: bool, key_type: str, columns: int = 1):
    """x: contiguous, n elements (columns == 1) or [n, ...] with `columns` words per row.  -> (values of x's shape cut to R along dim 0,
    int64 inverse of n entries or None, int64 counts or None)"""
    n = x.numel() // columns
    device = x.device
    flat = x.view(-1)
    values = torch.empty_like(x)
    inverse = torch.empty(n if return_inverse else 0, dtype=torch.int32, device=device)
    counts = torch.empty(n if return_counts else 0, dtype=torch.int32, device=device)
    runs = torch.empty(1, dtype=torch.int32, device=device)
    kb = x.element_size()
    if consecutive:
        sb = rle_scratch_bytes(n, kb, counts=return_counts, columns=columns)
    else:
        sb = unique_scratch_bytes(n, key_type, inverse=return_inverse, counts=return_counts, columns=columns)
    scratch = torch.empty(max(sb, 4), dtype=torch.uint8, device=device)
    ctx = context_for(device)
    form = _columns(columns)
    with buffers(ctx, flat, values.view(-1), runs, scratch, inverse, counts) as (keys, out_keys, num_runs, scr, inv, cnt):
        if consecutive:
            ctx.check(ctx.lib.vrs_run_length_encode(ctx.handle, keys, n, kb | form, out_keys, None, cnt, inv, num_runs, scr))
        else:
            ctx.check(ctx.lib.vrs_unique(ctx.handle, keys, n, _KEY_TYPES[key_type] | form, out_keys, cnt, inv, num_runs, scr))
    R = int(runs.item())  # the one host synchronisation: the size of the result
    values = values.view(-1)[:R] if columns == 1 else values[:R]
    return (values, positions_to_int64(inverse, n) if return_inverse else None, positions_to_int64(counts[:R], n) if return_counts else None)


def _empty(torch, x, return_inverse: bool, return_counts: bool):
    return _result(torch.empty(0, dtype=x.dtype, device=x.device), torch.zeros(x.shape, dtype=torch.int64, device=x.device),
                   torch.empty(0, dtype=torch.int64, device=x.device), return_inverse, return_counts)


def _call(x, name: str, return_inverse: bool, return_counts: bool, dim, consecutive: bool):
    import torch

    key_type, dim = _check_tensor(torch, x, name, dim)
    if dim is None:
        if x.numel() == 0:
            return _empty(torch, x, return_inverse, return_counts)
        values, inv, cnt = _run(torch, x, return_inverse, return_counts, consecutive, key_type)
        return _result(values, inv.view(x.shape) if return_inverse else None, cnt, return_inverse, return_counts)
    if x.numel() == 0:
        if any(s == 0 for i, s in enumerate(x.shape) if i != dim):
            raise RuntimeError("There are 0 sized dimensions, and they aren't selected, so unique cannot be applied")
        return _result(torch.empty(x.shape, dtype=x.dtype, device=x.device), torch.empty(0, dtype=torch.int64, device=x.device),
                       torch.empty(0, dtype=torch.int64, device=x.device), return_inverse, return_counts)
    rows = x.movedim(dim, 0).contiguous()  # [N, *rest]: a row is the slice's elements in C order
    columns = rows.numel() // rows.shape[0]
    if columns >= 1 << 23:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name}(dim={dim}) takes rows of fewer than 2^23 elements")
    values, inv, cnt = _run(torch, rows, return_inverse, return_counts, consecutive, key_type, columns)
    if columns == 1:
        values = values.view(-1, *rows.shape[1:])
    return _result(values.movedim(0, dim), inv, cnt, return_inverse, return_counts)


def unique(x, sorted: bool = True, return_inverse: bool = False, return_counts: bool = False, dim=None):
    """torch.unique(x, sorted, return_inverse, return_counts, dim) of an int32, int64, float32 or float64 tensor on a GPU.
    dim=None (x contiguous): the distinct values ascending (also for sorted=False, as torch does on a GPU), the int64 index of each
    element's value shaped like x, and int64 counts -- the same tuple as torch for every flag combination.  Equal means bit-identical: the
    result equals torch.unique's for inputs without NaN and without -0.0.  The library keeps -0.0 and +0.0 apart (-0.0 first) and merges
    NaNs of the same bits, which sort by the IEEE-754 total order (a NaN with its sign bit set first, one without it last); torch merges
    -0.0 into +0.0 and keeps every NaN apart.
    dim=d (any strides): the distinct slices along d -- x seen as [N, C] rows, N = x.size(d), as torch's movedim(d, 0).reshape(N, -1) --
    in lexicographic order of the words by the same order and equality, shaped [R, *rest] moved back to d; inverse int64 [N], counts
    int64 [R].  One call of the row form of vrs_unique; R is read once.  An out-of-range d raises torch's IndexError, a zero-sized dim
    other than d torch's RuntimeError."""
    return _call(x, "unique", return_inverse, return_counts, dim, False)


def unique_consecutive(x, return_inverse: bool = False, return_counts: bool = False, dim=None):
    """torch.unique_consecutive(x, return_inverse, return_counts, dim) of an int32, int64, float32 or float64 tensor on a GPU.
    dim=None (x contiguous): one value per maximal run of equal consecutive elements (in flattened order), the int64 run of each element
    shaped like x, and int64 run lengths.  Equal means bit-identical (-0.0 and +0.0 start a new run, NaNs of the same bits do not), where
    torch compares values.  dim=d (any strides): one slice per maximal run of bit-identical consecutive slices along d, as unique's dim."""
    return _call(x, "unique_consecutive", return_inverse, return_counts, dim, True)
