"""Run-length encoding and unique: maximal runs of equal consecutive keys (vrs_run_length_encode) and the distinct keys of a buffer by
the stable one-call sort plus that encode (vrs_unique).

run_length_encode and unique_keys work on Buffers of a GPUContext; unique and unique_consecutive are torch.unique /
torch.unique_consecutive of an int32, int64, float32 or float64 tensor on a GPU, on torch's current stream.
"""
from __future__ import annotations

from . import capi
from ._torch import buffers, context_for, positions_to_int64
from .capi import VrsError

_KEY_TYPES = {"u32": capi.VRS_UNIQUE_U32, "i32": capi.VRS_UNIQUE_I32, "f32": capi.VRS_UNIQUE_F32,
              "u64": capi.VRS_UNIQUE_U64, "i64": capi.VRS_UNIQUE_I64, "f64": capi.VRS_UNIQUE_F64}


def rle_scratch_bytes(num_elements: int, key_bytes: int = 4, counts: bool = False) -> int:
    """Bytes of scratch vrs_run_length_encode needs (no device); counts=True when out_counts is given without out_offsets."""
    return capi.query_u64("vrs_run_length_encode_scratch_bytes", num_elements, key_bytes, capi.VRS_RLE_COUNTS if counts else 0)


def unique_scratch_bytes(num_elements: int, key_type: str = "u32", inverse: bool = False, counts: bool = False) -> int:
    """Bytes of scratch vrs_unique needs for these outputs (no device)."""
    if key_type not in _KEY_TYPES:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"key_type must be one of {sorted(_KEY_TYPES)}")
    flags = (capi.VRS_UNIQUE_INVERSE if inverse else 0) | (capi.VRS_UNIQUE_COUNTS if counts else 0)
    return capi.query_u64("vrs_unique_scratch_bytes", num_elements, _KEY_TYPES[key_type], flags)


def _h(b):
    return b.handle if b is not None else None


def run_length_encode(ctx, keys, num_elements: int, out_num_runs, scratch, key_bytes: int = 4, out_keys=None, out_offsets=None,
                      out_counts=None, out_run_ids=None) -> None:
    """The maximal runs of bit-identical consecutive keys of `keys` (4- or 8-byte keys, any order): out_keys[j], out_offsets[j] (and
    out_offsets[R] = n), out_counts[j] per run, out_run_ids[i] per element, out_num_runs[0] = R.  Any out_* may be None.  scratch: a
    Buffer of at least rle_scratch_bytes(...) bytes.  Stream-ordered on the context's stream."""
    if scratch is None:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "run_length_encode needs a scratch Buffer of rle_scratch_bytes(...) bytes")
    ctx.check(ctx.lib.vrs_run_length_encode(ctx.handle, keys.handle, num_elements, key_bytes, _h(out_keys), _h(out_offsets), _h(out_counts),
                                            _h(out_run_ids), out_num_runs.handle, scratch.handle))


def unique_keys(ctx, keys, num_elements: int, out_keys, out_num_runs, scratch, key_type: str = "u32", out_counts=None,
                out_inverse=None) -> None:
    """The distinct keys of `keys` in ascending order of key_type ("u32", "i32", "f32", "u64", "i64", "f64"; floats by the IEEE-754
    total order, equality of bit patterns) into out_keys, their occurrences into out_counts, the index of each element's key into
    out_inverse, R into out_num_runs[0].  scratch: a Buffer of at least unique_scratch_bytes(...) bytes.  Stream-ordered; may wait for
    the inner sort's plan, never for the sort."""
    if key_type not in _KEY_TYPES:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"key_type must be one of {sorted(_KEY_TYPES)}")
    if scratch is None:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, "unique_keys needs a scratch Buffer of unique_scratch_bytes(...) bytes")
    ctx.check(ctx.lib.vrs_unique(ctx.handle, keys.handle, num_elements, _KEY_TYPES[key_type], out_keys.handle, _h(out_counts),
                                 _h(out_inverse), out_num_runs.handle, scratch.handle))


def _check_tensor(torch, x, name: str, dim):
    if dim is not None:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name}: only dim=None is supported")
    if not x.is_cuda:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes a tensor on a GPU")
    if not x.is_contiguous():
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes a contiguous tensor")
    types = {torch.int32: "i32", torch.int64: "i64", torch.float32: "f32", torch.float64: "f64"}
    if x.dtype not in types:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes int32, int64, float32 or float64, not {x.dtype}")
    if x.numel() >= 1 << 32:
        raise VrsError(capi.VRS_ERROR_INVALID_ARGUMENT, f"{name} takes fewer than 2^32 elements")
    return types[x.dtype]


def _result(values, inverse, counts, return_inverse: bool, return_counts: bool):
    out = (values,) + ((inverse,) if return_inverse else ()) + ((counts,) if return_counts else ())
    return out[0] if len(out) == 1 else out


def _run(torch, x, return_inverse: bool, return_counts: bool, consecutive: bool, key_type: str):
    n = x.numel()
    device = x.device
    flat = x.view(-1)
    values = torch.empty(n, dtype=x.dtype, device=device)
    inverse = torch.empty(n if return_inverse else 0, dtype=torch.int32, device=device)
    counts = torch.empty(n if return_counts else 0, dtype=torch.int32, device=device)
    runs = torch.empty(1, dtype=torch.int32, device=device)
    kb = x.element_size()
    if consecutive:
        sb = rle_scratch_bytes(n, kb, counts=return_counts)
    else:
        sb = unique_scratch_bytes(n, key_type, inverse=return_inverse, counts=return_counts)
    scratch = torch.empty(max(sb, 4), dtype=torch.uint8, device=device)
    ctx = context_for(device)
    with buffers(ctx, flat, values, runs, scratch, inverse, counts) as (keys, out_keys, num_runs, scr, inv, cnt):
        if consecutive:
            ctx.check(ctx.lib.vrs_run_length_encode(ctx.handle, keys, n, kb, out_keys, None, cnt, inv, num_runs, scr))
        else:
            ctx.check(ctx.lib.vrs_unique(ctx.handle, keys, n, _KEY_TYPES[key_type], out_keys, cnt, inv, num_runs, scr))
    R = int(runs.item())  # the one host synchronisation: the size of the result
    inv = positions_to_int64(inverse, n).view(x.shape) if return_inverse else None
    return _result(values[:R], inv, positions_to_int64(counts[:R], n) if return_counts else None, return_inverse, return_counts)


def _empty(torch, x, return_inverse: bool, return_counts: bool):
    return _result(torch.empty(0, dtype=x.dtype, device=x.device), torch.zeros(x.shape, dtype=torch.int64, device=x.device),
                   torch.empty(0, dtype=torch.int64, device=x.device), return_inverse, return_counts)


def unique(x, sorted: bool = True, return_inverse: bool = False, return_counts: bool = False, dim=None):
    """torch.unique(x, sorted, return_inverse, return_counts, dim=None) of a contiguous int32, int64, float32 or float64 tensor on a GPU:
    the distinct values ascending (also for sorted=False, as torch does on a GPU), the int64 index of each element's value shaped like x,
    and int64 counts -- the same tuple as torch for every flag combination.  Equal means bit-identical: the result equals torch.unique's
    for inputs without NaN and without -0.0.  The library keeps -0.0 and +0.0 apart (-0.0 first) and merges NaNs of the same bits, which
    sort by the IEEE-754 total order (a NaN with its sign bit set first, one without it last); torch merges -0.0 into +0.0 and keeps
    every NaN apart."""
    import torch

    key_type = _check_tensor(torch, x, "unique", dim)
    if x.numel() == 0:
        return _empty(torch, x, return_inverse, return_counts)
    return _run(torch, x, return_inverse, return_counts, False, key_type)


def unique_consecutive(x, return_inverse: bool = False, return_counts: bool = False, dim=None):
    """torch.unique_consecutive(x, return_inverse, return_counts, dim=None) of a contiguous int32, int64, float32 or float64 tensor on a
    GPU: one value per maximal run of equal consecutive elements (in flattened order), the int64 run of each element shaped like x, and
    int64 run lengths.  Equal means bit-identical (-0.0 and +0.0 start a new run, NaNs of the same bits do not), where torch compares
    values."""
    import torch

    key_type = _check_tensor(torch, x, "unique_consecutive", dim)
    if x.numel() == 0:
        return _empty(torch, x, return_inverse, return_counts)
    return _run(torch, x, return_inverse, return_counts, True, key_type)
