"""The row form of the ordered compaction (vrs_compact_outputs.row_elems, header section "K15") without a device: the structures keep
their layout, vrs_compact_host with row_elems = W against numpy's values[flags != 0] and the row form of
out[i] = flag[i] ? source[rank(i)] : input[i], row_elems of 0 and 1 as the element form, the refusal of a short source, the word-width
rule through behaviour (bases off the 16-byte boundary, rows of 12, 20 and 4100 bytes), and the refusals of mask_index / mask_index_put
that need no device.

Everything is compared as bytes: there are no tolerances.  tests/test_gpu_mask_index.py holds the device to vrs_compact_host.
"""
import ctypes

import numpy as np
import pytest
import torch

import vkradixsort_amd as vrs
from vkradixsort_amd import capi

OK, REFUSED = capi.VRS_OK, capi.VRS_ERROR_INVALID_ARGUMENT
FLAG_CODES = {np.dtype(np.bool_): capi.VRS_COMPACT_BOOL, np.dtype(np.float32): capi.VRS_SORT_FLOAT32, np.dtype(np.int64): capi.VRS_SORT_INT64}
ROWS = [(2, 1), (3, 1), (3, 4), (4, 4), (5, 4), (6, 8), (256, 4)]  # (W, value_bytes)
SIZES = [1, 63, 4095, 4097, 16385]
PATTERNS = ["none", "all", "last", "half"]
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def pattern(name, n):
    if name == "none":
        return np.zeros(n, dtype=bool)
    if name == "all":
        return np.ones(n, dtype=bool)
    if name == "last":
        return np.arange(n) == n - 1
    return np.random.default_rng(n).random(n) < 0.5


def dress(mask, dtype):
    """flags of dtype that are nonzero exactly where mask is set: for floats NaN, a subnormal and -inf against both zeros"""
    n = mask.size
    if dtype == np.bool_:
        return mask.copy()
    if dtype == np.float32:
        nz = np.array([np.nan, 1e-45, -np.inf, 1.0], dtype=np.float32)
        z = np.array([0.0, -0.0], dtype=np.float32)
    else:
        nz = np.array([1, -1, np.iinfo(np.int64).min, 1 << 40], dtype=np.int64)
        z = np.array([0], dtype=np.int64)
    flags = np.where(mask, np.resize(nz, n), np.resize(z, n)).astype(dtype)
    assert np.array_equal(flags != 0, mask)  # (numpy's own predicate: -0.0 is zero, NaN is not)
    return flags


def address(a):
    return a.ctypes.data


def host_rows(lib, flags, W, vb, *, values=None, gather_out=None, scatter=None, scatter_out=None, source_elems=None, expect=OK):
    """vrs_compact_host on numpy arrays of bytes: values / gather_out, scatter = (input, source) / scatter_out.  Answers R."""
    o = capi.CompactHostOutputs()
    o.value_bytes, o.row_elems = vb, W
    if values is not None:
        o.gather_values, o.gather_out = address(values), address(gather_out)
    if scatter is not None:
        inp, src = scatter
        o.scatter_input, o.scatter_source, o.scatter_out = address(inp), address(src), address(scatter_out)
        o.scatter_source_elems = src.size // vb if source_elems is None else source_elems
    count = ctypes.c_uint64(1 << 50)
    rc = lib.vrs_compact_host(address(flags), flags.size, FLAG_CODES[flags.dtype], ctypes.byref(o), ctypes.byref(count))
    assert rc == expect, rc
    return count.value


def random_bytes(rng, rows, row_bytes):
    return rng.integers(0, 256, (rows, row_bytes), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- the structures

def test_structures_keep_their_layout():
    """size and offsets of the parent commit's structures, whose `reserved` word is now row_elems"""
    device = {"num_selected": 0, "flat": 8, "coords": 16, "coords_layout": 24, "ndim": 28, "shape": 32, "gather_values": 64, "gather_out": 72,
              "value_bytes": 80, "row_elems": 84, "scatter_input": 88, "scatter_source": 96, "scatter_out": 104}
    host = {"flat": 0, "coords": 8, "coords_layout": 16, "ndim": 20, "shape": 24, "gather_values": 56, "gather_out": 64, "value_bytes": 72,
            "row_elems": 76, "scatter_input": 80, "scatter_source": 88, "scatter_source_elems": 96, "scatter_out": 104}
    for structure, want in ((capi.CompactOutputs, device), (capi.CompactHostOutputs, host)):
        assert ctypes.sizeof(structure) == 112
        assert [name for name, _ in structure._fields_] == list(want)
        assert {name: getattr(structure, name).offset for name in want} == want
        assert getattr(structure, "row_elems").size == 4 and not hasattr(structure, "reserved")


# ---------------------------------------------------------------------------------------------- vrs_compact_host against numpy

@pytest.mark.parametrize("flag_dtype", [np.bool_, np.float32, np.int64], ids=["bool", "float32", "int64"])
@pytest.mark.parametrize("W,vb", ROWS, ids=[f"{w}x{b}" for w, b in ROWS])
def test_host_rows_against_numpy(lib, W, vb, flag_dtype):
    row_bytes = W * vb
    rng = np.random.default_rng(W * 16 + vb)
    for n in SIZES:
        values, source = random_bytes(rng, n, row_bytes), random_bytes(rng, n + 3, row_bytes)
        for name in PATTERNS:
            mask = pattern(name, n)
            flags = dress(mask, flag_dtype)
            R = int(mask.sum())
            # gather: out row r = values row position(r); nothing behind row R is written
            out = np.full((n + 1, row_bytes), SENTINEL, dtype=np.uint8)
            assert host_rows(lib, flags, W, vb, values=values, gather_out=out) == R, (n, name)
            assert np.array_equal(out[:R], values[flags != 0]), (n, name)
            assert (out[R:] == SENTINEL).all(), (n, name)
            # scatter: out row i = flag[i] ? source row rank(i) : input row i; a source of exactly R rows is enough
            want = values.copy()
            want[mask] = source[:R]
            for src in (source, source[:R]):
                got = np.full((n + 1, row_bytes), SENTINEL, dtype=np.uint8)
                assert host_rows(lib, flags, W, vb, scatter=(values, np.ascontiguousarray(src)), scatter_out=got) == R
                assert np.array_equal(got[:n], want), (n, name)
                assert (got[n:] == SENTINEL).all()


def test_gather_and_scatter_in_one_call(lib):
    n, W, vb = 4097, 5, 4
    rng = np.random.default_rng(2)
    mask = pattern("half", n)
    values, source = random_bytes(rng, n, W * vb), random_bytes(rng, n, W * vb)
    out, got = np.zeros((n, W * vb), dtype=np.uint8), np.zeros((n, W * vb), dtype=np.uint8)
    R = host_rows(lib, mask, W, vb, values=values, gather_out=out, scatter=(values, source), scatter_out=got)
    want = values.copy()
    want[mask] = source[:R]
    assert np.array_equal(out[:R], values[mask]) and np.array_equal(got, want)


@pytest.mark.parametrize("W", [0, 1])
def test_row_elems_of_0_and_1_are_the_element_form(lib, W):
    n = 4097
    rng = np.random.default_rng(3)
    mask = pattern("half", n)
    R = int(mask.sum())
    for dtype in (np.uint8, np.uint16, np.uint32, np.uint64):
        values = rng.integers(0, 200, n).astype(dtype)
        source = rng.integers(0, 200, R).astype(dtype)
        out, got = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
        vb = values.itemsize
        assert host_rows(lib, mask, W, vb, values=values, gather_out=out, scatter=(values, source), scatter_out=got, source_elems=R) == R
        want = values.copy()
        want[mask] = source
        assert np.array_equal(out[:R], values[mask]) and np.array_equal(got, want)


def test_a_source_below_R_rows_is_refused_with_nothing_written(lib):
    n, W, vb = 4097, 3, 4
    rng = np.random.default_rng(4)
    mask = pattern("half", n)
    R = int(mask.sum())
    values, source = random_bytes(rng, n, W * vb), random_bytes(rng, R, W * vb)
    got = np.full((n, W * vb), SENTINEL, dtype=np.uint8)
    for short in (R * W - 1, R * W - W, R, 0):  # (elements: one too few, one row too few, R elements where R rows are needed)
        host_rows(lib, mask, W, vb, scatter=(values, source), scatter_out=got, source_elems=short, expect=REFUSED)
        assert (got == SENTINEL).all()
    assert host_rows(lib, mask, W, vb, scatter=(values, source), scatter_out=got, source_elems=R * W) == R
    assert not (got == SENTINEL).all()


def test_a_row_form_past_2_62_bytes_is_refused(lib):
    flags = np.zeros(8, dtype=bool)
    o = capi.CompactHostOutputs()
    o.value_bytes, o.row_elems = 8, 2 ** 32 - 1
    o.gather_values = o.gather_out = address(flags)
    assert lib.vrs_compact_host(address(flags), 2 ** 32 - 1, capi.VRS_COMPACT_BOOL, ctypes.byref(o), None) == REFUSED


# ---------------------------------------------------------------------------------------------- the word-width rule, through behaviour

def offset_copy(a, offset):
    """a's bytes again, starting `offset` bytes behind a 64-byte boundary"""
    raw = np.zeros(a.size + 128, dtype=np.uint8)
    start = (-address(raw)) % 64 + offset
    view = raw[start:start + a.size].reshape(a.shape)
    view[...] = a
    assert address(view) % 64 == offset % 64
    return view


@pytest.mark.parametrize("W,vb", [(12, 1), (20, 1), (4100, 1), (3, 4), (5, 4), (1025, 4), (3, 2), (2, 8), (4, 4)],
                         ids=lambda v: str(v))
def test_bases_off_the_boundary_give_the_same_bytes(lib, W, vb):
    """every buffer in turn one element (and 2, 4, 8 bytes) behind a 16-byte boundary: the word the copy uses shrinks to 8, 4, 2 or 1
    bytes; the result does not change"""
    n, row_bytes = 4097, W * vb
    rng = np.random.default_rng(row_bytes)
    mask = pattern("half", n)
    R = int(mask.sum())
    values, source = random_bytes(rng, n, row_bytes), random_bytes(rng, R, row_bytes)
    want_gather = values[mask]
    want_scatter = values.copy()
    want_scatter[mask] = source
    for off in sorted({0, vb, 2, 4, 8} - {o for o in (2, 4, 8) if o % vb}):
        for moved in range(3):
            v = offset_copy(values, off if moved == 0 else 0)
            s = offset_copy(source, off if moved == 1 else 0)
            out = offset_copy(np.full((n, row_bytes), SENTINEL, dtype=np.uint8), off if moved == 2 else 0)
            got = offset_copy(np.full((n, row_bytes), SENTINEL, dtype=np.uint8), off if moved == 2 else 0)
            assert host_rows(lib, mask, W, vb, values=v, gather_out=out, scatter=(v, s), scatter_out=got) == R
            assert np.array_equal(out[:R], want_gather) and (out[R:] == SENTINEL).all(), (off, moved)
            assert np.array_equal(got, want_scatter), (off, moved)


# ---------------------------------------------------------------------------------------------- refusals that need no device

def test_exports():
    assert vrs.mask_index is not None and vrs.mask_index_put is not None


@pytest.mark.parametrize("mask_dtype", [torch.uint8, torch.int64, torch.float32], ids=str)
def test_a_mask_that_is_not_bool_is_refused(mask_dtype):
    x, m = torch.ones(4, 3), torch.ones(4, dtype=mask_dtype)
    with pytest.raises(IndexError):
        vrs.mask_index(x, m)
    with pytest.raises(IndexError):
        vrs.mask_index_put(x, m, x)


@pytest.mark.parametrize("shape", [(5,), (4, 2), (3,), (4, 3, 1), (1,)], ids=str)
def test_a_mask_of_another_shape_is_refused(shape):
    x, m = torch.ones(4, 3), torch.ones(shape, dtype=torch.bool)
    with pytest.raises(IndexError):
        vrs.mask_index(x, m)
    with pytest.raises(IndexError):
        vrs.mask_index_put(x, m, x)
    with pytest.raises(IndexError):
        x[m]  # (torch refuses the same pair)


def test_accumulate_is_refused():
    x, m = torch.ones(4, 3), torch.ones(4, dtype=torch.bool)
    with pytest.raises(vrs.VrsError) as e:
        vrs.mask_index_put(x, m, x, accumulate=True)
    assert e.value.code == REFUSED and "accumulate" in e.value.message


@pytest.mark.parametrize("shape", [(4, 2), (2,), (1, 4, 3), (3, 1, 3)], ids=str)
def test_values_that_do_not_broadcast_are_refused(shape):
    x, m = torch.ones(4, 3), torch.ones(4, dtype=torch.bool)
    with pytest.raises(RuntimeError):
        vrs.mask_index_put(x, m, torch.ones(shape))
    with pytest.raises(RuntimeError):
        torch.index_put(x, (m,), torch.ones(shape))  # (torch refuses the same values)


def test_values_of_another_dtype_are_refused():
    x, m = torch.ones(4, 3), torch.ones(4, dtype=torch.bool)
    with pytest.raises(RuntimeError):
        vrs.mask_index_put(x, m, torch.ones(4, 3, dtype=torch.float64))


def test_cpu_tensors_are_refused():
    x, m = torch.ones(4, 3), torch.ones(4, dtype=torch.bool)
    for call in (lambda: vrs.mask_index(x, m), lambda: vrs.mask_index_put(x, m, x), lambda: vrs.mask_index_put(x, m, 2.0)):
        with pytest.raises(vrs.VrsError) as e:
            call()
        assert e.value.code == REFUSED and "GPU" in e.value.message
