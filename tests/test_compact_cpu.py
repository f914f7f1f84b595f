"""Ordered stream compaction (vrs_compact_*, header section "K15") without a device: the pure companions, the predicate, order and
coordinate arithmetic of vrs_compact_host against numpy, the division by constants against // and %, the scatter form, and the
torch-level refusals.

vrs_compact_host compiles the functions the kernels compile (csrc/vrs_compact_order.hpp); tests/test_gpu_compact.py holds the device to
it and to torch bit for bit, so what is pinned here is pinned for the device too.
"""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

import vkradixsort_amd as vrs
from vkradixsort_amd import capi

CODES = {torch.int8: capi.VRS_SORT_INT8, torch.uint8: capi.VRS_SORT_UINT8, torch.int16: capi.VRS_SORT_INT16, torch.int32: capi.VRS_SORT_INT32,
         torch.int64: capi.VRS_SORT_INT64, torch.float16: capi.VRS_SORT_FLOAT16, torch.bfloat16: capi.VRS_SORT_BFLOAT16,
         torch.float32: capi.VRS_SORT_FLOAT32, torch.float64: capi.VRS_SORT_FLOAT64, torch.bool: capi.VRS_COMPACT_BOOL}
DTYPES = list(CODES)
BITS = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
T_DEFAULT, T_MIN, T_MAX = capi.COMPACT_TILE_ELEMS_DEFAULT, capi.COMPACT_TILE_ELEMS_MIN, capi.COMPACT_TILE_ELEMS_MAX
ROWS, COLUMNS = capi.VRS_COMPACT_ROWS, capi.VRS_COMPACT_COLUMNS
SHAPES = [(7,), (3, 5), (2, 1, 4, 3), (2, 1, 3, 1, 2, 1, 2, 3), (1, 65537), (65537, 1)]


def name_of(dtype):
    return str(dtype).replace("torch.", "")


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def bits(t):
    """the tensor's bytes as integers of its width (NaN payloads and the sign of zero compare)"""
    return t.contiguous().view(BITS[t.element_size()])


def specials(dtype):
    """the values the predicate has to get right, as a 1-D tensor of dtype"""
    if dtype == torch.bool:
        return torch.tensor([False, True, True, False])
    if dtype in (torch.float16, torch.bfloat16):
        # +0, -0, the smallest subnormal, NaNs of both signs (0x7e00 / 0xfe00; bfloat16 reads them as NaNs with a payload), infinities
        inf = 0x7c00 if dtype == torch.float16 else 0x7f80
        raw = [0x0000, 0x8000, 0x0001, 0x8001, 0x7e00, 0xfe00, inf, inf | 0x8000, 0x3c00, 0x7fff, 0xffff]
        return torch.tensor(np.array(raw, dtype=np.uint16).view(np.int16)).view(dtype)
    if dtype.is_floating_point:
        tiny = torch.finfo(dtype).smallest_normal * torch.finfo(dtype).eps  # the smallest subnormal
        nan = torch.tensor([float("nan")], dtype=dtype)
        neg_nan = (bits(nan) | torch.iinfo(BITS[nan.element_size()]).min).view(dtype)
        v = torch.tensor([0.0, -0.0, tiny, -tiny, float("inf"), float("-inf"), 1.0, -1.5], dtype=dtype)
        assert v[2] != 0 and v[2] / 2 == 0
        return torch.cat([v, nan, neg_nan])
    info = torch.iinfo(dtype)
    return torch.tensor([0, info.min, -1 if info.min < 0 else info.max, 1, info.max, 0], dtype=dtype)


def make_input(dtype, shape, seed=0):
    """a tensor of `shape` made of the specials, about half of them zeros of either sign, in a seeded order"""
    s = specials(dtype)
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(seed)
    pick = torch.randint(0, len(s), (n,), generator=g)
    zero = torch.rand(n, generator=g) < 0.5
    pick[zero] = torch.randint(0, 2, (int(zero.sum()),), generator=g) if dtype.is_floating_point else 0
    pick[-1] = 2 if dtype.is_floating_point else 1 if dtype == torch.bool else 3  # (the last element is set, so that the largest coordinate appears)
    return s[pick].reshape(shape)


def truth(x):
    """numpy's idea of x != 0, elementwise (float16 and bfloat16 widened exactly)"""
    if x.dtype in (torch.float16, torch.bfloat16):
        x = x.float()
    return x.numpy() != 0


def host_compact(lib, x, *, flat=False, coords=None, values=None, scatter=None, expect=capi.VRS_OK):
    """vrs_compact_host of the CPU tensor x.  coords: ROWS or COLUMNS; values: a tensor of x's shape to gather from; scatter: (input,
    source).  Answers a dict of what was asked for, and "count"."""
    x = x.contiguous()
    n = x.numel()
    o = capi.CompactHostOutputs()
    keep = {}
    if flat:
        keep["flat"] = torch.full((n,), -7, dtype=torch.int64)
        o.flat = keep["flat"].data_ptr()
    if coords is not None:
        shape = tuple(x.shape)
        keep["coords"] = torch.full((n * len(shape),), -7, dtype=torch.int64)
        o.coords, o.coords_layout, o.ndim = keep["coords"].data_ptr(), coords, len(shape)
        o.shape = (ctypes.c_uint32 * 8)(*shape)
    if values is not None:
        values = values.contiguous()
        keep["gather"] = torch.zeros(n, dtype=values.dtype)
        o.gather_values, o.gather_out, o.value_bytes = values.data_ptr(), keep["gather"].data_ptr(), values.element_size()
    if scatter is not None:
        inp, src = (t.contiguous() for t in scatter)
        keep["scatter"] = torch.zeros(n, dtype=inp.dtype)
        o.scatter_input, o.scatter_source, o.scatter_source_elems = inp.data_ptr(), src.data_ptr(), src.numel()
        o.scatter_out, o.value_bytes = keep["scatter"].data_ptr(), inp.element_size()
    count = ctypes.c_uint64(123)
    rc = lib.vrs_compact_host(x.data_ptr(), n, CODES[x.dtype], ctypes.byref(o), ctypes.byref(count))
    assert rc == expect, rc
    R = count.value
    out = {"count": R}
    if flat:
        assert (keep["flat"][R:] == -7).all()
        out["flat"] = keep["flat"][:R]
    if coords is not None:
        nd = len(x.shape)
        assert (keep["coords"][R * nd:] == -7).all()
        out["coords"] = keep["coords"][:R * nd].reshape((R, nd) if coords == ROWS else (nd, R))
    if values is not None:
        out["gather"] = keep["gather"][:R]
    if scatter is not None:
        out["scatter"] = keep["scatter"]
    return out


# ---------------------------------------------------------------------------------------------- pure functions

def _query(fn, ctype, *args):
    out = ctype()
    return fn(*args, ctypes.byref(out)), out.value


@pytest.mark.parametrize("T", [T_MIN, T_DEFAULT, T_MAX])
def test_tiles_and_scratch_bytes(lib, T):
    for n in (0, 1, T - 1, T, T + 1, 2 ** 32 - 1):
        rc, tiles = _query(lib.vrs_compact_tiles_for, ctypes.c_uint32, n, T)
        assert rc == capi.VRS_OK and tiles == -(-n // T), (n, T)
        rc, nbytes = _query(lib.vrs_compact_scratch_bytes, ctypes.c_uint64, n, T)
        assert rc == capi.VRS_OK and nbytes % 256 == 0
        assert 256 + 4 * tiles <= nbytes < 256 + 4 * tiles + 256, (n, T, nbytes)


def test_2_32_elements_and_more_are_refused(lib):
    for n in (2 ** 32, 2 ** 32 + 1, 2 ** 40, 2 ** 64 - 1):
        assert _query(lib.vrs_compact_tiles_for, ctypes.c_uint32, n, T_DEFAULT)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
        assert _query(lib.vrs_compact_scratch_bytes, ctypes.c_uint64, n, T_DEFAULT)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
        assert lib.vrs_compact_host(None, n, capi.VRS_COMPACT_BOOL, None, None) == capi.VRS_ERROR_INVALID_ARGUMENT


def test_tile_key_number_default_and_range(lib):
    assert capi.VRS_TUNE_COMPACT_TILE_ELEMS == 40
    assert (T_DEFAULT, T_MIN, T_MAX) == (16384, 4096, 65536) and T_DEFAULT % 4096 == 0
    assert capi.COMPACT_CHUNK == 4096 and capi.COMPACT_CARRY_BLOCK == 4096 and capi.COMPACT_MAX_DIMS == 8
    header = (Path(__file__).resolve().parent.parent / "include" / "vkradixsort_amd_tune.h").read_text()
    assert "VRS_TUNE_COMPACT_TILE_ELEMS = 40" in header and "Default 16384" in header
    for T in (0, 1, 2048, 4095, 4097, 6144, T_MAX + 4096, 2 ** 31):
        assert _query(lib.vrs_compact_tiles_for, ctypes.c_uint32, 1000, T)[0] == capi.VRS_ERROR_INVALID_ARGUMENT, T
        assert _query(lib.vrs_compact_scratch_bytes, ctypes.c_uint64, 1000, T)[0] == capi.VRS_ERROR_INVALID_ARGUMENT, T
    for T in range(T_MIN, T_MAX + 1, 4096):
        assert _query(lib.vrs_compact_tiles_for, ctypes.c_uint32, 1000, T) == (capi.VRS_OK, 1)
    for name in ("vrs_compact_count", "vrs_compact_emit", "vrs_compact_tiles_for", "vrs_compact_scratch_bytes", "vrs_compact_divide",
                 "vrs_compact_host", "vrs_compact_stats"):
        assert name in capi.EXPORTED_SYMBOLS


def test_device_calls_refuse_without_a_context(lib):
    assert lib.vrs_compact_count(None, None, 10, capi.VRS_COMPACT_BOOL, None, None, None) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_compact_emit(None, None, 10, capi.VRS_COMPACT_BOOL, None, None) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_compact_stats(None, None, None, None) == capi.VRS_ERROR_INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------- division by constants

DIVISORS = sorted({1, 2, 3, 2 ** 32 - 1} | {d for k in range(1, 32) for d in (2 ** k - 1, 2 ** k, 2 ** k + 1)})


def _divide(lib, a, d):
    q, r = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.vrs_compact_divide(a, d, ctypes.byref(q), ctypes.byref(r)) == capi.VRS_OK
    return q.value, r.value


def test_division_at_the_edges(lib):
    assert lib.vrs_compact_divide(5, 0, None, None) == capi.VRS_ERROR_INVALID_ARGUMENT
    for d in DIVISORS:
        for a in (0, 1, d - 1, d, d + 1, 2 ** 31 - 1, 2 ** 31 + 1, 2 ** 32 - 1):
            if a < 2 ** 32:
                assert _divide(lib, a, d) == (a // d, a % d), (a, d)


def test_division_of_random_numerators(lib):
    rng = np.random.default_rng(15)
    numerators = rng.integers(0, 2 ** 32, 100000, dtype=np.uint64)
    divisors = np.array(DIVISORS, dtype=np.uint64)[rng.integers(0, len(DIVISORS), numerators.size)]
    fn, q, r = lib.vrs_compact_divide, ctypes.c_uint32(), ctypes.c_uint32()
    pq, pr = ctypes.byref(q), ctypes.byref(r)
    for a, d in zip(numerators.tolist(), divisors.tolist()):
        fn(a, d, pq, pr)
        assert (q.value, r.value) == (a // d, a % d), (a, d)


# ---------------------------------------------------------------------------------------------- vrs_compact_host against numpy

def test_specials_hold_what_the_issue_names():
    for dtype in (torch.float16, torch.bfloat16):
        raw = set((bits(specials(dtype)).numpy().view(np.uint16)).tolist())
        assert {0x0000, 0x8000, 0x0001, 0x7e00, 0xfe00} <= raw
    for dtype in (torch.int8, torch.int16, torch.int32, torch.int64):
        s = specials(dtype).tolist()
        assert torch.iinfo(dtype).min in s and -1 in s


@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_predicate_on_every_special(lib, dtype):
    s = specials(dtype)
    got = host_compact(lib, s, flat=True)
    want = np.flatnonzero(truth(s))
    assert got["count"] == want.size and np.array_equal(got["flat"].numpy(), want)
    if dtype.is_floating_point:  # -0.0 is zero; NaNs of both signs, infinities and the subnormals are not
        assert got["flat"].tolist() == list(range(2, s.numel()))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_host_against_numpy(lib, dtype, shape):
    x = make_input(dtype, shape, seed=len(shape))
    t = truth(x)
    want_rows = np.argwhere(t)
    values = torch.arange(x.numel(), dtype=torch.int32).reshape(shape)
    got = host_compact(lib, x, flat=True, coords=ROWS, values=values)
    assert got["count"] == want_rows.shape[0] > 0
    assert np.array_equal(got["flat"].numpy(), np.flatnonzero(t))
    assert np.array_equal(got["coords"].numpy(), want_rows)
    assert np.array_equal(got["gather"].numpy(), values.numpy()[t])
    cols = host_compact(lib, x, coords=COLUMNS)["coords"]
    assert np.array_equal(cols.numpy(), want_rows.T)
    if max(shape) > 65536:
        assert got["coords"].max() >= 65536  # (a coordinate passes 2^16)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.bfloat16, torch.float32, torch.float64], ids=name_of)
def test_gather_copies_bits(lib, dtype):
    """boolean indexing, value for value and bit for bit: NaN payloads and -0.0 survive"""
    mask = make_input(torch.bool, (3, 41), seed=3)
    values = make_input(dtype, (3, 41), seed=4)
    got = host_compact(lib, mask, values=values)["gather"]
    assert torch.equal(bits(got), bits(values)[mask])


def test_empty_and_all_zero(lib):
    assert lib.vrs_compact_host(None, 0, capi.VRS_COMPACT_BOOL, None, None) == capi.VRS_OK
    got = host_compact(lib, torch.zeros(100, dtype=torch.float32) * -1.0, flat=True, coords=ROWS)
    assert got["count"] == 0 and got["flat"].numel() == 0 and got["coords"].shape == (0, 1)


def test_host_refusals(lib):
    x = torch.ones(6, dtype=torch.int32)
    o = capi.CompactHostOutputs()
    coords = torch.empty(12, dtype=torch.int64)
    o.coords, o.ndim, o.shape = coords.data_ptr(), 2, (ctypes.c_uint32 * 8)(2, 4)  # the product is not n
    assert lib.vrs_compact_host(x.data_ptr(), 6, CODES[x.dtype], ctypes.byref(o), None) == capi.VRS_ERROR_INVALID_ARGUMENT
    o.ndim, o.shape = 9, (ctypes.c_uint32 * 8)(6)
    assert lib.vrs_compact_host(x.data_ptr(), 6, CODES[x.dtype], ctypes.byref(o), None) == capi.VRS_ERROR_INVALID_ARGUMENT
    o.ndim, o.coords_layout = 1, 2
    assert lib.vrs_compact_host(x.data_ptr(), 6, CODES[x.dtype], ctypes.byref(o), None) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_compact_host(x.data_ptr(), 6, 10, None, None) == capi.VRS_ERROR_INVALID_ARGUMENT  # no such dtype
    o = capi.CompactHostOutputs()
    o.gather_values = o.gather_out = coords.data_ptr()
    o.value_bytes = 3
    assert lib.vrs_compact_host(x.data_ptr(), 6, CODES[x.dtype], ctypes.byref(o), None) == capi.VRS_ERROR_INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------- the scatter form on the host

@pytest.mark.parametrize("dtype", [torch.uint8, torch.bfloat16, torch.float32, torch.int64], ids=name_of)
def test_scatter_form(lib, dtype):
    mask = make_input(torch.bool, (5, 13), seed=5)
    inp = make_input(dtype, (5, 13), seed=6)
    R = int(mask.sum())
    source = make_input(dtype, (R + 9,), seed=7)
    before = source.clone()
    got = host_compact(lib, mask, scatter=(inp, source))
    assert got["count"] == R
    assert torch.equal(bits(source), bits(before))  # (the tail, like the rest of source, is untouched)
    # rank(i) is the exclusive count of set flags before i
    rank = (torch.cumsum(mask.reshape(-1).long(), 0) - mask.reshape(-1).long())
    want = torch.where(mask.reshape(-1), bits(source)[rank.clamp(max=R - 1)], bits(inp).reshape(-1))
    assert torch.equal(bits(got["scatter"]), want)
    assert torch.equal(got["scatter"].view(BITS[inp.element_size()]), bits(torch.masked_scatter(inp, mask, source)).reshape(-1))
    # exactly R elements is enough; one fewer is refused
    assert torch.equal(bits(host_compact(lib, mask, scatter=(inp, source[:R]))["scatter"]), want)
    host_compact(lib, mask, scatter=(inp, source[:R - 1]), expect=capi.VRS_ERROR_INVALID_ARGUMENT)


# ---------------------------------------------------------------------------------------------- refusals that need no device

def test_cpu_tensors_are_refused():
    x, m = torch.ones(4), torch.ones(4, dtype=torch.bool)
    for call in (lambda: vrs.nonzero(x), lambda: vrs.nonzero(x, as_tuple=True), lambda: vrs.argwhere(x), lambda: vrs.where(m),
                 lambda: vrs.count_nonzero(x), lambda: vrs.masked_select(x, m), lambda: vrs.masked_scatter(x, m, x)):
        with pytest.raises(vrs.VrsError) as e:
            call()
        assert e.value.code == capi.VRS_ERROR_INVALID_ARGUMENT and "GPU" in e.value.message


def test_complex_dtypes_are_refused():
    z, m = torch.ones(4, dtype=torch.complex64), torch.ones(4, dtype=torch.bool)
    for call in (lambda: vrs.nonzero(z), lambda: vrs.argwhere(z), lambda: vrs.where(z), lambda: vrs.count_nonzero(z),
                 lambda: vrs.masked_select(z, m), lambda: vrs.masked_scatter(z, m, z)):
        with pytest.raises(vrs.VrsError) as e:
            call()
        assert "complex" in e.value.message


@pytest.mark.parametrize("mask_dtype", [torch.uint8, torch.int64, torch.float32], ids=name_of)
def test_a_mask_that_is_not_bool_is_refused(mask_dtype):
    x, m = torch.ones(4), torch.ones(4, dtype=mask_dtype)
    with pytest.raises(RuntimeError, match="BoolTensor"):
        vrs.masked_select(x, m)
    with pytest.raises(RuntimeError, match="BoolTensor"):
        vrs.masked_scatter(x, m, x)


def test_shapes_that_do_not_broadcast_are_refused():
    x, m = torch.ones(3, 4), torch.ones(3, 5, dtype=torch.bool)
    with pytest.raises(RuntimeError):
        vrs.masked_select(x, m)
    with pytest.raises(RuntimeError):
        vrs.masked_scatter(x, m, torch.ones(20))
    with pytest.raises(RuntimeError):
        torch.masked_select(x, m)  # (torch refuses the same pair)
