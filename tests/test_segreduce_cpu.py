"""The segmented reduction without a device: the lane map of a chunk (vrs_segment_reduce_map_for), the levels of a segment
(vrs_segment_reduce_levels_for), the scratch bound, the argument checks of vrs_segment_reduce, the order as the library's host function
evaluates it (vrs_segment_reduce_host) against numpy, and the torch-level refusals of segment_reduce / index_add / index_reduce /
scatter_reduce."""
import ctypes
import math
import re

import numpy as np
import pytest

from vkradixsort_amd import capi

BAD = capi.VRS_ERROR_INVALID_ARGUMENT
I32, I64 = capi.VRS_SORT_INT32, capi.VRS_SORT_INT64
F16, BF16, F32, F64 = capi.VRS_SORT_FLOAT16, capi.VRS_SORT_BFLOAT16, capi.VRS_SORT_FLOAT32, capi.VRS_SORT_FLOAT64
SUM, PROD, MIN, MAX = capi.VRS_REDUCE_SUM, capi.VRS_REDUCE_PROD, capi.VRS_REDUCE_MIN, capi.VRS_REDUCE_MAX
LANE, ROWS, COLUMNS = capi.VRS_REDUCE_MAP_LANE, capi.VRS_REDUCE_MAP_ROWS, capi.VRS_REDUCE_MAP_COLUMNS
CH, LR = capi.REDUCE_CHUNK_ROWS_DEFAULT, capi.REDUCE_LANE_ROWS_DEFAULT
LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1023, 1025)
STORAGE = {I32: np.int32, I64: np.int64, F16: np.uint16, BF16: np.uint16, F32: np.float32, F64: np.float64}


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def bf16_bits(x32):
    """float32 values as bfloat16 bits, rounded to nearest even"""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def to_storage(x, dtype):
    """values as the bytes the library reads for `dtype`"""
    if dtype == F16:
        return np.ascontiguousarray(x, dtype=np.float64).astype(np.float16).view(np.uint16)
    if dtype == BF16:
        return bf16_bits(np.asarray(x, dtype=np.float32))
    return np.ascontiguousarray(x).astype(STORAGE[dtype])


def from_storage(raw, dtype):
    if dtype == F16:
        return raw.view(np.float16).astype(np.float64)
    if dtype == BF16:
        return (raw.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return raw


def host(lib, raw, dtype, offsets, op, init=None, order=None, ch=CH, lr=LR):
    n, C = raw.shape
    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    S = offsets.size - 1
    out = np.full((S, C), 0x5A, dtype=np.uint8).repeat(raw.itemsize, axis=1).view(raw.dtype).copy()
    order = np.ascontiguousarray(order, dtype=np.uint32) if order is not None else None
    rc = lib.vrs_segment_reduce_host(ptr(np.ascontiguousarray(raw)), n, C, dtype, ptr(order), ptr(offsets), S, op, ptr(init), ch, lr, ptr(out))
    assert rc == 0, lib.vrs_last_error(None)
    return out


def offsets_of(lengths):
    return np.concatenate(([0], np.cumsum(lengths))).astype(np.uint32)


def test_new_symbols_are_bound_and_exported():
    for name in ("vrs_segment_reduce", "vrs_segment_reduce_scratch_bytes", "vrs_segment_reduce_map_for", "vrs_segment_reduce_levels_for",
                 "vrs_segment_reduce_host", "vrs_segment_reduce_stats"):
        assert name in capi.EXPORTED_SYMBOLS
    import vkradixsort_amd as vrs
    assert all(callable(f) for f in (vrs.segment_reduce, vrs.index_add, vrs.index_reduce, vrs.scatter_reduce, vrs.reduce_stats))
    assert (capi.VRS_TUNE_REDUCE_CHUNK_ROWS, capi.VRS_TUNE_REDUCE_LANE_ROWS) == (35, 36) and (CH, LR) == (512, 16)
    assert (SUM, PROD, MIN, MAX) == (0, 1, 2, 3) and (LANE, ROWS, COLUMNS) == (0, 1, 2)
    from pathlib import Path
    include = Path(__file__).resolve().parent.parent / "include"
    header = (include / "vkradixsort_amd_tune.h").read_text()
    assert re.search(r"VRS_TUNE_REDUCE_CHUNK_ROWS\s*=\s*35\b", header) and re.search(r"VRS_TUNE_REDUCE_LANE_ROWS\s*=\s*36\b", header)
    assert "K13" in (include / "vkradixsort_amd_ops.h").read_text()


def map_for(lib, rows, C, lr=LR):
    m = ctypes.c_int(-1)
    return lib.vrs_segment_reduce_map_for(rows, C, lr, ctypes.byref(m)), m.value


def test_map_at_every_boundary(lib):
    for lr in (LR, 0, 1, 64):
        for rows, want in ((0, LANE), (1, LANE if lr >= 1 else ROWS), (lr, LANE), (lr + 1, ROWS)):
            assert map_for(lib, rows, 63, lr) == (0, want), (lr, rows)
            assert map_for(lib, rows, 1, lr) == (0, want)
            assert map_for(lib, rows, 64, lr) == (0, COLUMNS) and map_for(lib, rows, 2 ** 32 - 1, lr) == (0, COLUMNS)
    assert map_for(lib, 2 ** 32 - 1, 63) == (0, ROWS)
    assert map_for(lib, 1, 0)[0] == BAD and b"row_width" in lib.vrs_last_error(None)
    assert map_for(lib, 1, 1, 65)[0] == BAD and b"lane_rows" in lib.vrs_last_error(None)
    assert lib.vrs_segment_reduce_map_for(1, 1, LR, None) == BAD


def levels_for(lib, n, ch=CH):
    v = ctypes.c_uint32(99)
    return lib.vrs_segment_reduce_levels_for(n, ch, ctypes.byref(v)), v.value


def test_levels_at_every_boundary(lib):
    for ch in (64, 512, 4096):
        assert levels_for(lib, 0, ch) == (0, 1) and levels_for(lib, 1, ch) == (0, 1)
        assert levels_for(lib, ch, ch) == (0, 1) and levels_for(lib, ch + 1, ch) == (0, 2)
        assert levels_for(lib, ch * ch, ch) == (0, 2) and levels_for(lib, ch * ch + 1, ch) == (0, 3)
    assert levels_for(lib, 4097, 64) == (0, 3) and levels_for(lib, 262145) == (0, 3)
    assert levels_for(lib, 2 ** 32 - 1, 64) == (0, 6) and levels_for(lib, 2 ** 32 - 1, 4096) == (0, 3)
    for ch in (0, 63, 4097):
        assert levels_for(lib, 10, ch)[0] == BAD and b"chunk_rows" in lib.vrs_last_error(None)
    assert lib.vrs_segment_reduce_levels_for(10, CH, None) == BAD


def scratch(lib, n, C, S, dtype=F32, ch=CH):
    out = ctypes.c_uint64(12345)
    return lib.vrs_segment_reduce_scratch_bytes(n, C, S, dtype, ch, ctypes.byref(out)), out.value


def test_scratch_bound_is_monotone(lib):
    sizes = sorted({0, 1, 63, 64, 65, 511, 512, 513, 4096, 4097, 262144, 262145, 10 ** 6, 10 ** 8, 2 ** 31, 2 ** 32 - 1} |
                   {int(x) for x in np.random.default_rng(1).integers(0, 2 ** 32, 200)})
    for C, S, dtype in ((1, 1, F32), (1, 16385, F32), (64, 2 ** 20, F64), (129, 1000, F16), (3, 2 ** 32 - 1, I64)):
        for ch in (64, 512, 4096):
            got = [scratch(lib, n, C, S, dtype, ch) for n in sizes]
            assert all(rc == 0 for rc, _ in got)
            assert all(a[1] <= b[1] for a, b in zip(got, got[1:])), (C, S, ch)
        for n in (0, 1000, 10 ** 8):  # ... and a longer chunk never needs more
            by_chunk = [scratch(lib, n, C, S, dtype, ch)[1] for ch in (64, 128, 512, 1000, 4096)]
            assert all(a >= b for a, b in zip(by_chunk, by_chunk[1:]))
    # the items of level 0 (16 bytes for each of n / CH + S + 1) and the segments' list are in it
    assert scratch(lib, 10 ** 8, 1, 16385)[1] >= 16 * (10 ** 8 // 512 + 16385) + 4 * 16385
    assert scratch(lib, 10 ** 8, 1, 16385)[1] < 10 ** 7
    for dtype in (capi.VRS_SORT_INT8, capi.VRS_SORT_UINT8, capi.VRS_SORT_INT16, -1, 9):
        assert scratch(lib, 10, 1, 1, dtype)[0] == BAD and b"dtype" in lib.vrs_last_error(None)
    assert scratch(lib, 10, 0, 1)[0] == BAD and b"row_width" in lib.vrs_last_error(None)
    assert scratch(lib, 10, 1, 1, F32, 63)[0] == BAD and b"chunk_rows" in lib.vrs_last_error(None)
    assert lib.vrs_segment_reduce_scratch_bytes(10, 1, 1, F32, CH, None) == BAD


def test_segment_reduce_refuses_before_any_device_work(lib):
    def call(dtype=F32, op=SUM, C=1, S=1):
        return lib.vrs_segment_reduce(None, None, 10, C, dtype, None, None, S, op, None, None, None)
    assert call() == BAD and b"NULL" in lib.vrs_last_error(None)
    assert call(S=0) == BAD and b"NULL" in lib.vrs_last_error(None)
    for dtype in (capi.VRS_SORT_INT8, capi.VRS_SORT_UINT8, capi.VRS_SORT_INT16, -1, 9):
        assert call(dtype=dtype) == BAD and b"dtype" in lib.vrs_last_error(None)
    for op in (-1, 4, 100):
        assert call(op=op) == BAD and b"unknown op" in lib.vrs_last_error(None)
    assert call(C=0) == BAD and b"row_width" in lib.vrs_last_error(None)
    c = ctypes.c_uint64()
    assert lib.vrs_segment_reduce_stats(None, ctypes.byref(c), None, None, None) == BAD
    x, o = np.zeros((4, 1), dtype=np.float32), np.zeros(2, dtype=np.uint32)
    assert lib.vrs_segment_reduce_host(ptr(x), 4, 1, capi.VRS_SORT_INT16, None, ptr(o), 1, SUM, None, CH, LR, ptr(x)) == BAD
    assert lib.vrs_segment_reduce_host(ptr(x), 4, 1, F32, None, ptr(o), 1, 7, None, CH, LR, ptr(x)) == BAD
    assert lib.vrs_segment_reduce_host(ptr(x), 4, 0, F32, None, ptr(o), 1, SUM, None, CH, LR, ptr(x)) == BAD
    assert lib.vrs_segment_reduce_host(ptr(x), 4, 1, F32, None, ptr(o), 1, SUM, None, 32, LR, ptr(x)) == BAD
    assert lib.vrs_segment_reduce_host(ptr(x), 4, 1, F32, None, ptr(o), 1, SUM, None, CH, 65, ptr(x)) == BAD
    assert lib.vrs_segment_reduce_host(None, 4, 1, F32, None, ptr(o), 1, SUM, None, CH, LR, ptr(x)) == BAD and b"NULL" in lib.vrs_last_error(None)
    assert lib.vrs_segment_reduce_host(None, 0, 1, F32, None, None, 0, SUM, None, CH, LR, None) == 0


# ---------------------------------------------------------------------------------------------- the order on the host

NUMPY_OPS = {SUM: np.add, PROD: np.multiply, MIN: np.minimum, MAX: np.maximum}


def numpy_reduce(x, offsets, op, identity):
    out = np.empty((offsets.size - 1, x.shape[1]), dtype=x.dtype)
    with np.errstate(over="ignore"):
        for s in range(offsets.size - 1):
            rows = x[offsets[s]:offsets[s + 1]]
            out[s] = NUMPY_OPS[op].reduce(rows, axis=0) if rows.shape[0] else identity
    return out


@pytest.mark.parametrize("dtype", [I32, I64])
@pytest.mark.parametrize("C", [1, 3, 64, 65])
def test_integers_equal_numpy_wrapped(lib, dtype, C):
    rng = np.random.default_rng(10 * dtype + C)
    T = STORAGE[dtype]
    info = np.iinfo(T)
    lengths = rng.permutation(LENGTHS)
    offsets = offsets_of(lengths)
    x = rng.integers(info.min, info.max, (int(offsets[-1]), C), dtype=T, endpoint=True)
    small = rng.integers(-3, 4, x.shape).astype(T)  # (products that do not collapse to zero at once)
    for op, values, identity in ((SUM, x, 0), (PROD, small | 1, 1), (PROD, x, 1), (MIN, x, info.max), (MAX, x, info.min)):
        want = numpy_reduce(values, offsets, op, identity)
        for ch, lr in ((CH, LR), (64, 0), (64, 64)):
            assert np.array_equal(host(lib, values, dtype, offsets, op, ch=ch, lr=lr), want), (op, ch, lr)
    init = rng.integers(info.min, info.max, (lengths.size, C), dtype=T, endpoint=True)
    with np.errstate(over="ignore"):
        assert np.array_equal(host(lib, x, dtype, offsets, SUM, init=init), init + numpy_reduce(x, offsets, SUM, 0))
    order = rng.permutation(x.shape[0])
    assert np.array_equal(host(lib, x, dtype, offsets, SUM, order=order), numpy_reduce(x[order], offsets, SUM, 0))


@pytest.mark.parametrize("dtype", [F16, BF16, F32, F64])
@pytest.mark.parametrize("C", [1, 5, 64])
def test_float_sums_of_small_integers_are_exact(lib, dtype, C):
    """values in [-8, 8] and L <= 2^16: every partial sum is an integer below 2^20, exact in float32 whatever the order"""
    rng = np.random.default_rng(20 * dtype + C)
    lengths = list(rng.permutation(LENGTHS)) + ([2 ** 16, 4097] if C == 1 else [4097])
    offsets = offsets_of(lengths)
    x = rng.integers(-8, 9, (int(offsets[-1]), C)).astype(np.float64)
    exact = numpy_reduce(x, offsets, SUM, 0.0)
    want = to_storage(exact, dtype)  # (rounded once, to nearest even: 16-bit results beyond 2^11 / 2^8 are not integers of the type)
    for ch, lr in ((CH, LR), (64, 16), (4096, 64)):
        got = host(lib, to_storage(x, dtype), dtype, offsets, SUM, ch=ch, lr=lr)
        assert np.array_equal(got, want), (ch, lr)
    init = rng.integers(-8, 9, (len(lengths), C)).astype(np.float64)
    got = host(lib, to_storage(x, dtype), dtype, offsets, SUM, init=to_storage(init, dtype))
    assert np.array_equal(got, to_storage(exact + init, dtype))


@pytest.mark.parametrize("dtype,eps", [(F32, 2.0 ** -23), (F64, 2.0 ** -52)])
@pytest.mark.parametrize("C", [1, 7, 64])
def test_random_float_sums_are_within_the_bound_of_any_order(lib, dtype, eps, C):
    rng = np.random.default_rng(30 * dtype + C)
    lengths = list(LENGTHS) + [4097] + ([70000] if C == 1 else [])
    offsets = offsets_of(lengths)
    x = (rng.standard_normal((int(offsets[-1]), C)) * np.exp(rng.uniform(-3, 3, (int(offsets[-1]), C)))).astype(STORAGE[dtype])
    for ch, lr in ((CH, LR), (64, 0)):
        got = host(lib, x, dtype, offsets, SUM, ch=ch, lr=lr)
        for s, L in enumerate(lengths):
            rows = x[offsets[s]:offsets[s + 1]].astype(np.float64)
            for col in range(C):
                exact = math.fsum(rows[:, col])  # (the correctly rounded sum of the float64 values: the exact one to 2^-53)
                bound = (L + 1) * eps * float(np.abs(rows[:, col]).sum())
                assert abs(float(got[s, col]) - exact) <= bound, (s, L, col)


@pytest.mark.parametrize("dtype", [F16, F32, F64])
@pytest.mark.parametrize("C", [1, 3, 63, 64])
def test_a_segment_does_not_depend_on_where_it_sits(lib, dtype, C):
    rng = np.random.default_rng(40 * dtype + C)
    for L in (17, 513, 4097):
        seg = to_storage(rng.standard_normal((L, C)), dtype)
        alone = host(lib, seg, dtype, [0, L], SUM, ch=64)
        for before, after in ((1, 0), (63, 700), (1000, 1)):
            x = np.concatenate((to_storage(rng.standard_normal((before, C)) * 1e3, dtype), seg, to_storage(rng.standard_normal((after, C)) * 1e3, dtype)))
            got = host(lib, x, dtype, [0, before, before + L, before + L + after], SUM, ch=64)
            assert np.array_equal(got[1], alone[0]), (L, before, after)
        order = np.concatenate((np.arange(L) + 5, np.arange(5)))  # ... nor on where its rows come from
        moved = np.concatenate((seg[:5] * 0, seg))
        assert np.array_equal(host(lib, moved, dtype, [0, L], SUM, order=order, ch=64), alone)


@pytest.mark.parametrize("dtype", [F16, BF16, F32, F64])
def test_nan_and_empty_segments_for_every_op(lib, dtype):
    inf, nan = np.inf, np.nan
    lengths = [0, 3, 0, 600, 40]
    offsets = offsets_of(lengths)
    for C in (2, 64):
        x = np.ones((643, C))
        x[1, 0] = nan        # segment 1, column 0
        x[3 + 555, 1] = nan  # segment 3, column 1 (second chunk of two)
        x[620, 0] = -2.0
        raw = to_storage(x, dtype)
        for op, identity in ((SUM, 0.0), (PROD, 1.0), (MIN, inf), (MAX, -inf)):
            got = from_storage(host(lib, raw, dtype, offsets, op), dtype)
            assert (got[0] == identity).all() and (got[2] == identity).all()                   # empty segments: the identity
            assert np.isnan(got[1, 0]) and np.isnan(got[3, 1])                                  # NaN reaches the answer in every op
            assert not np.isnan(got[1, 1]) and not np.isnan(got[3, 0]) and not np.isnan(got[4]).any()
            assert got[4, 0] == {SUM: 37.0, PROD: -2.0, MIN: -2.0, MAX: 1.0}[op]
            init = to_storage(np.full((5, C), 5.0), dtype)
            init[2] = to_storage(np.full(C, -0.0), dtype)
            with_init = host(lib, raw, dtype, offsets, op, init=init)
            assert np.array_equal(with_init[0], init[0]) and np.array_equal(with_init[2], init[2])  # empty: init's own bits, -0.0 included
            assert np.isnan(from_storage(with_init, dtype)[1, 0])
            assert from_storage(with_init, dtype)[4, 0] == {SUM: 42.0, PROD: -10.0, MIN: -2.0, MAX: 5.0}[op]
    # the sign of a zero sum: +0.0, whatever went in
    zeros = to_storage(np.full((20, 1), -0.0), dtype)
    for L in (1, 16, 17, 20):
        assert host(lib, zeros, dtype, [0, L], SUM).view(np.uint8).any() == False  # noqa: E712
    for dt, T in ((I32, np.int32), (I64, np.int64)):
        e = host(lib, np.zeros((0, 1), dtype=T), dt, [0, 0], SUM)
        assert e[0, 0] == 0 and host(lib, np.zeros((0, 1), dtype=T), dt, [0, 0], PROD)[0, 0] == 1
        assert host(lib, np.zeros((0, 1), dtype=T), dt, [0, 0], MIN)[0, 0] == np.iinfo(T).max
        assert host(lib, np.zeros((0, 1), dtype=T), dt, [0, 0], MAX)[0, 0] == np.iinfo(T).min


def test_offsets_are_clamped_like_the_segmented_sorts(lib):
    x = np.arange(10, dtype=np.int32).reshape(10, 1)
    got = host(lib, x, I32, [2, 5, 3, 100, 2 ** 32 - 1], SUM)  # [2, 5) | [5, 5) | [3, 10) | [10, 10)
    assert got[:, 0].tolist() == [9, 0, 42, 0]
    t, cb, ce = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.vrs_segment_tier_for(5, 3, 10, 0, 0, ctypes.byref(t), ctypes.byref(cb), ctypes.byref(ce)) == 0 and (cb.value, ce.value) == (5, 5)


# ---------------------------------------------------------------------------------------------- the wrappers

def test_torch_level_refusals_on_cpu_tensors():
    torch = pytest.importorskip("torch")
    import vkradixsort_amd as vrs

    x, idx, lens = torch.rand(10, 3), torch.arange(10) % 4, torch.tensor([4, 6])
    base = torch.zeros(4, 3)
    refused = [
        (lambda: vrs.segment_reduce(x, "sum", lengths=lens), "segment_reduce takes tensors on a GPU"),  # CPU tensors: no fallback
        (lambda: vrs.index_add(base, 0, idx, x), "index_add takes tensors on a GPU"),
        (lambda: vrs.index_reduce(base, 0, idx, x, "amax"), "index_reduce takes tensors on a GPU"),
        (lambda: vrs.scatter_reduce(base[:, 0], 0, idx, x[:, 0], "sum"), "scatter_reduce takes tensors on a GPU"),
        (lambda: vrs.segment_reduce(x, "median", lengths=lens), "sum, mean, max, min or prod"),
        (lambda: vrs.segment_reduce(x, "sum"), "either lengths or offsets"),
        (lambda: vrs.segment_reduce(x, "sum", lengths=lens, offsets=lens), "either lengths or offsets"),
        (lambda: vrs.segment_reduce(x, "sum", lengths=lens.view(1, 2)), "1-D int32 or int64"),
        (lambda: vrs.segment_reduce(x, "sum", lengths=lens.float()), "1-D int32 or int64"),
        (lambda: vrs.segment_reduce(x, "sum", lengths=lens, axis=1), "axis 0 only"),
        (lambda: vrs.segment_reduce(x.to(torch.int8), "sum", lengths=lens), "not torch.int8"),
        (lambda: vrs.segment_reduce([1.0], "sum", lengths=lens), "segment_reduce takes a tensor"),
        (lambda: vrs.index_add(base, 0, idx.float(), x), "1-D int32 or int64 index"),
        (lambda: vrs.index_add(base, 0, idx, x.double()), "source must have the input's dtype"),
        (lambda: vrs.index_add(base, 0, idx[:9], x), "index.numel() entries along dim"),
        (lambda: vrs.index_add(base, 0, idx, x[:, :2]), "index.numel() entries along dim"),
        (lambda: vrs.index_add(base.bool(), 0, idx, x.bool()), "not torch.bool"),
        (lambda: vrs.index_reduce(base, 0, idx, x, "sum"), "prod, mean, amax or amin"),
        (lambda: vrs.scatter_reduce(base[:, 0], 0, idx, x[:, 0], "max"), "sum, prod, mean, amax or amin"),
        (lambda: vrs.scatter_reduce(base[:, 0], 0, idx, x[:5, 0], "sum"), "index may not be longer than src"),
    ]
    for i, (thunk, message) in enumerate(refused):
        with pytest.raises(vrs.VrsError, match=re.escape(message)) as e:
            thunk()
        assert e.value.code == BAD, i
    with pytest.raises(NotImplementedError):
        vrs.scatter_reduce(base, 0, idx.view(10, 1).expand(10, 3), x, "sum")
    with pytest.raises(IndexError):
        vrs.index_add(base, 2, idx, x)
