"""The sorted-sequence search without a device: the tier decision (vrs_search_tier_for), the scratch sizes (vrs_search_scratch_bytes),
the argument checks of vrs_search_sorted and the torch-level refusals of searchsorted / bucketize."""
import ctypes

import pytest

from vkradixsort_amd import capi

LDS = capi.SEARCH_LDS_BYTES_DEFAULT
TMIN = capi.SEARCH_TABLE_MIN_QUERIES_DEFAULT
IMIN = capi.SEARCH_INDEX_MIN_QUERIES_DEFAULT
T_LDS, T_TABLE, T_DIRECT, T_INDEXED = capi.VRS_SEARCH_LDS, capi.VRS_SEARCH_TABLE, capi.VRS_SEARCH_DIRECT, capi.VRS_SEARCH_INDEXED
# dtype -> (element bytes, rank bytes)
WIDTHS = {capi.VRS_SORT_INT8: (1, 4), capi.VRS_SORT_UINT8: (1, 4), capi.VRS_SORT_INT16: (2, 4), capi.VRS_SORT_FLOAT16: (2, 4),
          capi.VRS_SORT_BFLOAT16: (2, 4), capi.VRS_SORT_INT32: (4, 4), capi.VRS_SORT_FLOAT32: (4, 4), capi.VRS_SORT_INT64: (8, 8),
          capi.VRS_SORT_FLOAT64: (8, 8)}


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def tier_for(lib, nb, m, nq, q_len, dtype, lds=LDS, tmin=TMIN, imin=IMIN):
    t = ctypes.c_int(-1)
    rc = lib.vrs_search_tier_for(nb, m, nq, q_len, dtype, lds, tmin, imin, ctypes.byref(t))
    return rc, t.value


def scratch(lib, nb, m, dtype, sorter, tier):
    out = ctypes.c_uint64(12345)
    return lib.vrs_search_scratch_bytes(nb, m, dtype, sorter, tier, ctypes.byref(out)), out.value


def test_new_symbols_are_bound_and_exported():
    for name in ("vrs_search_sorted", "vrs_search_tier_for", "vrs_search_scratch_bytes", "vrs_search_plan", "vrs_search_stats"):
        assert name in capi.EXPORTED_SYMBOLS
    import vkradixsort_amd as vrs
    assert callable(vrs.searchsorted) and callable(vrs.bucketize) and callable(vrs.search_stats)
    assert (capi.VRS_TUNE_SEARCH_LDS_BYTES, capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES, capi.VRS_TUNE_SEARCH_INDEX_MIN_QUERIES) == (29, 30, 31)
    assert capi.VRS_KERNEL_COUNT == 10


@pytest.mark.parametrize("dtype", [capi.VRS_SORT_INT32, capi.VRS_SORT_FLOAT32, capi.VRS_SORT_INT64, capi.VRS_SORT_FLOAT64])
def test_wide_dtypes_at_every_tier_boundary(lib, dtype):
    rb = WIDTHS[dtype][1]
    cap = LDS // rb
    for q, beyond in ((1, T_DIRECT), (IMIN - 1, T_DIRECT), (IMIN, T_INDEXED), (IMIN + 1, T_INDEXED), (10 ** 8, T_INDEXED)):
        for m, want in ((1, T_LDS), (2, T_LDS), (cap - 1, T_LDS), (cap, T_LDS), (cap + 1, beyond), (10 ** 8, beyond),
                        (2 ** 32 - 1, beyond)):
            assert tier_for(lib, m, m, q, q, dtype) == (0, want), (m, q)
    # no boundaries at all: the LDS tier whatever the queries; no table for wide dtypes
    assert tier_for(lib, 0, 0, 10 ** 8, 10 ** 8, dtype) == (0, T_LDS)
    assert tier_for(lib, 100, 100, 10 ** 8, 10 ** 8, dtype, tmin=1) == (0, T_LDS)


@pytest.mark.parametrize("dtype", [capi.VRS_SORT_INT8, capi.VRS_SORT_UINT8, capi.VRS_SORT_INT16, capi.VRS_SORT_FLOAT16, capi.VRS_SORT_BFLOAT16])
def test_narrow_dtypes_at_every_tier_boundary(lib, dtype):
    eb, rb = WIDTHS[dtype]
    cap = LDS // rb
    tmin = TMIN if eb == 2 else TMIN >> 8
    for m in (1, 1000, cap, cap + 1, 10 ** 8):
        below = T_LDS if m <= cap else T_DIRECT
        assert tier_for(lib, m, m, tmin - 1, tmin - 1, dtype) == (0, below), m
        assert tier_for(lib, m, m, tmin, tmin, dtype) == (0, T_TABLE), m
        assert tier_for(lib, m, m, 10 ** 8, 10 ** 8, dtype) == (0, T_TABLE), m
        # the table is switched off: the other tiers by size and queries
        assert tier_for(lib, m, m, 10 ** 8, 10 ** 8, dtype, tmin=0) == (0, T_LDS if m <= cap else T_INDEXED), m
    assert tier_for(lib, 0, 0, 10 ** 8, 10 ** 8, dtype) == (0, T_LDS)
    # a boundary row per query row: never the table; the queries that count are those of one row
    rows, m = 4, cap + 1
    assert tier_for(lib, rows * m, m, rows * 10 ** 6, 10 ** 6, dtype) == (0, T_INDEXED)
    assert tier_for(lib, rows * m, m, rows * 100, 100, dtype) == (0, T_DIRECT)
    assert tier_for(lib, rows * 100, 100, rows * 10 ** 6, 10 ** 6, dtype) == (0, T_LDS)


def test_tuning_thresholds(lib):
    f32, bf16, u8 = capi.VRS_SORT_FLOAT32, capi.VRS_SORT_BFLOAT16, capi.VRS_SORT_UINT8
    for lds in (0, 1024, 4096, 65536, 160 * 1024):
        cap = lds // 4
        assert tier_for(lib, cap, cap, 10, 10, f32, lds=lds)[1] == T_LDS
        assert tier_for(lib, cap + 1, cap + 1, 10, 10, f32, lds=lds)[1] == T_DIRECT
        assert tier_for(lib, cap // 2 + 1, cap // 2 + 1, 10, 10, capi.VRS_SORT_INT64, lds=lds)[1] == T_DIRECT
    # beyond what a workgroup can claim the setting is clamped
    assert tier_for(lib, 40960, 40960, 10, 10, f32, lds=1 << 20)[1] == T_LDS
    assert tier_for(lib, 40961, 40961, 10, 10, f32, lds=1 << 20)[1] == T_DIRECT
    for imin in (1, 1000, 1 << 20):
        assert tier_for(lib, 10 ** 6, 10 ** 6, imin, imin, f32, imin=imin)[1] == T_INDEXED
        if imin > 1:
            assert tier_for(lib, 10 ** 6, 10 ** 6, imin - 1, imin - 1, f32, imin=imin)[1] == T_DIRECT
    assert tier_for(lib, 10 ** 6, 10 ** 6, 10 ** 8, 10 ** 8, f32, imin=0)[1] == T_DIRECT
    for tmin in (1, 512, 1 << 20):
        assert tier_for(lib, 50, 50, tmin, tmin, bf16, tmin=tmin)[1] == T_TABLE
        assert tier_for(lib, 50, 50, max(tmin >> 8, 1), max(tmin >> 8, 1), u8, tmin=tmin)[1] == T_TABLE
        if tmin > 1:
            assert tier_for(lib, 50, 50, tmin - 1, tmin - 1, bf16, tmin=tmin)[1] == T_LDS
        if tmin >> 8 > 1:
            assert tier_for(lib, 50, 50, (tmin >> 8) - 1, (tmin >> 8) - 1, u8, tmin=tmin)[1] == T_LDS


def test_tier_for_refuses(lib):
    f32 = capi.VRS_SORT_FLOAT32
    for bad in (-1, 9, 100):
        assert tier_for(lib, 10, 10, 10, 10, bad)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
        assert b"dtype" in lib.vrs_last_error(None)
    assert tier_for(lib, 10, 3, 10, 10, f32)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
    assert b"num_boundaries" in lib.vrs_last_error(None)
    assert tier_for(lib, 10, 0, 10, 10, f32)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
    assert tier_for(lib, 10, 10, 10, 3, f32)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
    assert b"num_queries" in lib.vrs_last_error(None)
    assert tier_for(lib, 30, 10, 20, 10, f32)[0] == capi.VRS_ERROR_INVALID_ARGUMENT  # 3 boundary rows, 2 query rows
    assert b"rows" in lib.vrs_last_error(None)
    assert tier_for(lib, 30, 10, 30, 10, f32)[0] == capi.VRS_OK
    assert tier_for(lib, 10, 10, 30, 10, f32)[0] == capi.VRS_OK
    assert lib.vrs_search_tier_for(10, 10, 10, 10, f32, LDS, TMIN, IMIN, None) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert b"tier" in lib.vrs_last_error(None)


def bound(nb, dtype, sorter):
    eb, rb = WIDTHS[dtype]
    return (nb * eb // 128) * rb * 33 // 32 + (nb * rb if sorter else 0) + 1024


def test_scratch_bytes_monotone_and_bounded(lib):
    ms = [0, 1, 31, 32, 33, 1000, 16384, 16385, 10 ** 6, 10 ** 8, 2 ** 31, 2 ** 32 - 1]
    for dtype, (eb, rb) in WIDTHS.items():
        for sorter in (0, 1):
            prev = -1
            for m in ms:
                rc, b = scratch(lib, m, m, dtype, sorter, T_INDEXED)
                assert rc == capi.VRS_OK
                assert b <= bound(m, dtype, sorter), (m, dtype, sorter, b)
                assert b >= (m // (128 // eb)) * rb + (m * rb if sorter else 0), (m, dtype, sorter, b)  # the index (and the gathered ranks) fit
                assert b >= prev
                prev = b
            for tier in (T_LDS, T_DIRECT):
                assert scratch(lib, 10 ** 8, 10 ** 8, dtype, sorter, tier) == (capi.VRS_OK, 0)
            if eb <= 2:
                assert scratch(lib, 10 ** 8, 10 ** 8, dtype, sorter, T_TABLE) == (capi.VRS_OK, 4 << (8 * eb))
        # rows: three rows of m need what one row of 3 m needs, up to rounding
        one, three = scratch(lib, 3 * 10 ** 6, 3 * 10 ** 6, dtype, 1, T_INDEXED)[1], scratch(lib, 3 * 10 ** 6, 10 ** 6, dtype, 1, T_INDEXED)[1]
        assert abs(one - three) <= 1024


def test_scratch_bytes_refuses(lib):
    f32 = capi.VRS_SORT_FLOAT32
    assert scratch(lib, 10, 10, 99, 0, T_DIRECT)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
    assert b"dtype" in lib.vrs_last_error(None)
    assert scratch(lib, 10, 3, f32, 0, T_DIRECT)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
    assert b"num_boundaries" in lib.vrs_last_error(None)
    for tier in (-1, 4):
        assert scratch(lib, 10, 10, f32, 0, tier)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
        assert b"tier" in lib.vrs_last_error(None)
    assert scratch(lib, 10, 10, f32, 0, T_TABLE)[0] == capi.VRS_ERROR_INVALID_ARGUMENT
    assert b"table" in lib.vrs_last_error(None)
    assert lib.vrs_search_scratch_bytes(10, 10, f32, 0, T_DIRECT, None) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert b"bytes" in lib.vrs_last_error(None)


def call(lib, nb=10, m=10, nq=10, q_len=10, dtype=capi.VRS_SORT_FLOAT32, flags=0):
    return lib.vrs_search_sorted(None, None, nb, m, None, nq, q_len, dtype, flags, None, None, None)


def test_search_sorted_invalid_arguments(lib):
    bad = capi.VRS_ERROR_INVALID_ARGUMENT
    assert call(lib) == bad and b"NULL" in lib.vrs_last_error(None)
    for dtype in (-1, 9, 1000):
        assert call(lib, dtype=dtype) == bad and b"dtype" in lib.vrs_last_error(None)
    for flags in (4, 8, -1, 1 << 30):
        assert call(lib, flags=flags) == bad and b"flag" in lib.vrs_last_error(None)
    assert call(lib, nb=10, m=4) == bad and b"num_boundaries" in lib.vrs_last_error(None)
    assert call(lib, nq=10, q_len=4) == bad and b"num_queries" in lib.vrs_last_error(None)
    assert call(lib, nb=40, m=10, nq=20, q_len=10) == bad and b"rows" in lib.vrs_last_error(None)
    assert call(lib, nq=0, q_len=0) == bad  # (a NULL context is refused even when there is nothing to do)
    t, b = ctypes.c_int(), ctypes.c_uint64()
    assert lib.vrs_search_plan(None, 10, 10, 10, 10, capi.VRS_SORT_FLOAT32, 0, ctypes.byref(t), ctypes.byref(b)) == bad
    assert lib.vrs_search_stats(None, ctypes.byref(b), None, None, None) == bad


def test_torch_level_refusals_on_cpu_tensors():
    torch = pytest.importorskip("torch")
    import vkradixsort_amd as vrs

    seq, x = torch.arange(10, dtype=torch.float32), torch.rand(4, 5)
    refused = [
        lambda: vrs.searchsorted(seq, x),                                   # CPU tensors: no fallback
        lambda: vrs.bucketize(x, seq),
        lambda: vrs.searchsorted(seq, x, side="left", right=True),
        lambda: vrs.searchsorted(seq, x, side="middle"),
        lambda: vrs.searchsorted(torch.tensor(1.0), x),                     # a 0-d sequence
        lambda: vrs.searchsorted(torch.rand(3, 10), x),                     # leading dimensions differ
        lambda: vrs.searchsorted(torch.rand(4, 10), torch.rand(5)),         # dimensions differ
        lambda: vrs.searchsorted(torch.rand(4, 10), 0.5),                   # a number and an N-D sequence
        lambda: vrs.searchsorted(seq, x, sorter=torch.arange(10, dtype=torch.int32)),
        lambda: vrs.searchsorted(seq, x, sorter=torch.arange(9)),
        lambda: vrs.searchsorted(seq.bool(), x.bool()),                     # a dtype outside the nine
        lambda: vrs.searchsorted(seq, torch.zeros(3, dtype=torch.complex64)),  # promoted outside the nine
        lambda: vrs.searchsorted([1.0, 2.0], x),
        lambda: vrs.searchsorted(seq, "0.5"),
        lambda: vrs.bucketize(x, torch.rand(2, 5)),                         # boundaries must be 1-D
    ]
    for i, thunk in enumerate(refused):
        with pytest.raises(vrs.VrsError):
            thunk()
            pytest.fail(f"case {i} was not refused")
