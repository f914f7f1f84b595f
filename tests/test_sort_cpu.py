"""The torch.sort drop-in without a device: the 64-bit segmented sorts' classification (vrs_segment_tier_for_u64), the argument checks of
the new entry points, the rank widths and the package exports."""
import ctypes

import pytest

from vkradixsort_amd import capi


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def tier_for_u64(lib, b, e, n, pairs, min_keys=capi.SEGMENT_ONE_CALL_MIN_KEYS_DEFAULT):
    t, cb, ce = ctypes.c_int(-1), ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.vrs_segment_tier_for_u64(b, e, n, pairs, min_keys, ctypes.byref(t), ctypes.byref(cb), ctypes.byref(ce)) == capi.VRS_OK
    return t.value, cb.value, ce.value


def expected_tier_u64(length, pairs, min_keys):
    block = capi.SEGMENT_BLOCK_MAX_PAIRS_U64 if pairs else capi.SEGMENT_BLOCK_MAX_KEYS_U64
    if length <= capi.SEGMENT_WAVE_MAX_U64:
        return capi.VRS_SEGMENT_WAVE
    if length <= block:
        return capi.VRS_SEGMENT_BLOCK
    if min_keys and length >= min_keys:
        return capi.VRS_SEGMENT_ONE_CALL
    return capi.VRS_SEGMENT_GLOBAL


def test_u64_capacities():
    assert (capi.SEGMENT_WAVE_MAX_U64, capi.SEGMENT_BLOCK_MAX_KEYS_U64, capi.SEGMENT_BLOCK_MAX_PAIRS_U64) == (896, 13312, 6656)


@pytest.mark.parametrize("pairs", [0, 1])
def test_u64_every_tier_boundary(lib, pairs):
    block = capi.SEGMENT_BLOCK_MAX_PAIRS_U64 if pairs else capi.SEGMENT_BLOCK_MAX_KEYS_U64
    thr = capi.SEGMENT_ONE_CALL_MIN_KEYS_DEFAULT
    n = 1 << 24
    cases = {0: capi.VRS_SEGMENT_WAVE, 1: capi.VRS_SEGMENT_WAVE, 2: capi.VRS_SEGMENT_WAVE,
             895: capi.VRS_SEGMENT_WAVE, 896: capi.VRS_SEGMENT_WAVE, 897: capi.VRS_SEGMENT_BLOCK,
             block - 1: capi.VRS_SEGMENT_BLOCK, block: capi.VRS_SEGMENT_BLOCK, block + 1: capi.VRS_SEGMENT_GLOBAL,
             thr - 1: capi.VRS_SEGMENT_GLOBAL, thr: capi.VRS_SEGMENT_ONE_CALL, thr + 1: capi.VRS_SEGMENT_ONE_CALL}
    for length, tier in cases.items():
        for b in (0, 3, 12345):
            assert tier_for_u64(lib, b, b + length, n, pairs) == (tier, b, b + length), (length, b)
    # 64-bit keys and pairs differ between the two block capacities only
    assert tier_for_u64(lib, 0, 13312, n, 0)[0] == capi.VRS_SEGMENT_BLOCK
    assert tier_for_u64(lib, 0, 13312, n, 1)[0] == capi.VRS_SEGMENT_GLOBAL


def test_u64_threshold_setting(lib):
    n = 1 << 24
    assert tier_for_u64(lib, 0, 1 << 22, n, 0, 0)[0] == capi.VRS_SEGMENT_GLOBAL  # 0: never the one-call tier
    assert tier_for_u64(lib, 0, 20000, n, 0, 20000)[0] == capi.VRS_SEGMENT_ONE_CALL
    assert tier_for_u64(lib, 0, 19999, n, 0, 20000)[0] == capi.VRS_SEGMENT_GLOBAL
    assert tier_for_u64(lib, 0, 5000, n, 0, 1000)[0] == capi.VRS_SEGMENT_BLOCK  # the LDS tiers come first
    for length in (0, 1, 2, 256, 257, 895, 896, 897, 1789, 1790, 4096, 4097, 6656, 6657, 13312, 13313, 99999, 1 << 20, (1 << 20) + 1):
        for pairs in (0, 1):
            for min_keys in (0, 50000, 1 << 20):
                assert tier_for_u64(lib, 7, 7 + length, n, pairs, min_keys)[0] == expected_tier_u64(length, pairs, min_keys)


def test_u64_malformed_ranges_clamp(lib):
    n = 10000
    assert tier_for_u64(lib, 500, 100, n, 0)[1:] == (500, 500)
    assert tier_for_u64(lib, 9000, 20000, n, 0)[1:] == (9000, n)
    assert tier_for_u64(lib, 20000, 30000, n, 0)[1:] == (n, n)
    assert tier_for_u64(lib, 0xFFFFFFFF, 0xFFFFFFFF, n, 1)[1:] == (n, n)
    assert tier_for_u64(lib, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0) == (capi.VRS_SEGMENT_GLOBAL, 0, 0xFFFFFFFF)


def test_u32_classification_unchanged(lib):
    t, cb, ce = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32()
    for length, pairs, tier in ((1789, 0, capi.VRS_SEGMENT_WAVE), (1790, 0, capi.VRS_SEGMENT_BLOCK), (14333, 0, capi.VRS_SEGMENT_BLOCK),
                                (13313, 1, capi.VRS_SEGMENT_GLOBAL), (897, 1, capi.VRS_SEGMENT_WAVE)):
        assert lib.vrs_segment_tier_for(0, length, 1 << 24, pairs, 1 << 20, ctypes.byref(t), ctypes.byref(cb), ctypes.byref(ce)) == 0
        assert t.value == tier, (length, pairs)


def test_tier_for_u64_rejects_null_outputs(lib):
    t, c = ctypes.c_int(), ctypes.c_uint32()
    assert lib.vrs_segment_tier_for_u64(0, 10, 10, 0, 0, None, ctypes.byref(c), ctypes.byref(c)) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_segment_tier_for_u64(0, 10, 10, 0, 0, ctypes.byref(t), None, ctypes.byref(c)) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_segment_tier_for_u64(0, 10, 10, 0, 0, ctypes.byref(t), ctypes.byref(c), None) == capi.VRS_ERROR_INVALID_ARGUMENT


def test_entry_points_reject_null_arguments(lib):
    assert lib.vrs_sort_segments_u64(None, None, None, 16, None, 1) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_sort_segments_u64(None, None, None, 0, None, 0) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_sort_segments_pairs_u64(None, None, None, None, None, 16, None, 1) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_sort_rank_keys(None, None, 16, 4, capi.VRS_SORT_INT32, 0, None, None) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_sort_restore(None, None, None, None, 16, 4, capi.VRS_SORT_INT32, 0, None, None) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert b"NULL" in lib.vrs_last_error(None)


def test_rank_bytes_and_unknown_dtypes(lib):
    rb = ctypes.c_int()
    widths = {capi.VRS_SORT_INT8: 4, capi.VRS_SORT_UINT8: 4, capi.VRS_SORT_INT16: 4, capi.VRS_SORT_INT32: 4, capi.VRS_SORT_INT64: 8,
              capi.VRS_SORT_FLOAT16: 4, capi.VRS_SORT_BFLOAT16: 4, capi.VRS_SORT_FLOAT32: 4, capi.VRS_SORT_FLOAT64: 8}
    for dtype, w in widths.items():
        assert lib.vrs_sort_rank_bytes(dtype, ctypes.byref(rb)) == capi.VRS_OK and rb.value == w
    for bad in (-1, 9, 100):
        assert lib.vrs_sort_rank_bytes(bad, ctypes.byref(rb)) == capi.VRS_ERROR_INVALID_ARGUMENT
        assert b"dtype" in lib.vrs_last_error(None)
    assert lib.vrs_sort_rank_bytes(capi.VRS_SORT_INT32, None) == capi.VRS_ERROR_INVALID_ARGUMENT


def test_pins_unchanged():
    assert capi.VRS_KERNEL_COUNT == 10
    assert capi.VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS == 27 and capi.VRS_TUNE_TOPK_GRID_MIN_KEYS == 28
    assert capi.VRS_SORT_DESCENDING == 1 and capi.VRS_SORT_FLOAT64 == 8


def test_new_symbols_are_bound():
    for name in ("vrs_sort_segments_u64", "vrs_sort_segments_pairs_u64", "vrs_segment_tier_for_u64", "vrs_sort_rank_keys",
                 "vrs_sort_restore", "vrs_sort_rank_bytes"):
        assert name in capi.EXPORTED_SYMBOLS


def test_package_exports():
    import vkradixsort_amd as vrs
    assert callable(vrs.sort) and callable(vrs.argsort) and callable(vrs.sort_values)


def test_python_rejects_cpu_tensors_and_unsupported_dtypes():
    torch = pytest.importorskip("torch")
    import vkradixsort_amd as vrs
    with pytest.raises(vrs.VrsError):
        vrs.sort(torch.arange(10, dtype=torch.int32))  # a CPU tensor: no fallback
    with pytest.raises(vrs.VrsError):
        vrs.argsort(torch.ones(4, dtype=torch.float32))
    import importlib
    sort_mod = importlib.import_module("vkradixsort_amd.sort")  # (the package's `sort` is the function)
    for dt in (torch.bool, torch.complex64):
        with pytest.raises(vrs.VrsError):
            sort_mod._dtype_code(torch, dt)
    for name in ("uint16", "uint32", "uint64"):
        if hasattr(torch, name):
            with pytest.raises(vrs.VrsError):
                sort_mod._dtype_code(torch, getattr(torch, name))
