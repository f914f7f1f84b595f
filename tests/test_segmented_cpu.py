"""The segmented sorts' classification (vrs_segment_tier_for, the function the kernels use too) and argument checks: no device."""
import ctypes

import pytest

from vkradixsort_amd import capi


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def tier_for(lib, b, e, n, pairs, min_keys=capi.SEGMENT_ONE_CALL_MIN_KEYS_DEFAULT):
    t, cb, ce = ctypes.c_int(-1), ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.vrs_segment_tier_for(b, e, n, pairs, min_keys, ctypes.byref(t), ctypes.byref(cb), ctypes.byref(ce)) == capi.VRS_OK
    return t.value, cb.value, ce.value


def expected_tier(length, pairs, min_keys):
    block = capi.SEGMENT_BLOCK_MAX_PAIRS if pairs else capi.SEGMENT_BLOCK_MAX_KEYS
    if length <= capi.SEGMENT_WAVE_MAX:
        return capi.VRS_SEGMENT_WAVE
    if length <= block:
        return capi.VRS_SEGMENT_BLOCK
    if min_keys and length >= min_keys:
        return capi.VRS_SEGMENT_ONE_CALL
    return capi.VRS_SEGMENT_GLOBAL


@pytest.mark.parametrize("pairs", [0, 1])
def test_every_tier_boundary(lib, pairs):
    block = capi.SEGMENT_BLOCK_MAX_PAIRS if pairs else capi.SEGMENT_BLOCK_MAX_KEYS
    thr = capi.SEGMENT_ONE_CALL_MIN_KEYS_DEFAULT
    n = 1 << 24
    cases = {0: capi.VRS_SEGMENT_WAVE, 1: capi.VRS_SEGMENT_WAVE, 2: capi.VRS_SEGMENT_WAVE,
             1789: capi.VRS_SEGMENT_WAVE, 1790: capi.VRS_SEGMENT_BLOCK,
             block: capi.VRS_SEGMENT_BLOCK, block + 1: capi.VRS_SEGMENT_GLOBAL,
             thr - 1: capi.VRS_SEGMENT_GLOBAL, thr: capi.VRS_SEGMENT_ONE_CALL, thr + 1: capi.VRS_SEGMENT_ONE_CALL}
    for length, tier in cases.items():
        for b in (0, 3, 12345):
            assert tier_for(lib, b, b + length, n, pairs) == (tier, b, b + length), (length, b)
    # keys and pairs differ between the two block capacities only
    assert tier_for(lib, 0, 14333, n, 0)[0] == capi.VRS_SEGMENT_BLOCK
    assert tier_for(lib, 0, 14333, n, 1)[0] == capi.VRS_SEGMENT_GLOBAL


def test_threshold_setting(lib):
    n = 1 << 24
    assert tier_for(lib, 0, 1 << 22, n, 0, 0)[0] == capi.VRS_SEGMENT_GLOBAL  # 0: never the one-call tier
    assert tier_for(lib, 0, 20000, n, 0, 20000)[0] == capi.VRS_SEGMENT_ONE_CALL
    assert tier_for(lib, 0, 19999, n, 0, 20000)[0] == capi.VRS_SEGMENT_GLOBAL
    assert tier_for(lib, 0, 5000, n, 0, 1000)[0] == capi.VRS_SEGMENT_BLOCK  # the LDS tiers come first
    for length in (0, 1, 2, 256, 257, 1789, 1790, 4096, 4097, 13312, 13313, 14333, 14334, 99999, 1 << 20, (1 << 20) + 1):
        for pairs in (0, 1):
            for min_keys in (0, 50000, 1 << 20):
                assert tier_for(lib, 7, 7 + length, n, pairs, min_keys)[0] == expected_tier(length, pairs, min_keys)


def test_malformed_ranges_clamp(lib):
    n = 10000
    assert tier_for(lib, 500, 100, n, 0)[1:] == (500, 500)      # e < b: empty at b
    assert tier_for(lib, 9000, 20000, n, 0)[1:] == (9000, n)    # e > n: cut at n
    assert tier_for(lib, 20000, 30000, n, 0)[1:] == (n, n)      # b > n: empty at n
    assert tier_for(lib, 20000, 5, n, 0)[1:] == (n, n)
    assert tier_for(lib, 0xFFFFFFFF, 0xFFFFFFFF, n, 1)[1:] == (n, n)
    assert tier_for(lib, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0) == (capi.VRS_SEGMENT_GLOBAL, 0, 0xFFFFFFFF)
    assert tier_for(lib, 9000, 20000, n, 0)[0] == capi.VRS_SEGMENT_WAVE  # the tier of the clamped length


def test_tier_for_rejects_null_outputs(lib):
    t, c = ctypes.c_int(), ctypes.c_uint32()
    assert lib.vrs_segment_tier_for(0, 10, 10, 0, 0, None, ctypes.byref(c), ctypes.byref(c)) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_segment_tier_for(0, 10, 10, 0, 0, ctypes.byref(t), None, ctypes.byref(c)) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_segment_tier_for(0, 10, 10, 0, 0, ctypes.byref(t), ctypes.byref(c), None) == capi.VRS_ERROR_INVALID_ARGUMENT


def test_entry_points_reject_null_arguments(lib):
    u = ctypes.c_uint64()
    assert lib.vrs_sort_segments_u32(None, None, None, 16, None, 1) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_sort_segments_u32(None, None, None, 0, None, 0) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_sort_segments_pairs_u32(None, None, None, None, None, 16, None, 1) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert lib.vrs_segmented_stats(None, ctypes.byref(u), None, None, None) == capi.VRS_ERROR_INVALID_ARGUMENT
    assert b"NULL" in lib.vrs_last_error(None)


def test_tuning_key_is_new_and_kernel_ids_unchanged():
    assert capi.VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS == 27
    assert capi.VRS_KERNEL_COUNT == 10


def test_package_exports():
    import vkradixsort_amd as vrs
    assert callable(vrs.sort_segments) and callable(vrs.sort_rows) and callable(vrs.segmented_stats)
