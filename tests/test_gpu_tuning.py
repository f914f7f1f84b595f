"""vrs_set_tuning on a device, on a context of its own with its own stream: every key takes its default, every key with a bound refuses a
value outside it with the message it always gave, keys outside the enum are unknown; and the sorts that read the settings afterwards
(the one-call sort above the single-launch size, a segmented sort) still sort.  The two keys that run the placement probe again and
VRS_TUNE_DEBUG_POOL_NO_MEMORY are left out: they act on the context, not on a setting."""
import numpy as np
import pytest

import vkradixsort_amd as vrs
from vkradixsort_amd import capi

pytestmark = pytest.mark.gpu

# key: (default, a value outside the accepted range or None, the refusal) -- literals of this test, as include/vkradixsort_amd_tune.h
# documents the keys and as vrs_set_tuning answered before the settings had one table
KEYS = {
    capi.VRS_TUNE_XCD_REMAP: (1, None, None),
    capi.VRS_TUNE_SCATTER_VARIANT: (0, None, None),
    capi.VRS_TUNE_FUSED_PREFIX: (1, None, None),
    capi.VRS_TUNE_RANK_MODE: (0, 3, "rank mode must be 0 (auto), 1 (ballot) or 2 (atomic)"),
    capi.VRS_TUNE_ONE_CALL_MIN_KEYS: (1 << 13, -1, "one-call threshold must be >= 0"),
    capi.VRS_TUNE_DEBUG_MISPLACE_STREAMS: (0, None, None),
    capi.VRS_TUNE_LOOKBACK_SPIN_BUDGET: (4096, -1, "spin budget must be >= 0"),
    capi.VRS_TUNE_DEBUG_HOLD_TILE: (-1, None, None),
    capi.VRS_TUNE_DIGIT_TABLE_GROUPS: (0, 24, "digit table groups must be 0 (by size), 8, 16 or 32"),
    capi.VRS_TUNE_SINGLE_MAX_KEYS: (4096, -1, "single-launch threshold must be >= 0"),
    capi.VRS_TUNE_FUSED_PLAN: (0, None, None),
    capi.VRS_TUNE_HYBRID: (1, None, None),
    capi.VRS_TUNE_HYBRID_MIN_KEYS: (0, -1, "hybrid threshold must be >= 0"),
    capi.VRS_TUNE_HYBRID_FAST_COUNT: (1, 3, "fast count mode must be 0, 1 or 2"),
    capi.VRS_TUNE_ASYNC_SORT: (1, None, None),
    capi.VRS_TUNE_PLAN_WAIT_MS: (60000, -1, "the plan wait limit must be >= 0 ms"),
    capi.VRS_TUNE_MSD_RESERVE: (1, 3, "MSD reservation must be 0 (never) or 1 / 2 (bare keys of the hybrid form)"),
    capi.VRS_TUNE_MSD_POOL: (1, -1, "the pool form must be 0 (never), 1 (adaptive) or 2 (always tried)"),
    capi.VRS_TUNE_MSD_POOL_MIN_KEYS: (1 << 22, (1 << 22) - 1, "the pool form takes 2^22 keys or more"),
    capi.VRS_TUNE_MSD_POOL_SUB_BITS: (0, 5, "the pool form's second pass sorts by 6, 7 or 8 bits (0 = by size)"),
    capi.VRS_TUNE_MSD_POOL_REUSE_LAYOUT: (1, None, None),
    capi.VRS_TUNE_MSD_POOL_PAIRS: (1, None, None),
    capi.VRS_TUNE_MSD_POOL_TOP_BITS: (7, 9, "the pool form's first pass sorts by 6, 7 (the default) or 8 bits"),
    capi.VRS_TUNE_MSD_POOL_PAIRS_PACKED: (-1, -2, "the pairs' packed local sort: -1 (by size), 0 (never) or 1 (always)"),
    capi.VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS: (1 << 20, -1, "the segmented sorts' one-call threshold must be >= 0"),
    capi.VRS_TUNE_TOPK_GRID_MIN_KEYS: (1 << 17, -1, "the top-k grid tier's threshold must be >= 0"),
    capi.VRS_TUNE_SEARCH_LDS_BYTES: (64 * 1024, 160 * 1024 + 1, "the search's LDS capacity must be 0 .. 163840 bytes"),
    capi.VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: (1 << 16, -1, "the search's table threshold must be >= 0"),
    capi.VRS_TUNE_SEARCH_INDEX_MIN_QUERIES: (1 << 16, -1, "the search's index threshold must be >= 0"),
    capi.VRS_TUNE_BINCOUNT_LDS_BYTES: (64 * 1024, -1, "the counting kernels' LDS capacity must be 0 .. 163840 bytes"),
    capi.VRS_TUNE_SELECT_GRID_MIN_KEYS: (1 << 17, -1, "the selection's grid tier threshold must be >= 0"),
    capi.VRS_TUNE_SELECT_COMPACT_DIVISOR: (16, -1, "the selection's compaction divisor must be >= 0"),
    capi.VRS_TUNE_REDUCE_CHUNK_ROWS: (512, 63, "the reduction's chunk must be 64 .. 4096 rows"),
    capi.VRS_TUNE_REDUCE_LANE_ROWS: (16, 65, "the reduction's lane map takes 0 .. 64 rows"),
    capi.VRS_TUNE_SCAN_TILE_ROWS: (2048, 8192 + 256, "the scan's tile must be a multiple of 256 in 256 .. 8192 rows"),
    capi.VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS: (1 << 20, -1, "the scan's single pass starts at 0 (never) or more rows"),
    capi.VRS_TUNE_SCAN_SPIN_BUDGET: (4096, (1 << 20) + 1, "the scan's spin budget must be 0 .. 1048576 polls"),
    capi.VRS_TUNE_COMPACT_TILE_ELEMS: (16384, 4096 + 1, "the compaction's tile must be a multiple of 4096 in 4096 .. 65536 elements"),
}
LEFT_OUT = {capi.VRS_TUNE_DEBUG_XCC_STRAY_BLOCK, capi.VRS_TUNE_DEBUG_XCC_ROTATE, capi.VRS_TUNE_DEBUG_POOL_NO_MEMORY}


def test_defaults_refusals_and_the_sorts_that_read_them():
    assert set(KEYS) | LEFT_OUT == set(range(41))
    B = vrs.Buffer.BufferSettings
    with vrs.GPUContext(0) as ctx:
        lib = ctx.lib

        def refused(key, value, message):
            assert lib.vrs_set_tuning(ctx.handle, key, value) == capi.VRS_ERROR_INVALID_ARGUMENT, (key, value)
            assert lib.vrs_last_error(ctx.handle).decode() == message, (key, value)

        for key, (default, outside, message) in KEYS.items():
            assert lib.vrs_set_tuning(ctx.handle, key, default) == capi.VRS_OK, (key, lib.vrs_last_error(ctx.handle))
            if outside is not None:
                refused(key, outside, message)
        refused(41, 0, "unknown tuning key")
        refused(-1, 0, "unknown tuning key")
        assert ctx.tuning == {}  # (the raw calls above do not go through setTuning)

        rng = np.random.default_rng(41)
        keys = rng.integers(0, 1 << 32, 10000, dtype=np.uint64).astype(np.uint32)  # above the single-launch size: the one-call path
        k0, k1 = vrs.Buffer.fillDeviceWithStagingBuffer(ctx, B(4 * keys.size), keys), vrs.Buffer(ctx, B(4 * keys.size))
        ctx.check(lib.vrs_sort_keys_u32(ctx.handle, k0.handle, k1.handle, keys.size))
        out = np.empty_like(keys)
        k0.downloadWithStagingBuffer(out)
        assert np.array_equal(out, np.sort(keys))

        offsets = np.array([0, 1000, 1003, 5000], dtype=np.uint32)  # three segments, 5 000 keys in all
        seg_keys = keys[:5000].copy()
        s0, s1 = vrs.Buffer.fillDeviceWithStagingBuffer(ctx, B(4 * seg_keys.size), seg_keys), vrs.Buffer(ctx, B(4 * seg_keys.size))
        off = vrs.Buffer.fillDeviceWithStagingBuffer(ctx, B(4 * offsets.size), offsets)
        ctx.check(lib.vrs_sort_segments_u32(ctx.handle, s0.handle, s1.handle, seg_keys.size, off.handle, offsets.size - 1))
        got = np.empty_like(seg_keys)
        s0.downloadWithStagingBuffer(got)
        want = np.concatenate([np.sort(seg_keys[b:e]) for b, e in zip(offsets[:-1], offsets[1:])])
        assert np.array_equal(got, want)
        for b in (k0, k1, s0, s1, off):
            b.release()
