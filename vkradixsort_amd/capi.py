"""ctypes binding of the C ABI in the four headers under include/ (HEADERS below; the ONLY way Python reaches the GPU path).

There is no fallback: if libvkradixsort_amd.so has not been built, or no HIP device is present, the
calls raise.  Nothing here imports or knows about oracle/.
"""
from __future__ import annotations

import ctypes
from ctypes import (POINTER, Structure, byref, c_char_p, c_double, c_int, c_size_t, c_uint32, c_uint64,
                    c_void_p)
from pathlib import Path

import os as _os

# VRS_LIB: another build of the SAME library (the sanitizer builds: vkradixsort_amd/_build/san_asan/libvkradixsort_amd.so under a preloaded
# runtime, tools/asan_fuzz.sh) -- never another implementation: there is none
LIB_PATH = Path(_os.environ["VRS_LIB"]).resolve() if _os.environ.get("VRS_LIB") else Path(__file__).resolve().parent / "libvkradixsort_amd.so"

VRS_OK = 0
VRS_ERROR_INVALID_ARGUMENT = 1
VRS_ERROR_HIP = 2
VRS_ERROR_NO_DEVICE = 3
VRS_ERROR_OUT_OF_MEMORY = 4
VRS_ERROR_UNBALANCED = 5
VRS_ERROR_TIMEOUT = 6
VRS_ERROR_PEER = 7

VRS_KERNEL_HISTOGRAM = 0
VRS_KERNEL_PREFIX = 1
VRS_KERNEL_SCATTER = 2
VRS_KERNEL_SINGLE = 3
VRS_KERNEL_DIGIT_TABLES = 4
VRS_KERNEL_LOOKBACK_SCATTER = 5
VRS_KERNEL_LOCAL_SORT = 6
VRS_KERNEL_POOL_SAMPLE = 7
VRS_KERNEL_POOL_PASS_A = 8
VRS_KERNEL_POOL_PASS_B = 9
VRS_KERNEL_COUNT = 10
KERNEL_NAMES = {0: "histogram", 1: "prefix", 2: "scatter", 3: "single", 4: "digit_tables", 5: "lookback_scatter",
                6: "local_sort", 7: "pool_sample", 8: "pool_pass_a", 9: "pool_pass_b"}

VRS_KEYS_INT32 = 0
VRS_KEYS_FLOAT32_TO_SORTABLE = 1
VRS_KEYS_SORTABLE_TO_FLOAT32 = 2

VRS_TUNE_XCD_REMAP = 0
VRS_TUNE_SCATTER_VARIANT = 1
VRS_TUNE_FUSED_PREFIX = 2
VRS_TUNE_RANK_MODE = 3
VRS_TUNE_ONE_CALL_MIN_KEYS = 4
ONE_CALL_MIN_KEYS_DEFAULT = 1 << 13  # the library's default for VRS_TUNE_ONE_CALL_MIN_KEYS
VRS_TUNE_DEBUG_MISPLACE_STREAMS = 5
VRS_TUNE_LOOKBACK_SPIN_BUDGET = 6
VRS_TUNE_DEBUG_HOLD_TILE = 7
VRS_TUNE_DIGIT_TABLE_GROUPS = 8
VRS_TUNE_SINGLE_MAX_KEYS = 9
VRS_TUNE_FUSED_PLAN = 10
VRS_TUNE_HYBRID = 11
VRS_TUNE_HYBRID_MIN_KEYS = 12
VRS_TUNE_HYBRID_FAST_COUNT = 13
VRS_TUNE_ASYNC_SORT = 14
VRS_TUNE_PLAN_WAIT_MS = 15
VRS_TUNE_MSD_RESERVE = 16
VRS_TUNE_MSD_POOL = 17
VRS_TUNE_MSD_POOL_MIN_KEYS = 18
VRS_TUNE_DEBUG_XCC_STRAY_BLOCK = 19
VRS_TUNE_MSD_POOL_SUB_BITS = 20
VRS_TUNE_DEBUG_XCC_ROTATE = 21
VRS_TUNE_MSD_POOL_REUSE_LAYOUT = 22
VRS_TUNE_MSD_POOL_PAIRS = 23
VRS_TUNE_MSD_POOL_TOP_BITS = 24
VRS_TUNE_DEBUG_POOL_NO_MEMORY = 25
VRS_TUNE_MSD_POOL_PAIRS_PACKED = 26
VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS = 27
SEGMENT_ONE_CALL_MIN_KEYS_DEFAULT = 1 << 20  # the library's default for VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS
# tiers of the segmented sorts (vrs_segment_tier) and the lengths that bound them
VRS_SEGMENT_WAVE, VRS_SEGMENT_BLOCK, VRS_SEGMENT_GLOBAL, VRS_SEGMENT_ONE_CALL = 0, 1, 2, 3
SEGMENT_WAVE_MAX = 1789
SEGMENT_BLOCK_MAX_KEYS, SEGMENT_BLOCK_MAX_PAIRS = 14333, 13312
SEGMENT_WAVE_MAX_U64 = 896  # the 64-bit forms (vrs_sort_segments_u64 / _pairs_u64)
SEGMENT_BLOCK_MAX_KEYS_U64, SEGMENT_BLOCK_MAX_PAIRS_U64 = 13312, 6656
VRS_TUNE_TOPK_GRID_MIN_KEYS = 28
TOPK_GRID_MIN_KEYS_DEFAULT = 1 << 17  # the library's default for VRS_TUNE_TOPK_GRID_MIN_KEYS
# top-k selection: key types, flags, tiers (vrs_topk_tier) and the lengths that bound them
VRS_TOPK_U32, VRS_TOPK_I32, VRS_TOPK_F32 = 0, 1, 2
VRS_TOPK_LARGEST, VRS_TOPK_SORTED = 1, 2
VRS_TOPK_RANK64 = 16  # goes with VRS_TOPK_DTYPE of int64 / float64: the scratch's sort area holds 8-byte ranks
VRS_TOPK_DTYPE_BASE = 0x100
VRS_TOPK_LDS, VRS_TOPK_BLOCK, VRS_TOPK_GRID = 0, 1, 2
TOPK_LDS_MAX = 8192
TOPK_SORT_IN_LDS_MAX_K = 4096  # VRS_TOPK_SORTED beyond this k sorts the survivors with vrs_sort_segments_pairs_u32
# one-rank selection (vrs_select_segments): modes, the flag, tiers (vrs_select_tier), the LDS tier's bytes of ranks, tuning keys and defaults
VRS_SELECT_KTH, VRS_SELECT_MEDIAN, VRS_SELECT_NANMEDIAN = 0, 1, 2
VRS_SELECT_DESCENDING = 1
VRS_SELECT_LDS, VRS_SELECT_BLOCK, VRS_SELECT_GRID = 0, 1, 2
SELECT_LDS_BYTES = 32 * 1024
VRS_TUNE_SELECT_GRID_MIN_KEYS, VRS_TUNE_SELECT_COMPACT_DIVISOR = 33, 34
SELECT_GRID_MIN_KEYS_DEFAULT, SELECT_COMPACT_DIVISOR_DEFAULT = 1 << 17, 16
# multi-rank selection (vrs_quantile_segments): interpolations, the flag, the most targets per segment (its tiers and tuning keys are the selection's)
VRS_QUANTILE_LINEAR, VRS_QUANTILE_LOWER, VRS_QUANTILE_HIGHER, VRS_QUANTILE_MIDPOINT, VRS_QUANTILE_NEAREST = 0, 1, 2, 3, 4
VRS_QUANTILE_IGNORE_NAN = 1
VRS_QUANTILE_MAX_TARGETS = 16
# run-length encoding and unique: scratch flags, key types, and the encode's tile (keys per look-back status word)
VRS_RLE_COUNTS = 1
VRS_UNIQUE_U32, VRS_UNIQUE_I32, VRS_UNIQUE_F32, VRS_UNIQUE_U64, VRS_UNIQUE_I64, VRS_UNIQUE_F64 = 0, 1, 2, 3, 4, 5
VRS_UNIQUE_INVERSE, VRS_UNIQUE_COUNTS = 1, 2
RLE_TILE = 4096
VRS_UNIQUE_COLUMNS_SHIFT = 8


def VRS_TOPK_DTYPE(d: int) -> int:
    """The top-k key type of an element of dtype d (a VRS_SORT_* code), ranked in torch's order."""
    return VRS_TOPK_DTYPE_BASE | d


def VRS_UNIQUE_COLUMNS(c: int) -> int:
    """the columns per row of the row forms, for vrs_unique's key_type and vrs_run_length_encode's key_bytes (bits 8 and up)"""
    return int(c) << VRS_UNIQUE_COLUMNS_SHIFT


# the torch.sort drop-in's rank / restore kernels: dtypes (vrs_sort_dtype) and flags
(VRS_SORT_INT8, VRS_SORT_UINT8, VRS_SORT_INT16, VRS_SORT_INT32, VRS_SORT_INT64, VRS_SORT_FLOAT16, VRS_SORT_BFLOAT16, VRS_SORT_FLOAT32,
 VRS_SORT_FLOAT64) = range(9)
VRS_SORT_DESCENDING = 1
VRS_SORT_MODE = 2  # vrs_sort_restore only: the mode form (positions is then the call's scratch)
# sorted-sequence search (vrs_search_sorted): flags, tiers (vrs_search_tier), tuning keys and the library's defaults for them
VRS_SEARCH_RIGHT, VRS_SEARCH_OUT_INT64 = 1, 2
VRS_SEARCH_MEMBER, VRS_SEARCH_MEMBER_INVERT = 16, 32  # the membership form (isin): a byte per query; bits 4 and 8 stay refused
VRS_SEARCH_LDS, VRS_SEARCH_TABLE, VRS_SEARCH_DIRECT, VRS_SEARCH_INDEXED = 0, 1, 2, 3
VRS_TUNE_SEARCH_LDS_BYTES, VRS_TUNE_SEARCH_TABLE_MIN_QUERIES, VRS_TUNE_SEARCH_INDEX_MIN_QUERIES = 29, 30, 31
SEARCH_LDS_BYTES_DEFAULT, SEARCH_LDS_BYTES_MAX = 64 * 1024, 160 * 1024
SEARCH_TABLE_MIN_QUERIES_DEFAULT, SEARCH_INDEX_MIN_QUERIES_DEFAULT = 1 << 16, 1 << 16
SEARCH_LINE_BYTES = 128  # boundaries one index entry stands for
# counting (vrs_bin_count): modes, tiers (vrs_bincount_tier), the tuning key and the library's default for it, the launch's shape
VRS_BIN_INDEX, VRS_BIN_LINEAR = 0, 1
VRS_BIN_NO_WEIGHTS = -1
VRS_BINCOUNT_LDS, VRS_BINCOUNT_GLOBAL = 0, 1
VRS_TUNE_BINCOUNT_LDS_BYTES = 32
BINCOUNT_LDS_BYTES_DEFAULT, BINCOUNT_LDS_BYTES_MAX = 64 * 1024, 160 * 1024
BINCOUNT_TILE_BYTES = 16 * 1024  # of elements, per workgroup and step of its loop
BINCOUNT_WORKGROUPS_PER_CU = 2   # one when a workgroup's counters take more than half of BINCOUNT_LDS_BYTES_MAX
# segmented reduction (vrs_segment_reduce): ops, lane maps (vrs_reduce_map), tuning keys and the library's defaults for them
VRS_REDUCE_SUM, VRS_REDUCE_PROD, VRS_REDUCE_MIN, VRS_REDUCE_MAX = 0, 1, 2, 3
VRS_REDUCE_MAP_LANE, VRS_REDUCE_MAP_ROWS, VRS_REDUCE_MAP_COLUMNS = 0, 1, 2
VRS_TUNE_REDUCE_CHUNK_ROWS, VRS_TUNE_REDUCE_LANE_ROWS = 35, 36
REDUCE_CHUNK_ROWS_DEFAULT, REDUCE_LANE_ROWS_DEFAULT = 512, 16
# prefix scan over rows (vrs_scan_rows): ops, tiers (vrs_scan_tier), tuning keys, the library's defaults for them and the order's constants
VRS_SCAN_SUM, VRS_SCAN_PROD, VRS_SCAN_MAX, VRS_SCAN_MIN = 0, 1, 2, 3
VRS_SCAN_TILE, VRS_SCAN_THREE_LAUNCH, VRS_SCAN_SINGLE_PASS = 0, 1, 2
VRS_TUNE_SCAN_TILE_ROWS, VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS, VRS_TUNE_SCAN_SPIN_BUDGET = 37, 38, 39
SCAN_TILE_ROWS_DEFAULT, SCAN_SINGLE_PASS_MIN_ROWS_DEFAULT, SCAN_SPIN_BUDGET_DEFAULT = 2048, 1 << 20, 4096
SCAN_TILE_ROWS_MIN, SCAN_TILE_ROWS_MAX, SCAN_FAN = 256, 8192, 64
# ordered compaction (vrs_compact_*): bool's dtype code after the nine of vrs_sort_dtype, the coordinate layouts, the tuning key, its
# default and range, and the constants of the phases (a chunk is what one step of emit stages in LDS; the carries take a block per step)
VRS_COMPACT_BOOL = 9
VRS_COMPACT_ROWS, VRS_COMPACT_COLUMNS = 0, 1
VRS_TUNE_COMPACT_TILE_ELEMS = 40
COMPACT_TILE_ELEMS_DEFAULT, COMPACT_TILE_ELEMS_MIN, COMPACT_TILE_ELEMS_MAX = 16384, 4096, 65536
COMPACT_CHUNK, COMPACT_CARRY_BLOCK, COMPACT_MAX_DIMS = 4096, 4096, 8
FORM_NAMES = {0: "none", 1: "single", 2: "contract", 3: "lsd", 4: "counted", 5: "pool"}
FORM_KNOBS = ["single_max_keys", "one_call_min_keys", "hybrid_min_keys", "pool_min_keys", "hybrid", "pool", "pool_pairs", "reserve", "groups", "xcc_map_valid",
              "atomic_rank", "pool_skip", "pool_skip_n", "wide_refused", "wide_skipped", "no_pool", "no_hybrid"]
# keys the local sort of one top-14-bit bucket can hold (msd_local_capacity): uint32 keys with the 256- / 512-thread workgroup, pairs and 64-bit keys
LOCAL_SORT_SMALL_KEYS, LOCAL_SORT_MAX_KEYS = 7165, 14333
LOCAL_SORT_SMALL_PAIRS, LOCAL_SORT_MAX_PAIRS = 6656, 13312  # pairs and 64-bit keys: 512 / 1024-thread workgroups
HYBRID_MIN_KEYS_DEFAULT = 0  # vrs_tuning.hpp: hybrid_min_keys == 0: the measured crossovers (1.3e7 keys, 2.5e7 pairs, 2e7 64-bit keys)
# the library's default per tuning key, for the keys that have a *_DEFAULT name above: what GPUContext.tuned(key) returns until the key
# is set.  tests/test_tuning_cpu.py holds every entry (and every *_MIN / *_MAX) against the table in csrc/vrs_tuning.hpp
TUNING_DEFAULTS = {
    VRS_TUNE_ONE_CALL_MIN_KEYS: ONE_CALL_MIN_KEYS_DEFAULT, VRS_TUNE_HYBRID_MIN_KEYS: HYBRID_MIN_KEYS_DEFAULT,
    VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS: SEGMENT_ONE_CALL_MIN_KEYS_DEFAULT, VRS_TUNE_TOPK_GRID_MIN_KEYS: TOPK_GRID_MIN_KEYS_DEFAULT,
    VRS_TUNE_SELECT_GRID_MIN_KEYS: SELECT_GRID_MIN_KEYS_DEFAULT, VRS_TUNE_SELECT_COMPACT_DIVISOR: SELECT_COMPACT_DIVISOR_DEFAULT,
    VRS_TUNE_SEARCH_LDS_BYTES: SEARCH_LDS_BYTES_DEFAULT, VRS_TUNE_SEARCH_TABLE_MIN_QUERIES: SEARCH_TABLE_MIN_QUERIES_DEFAULT,
    VRS_TUNE_SEARCH_INDEX_MIN_QUERIES: SEARCH_INDEX_MIN_QUERIES_DEFAULT, VRS_TUNE_BINCOUNT_LDS_BYTES: BINCOUNT_LDS_BYTES_DEFAULT,
    VRS_TUNE_REDUCE_CHUNK_ROWS: REDUCE_CHUNK_ROWS_DEFAULT, VRS_TUNE_REDUCE_LANE_ROWS: REDUCE_LANE_ROWS_DEFAULT,
    VRS_TUNE_SCAN_TILE_ROWS: SCAN_TILE_ROWS_DEFAULT, VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS: SCAN_SINGLE_PASS_MIN_ROWS_DEFAULT,
    VRS_TUNE_SCAN_SPIN_BUDGET: SCAN_SPIN_BUDGET_DEFAULT, VRS_TUNE_COMPACT_TILE_ELEMS: COMPACT_TILE_ELEMS_DEFAULT,
}


class PushConstants(Structure):
    """vrs_push_constants == MultiRadixSortPass::PushConstants(Histograms), 16 bytes std430."""
    _fields_ = [("g_num_elements", c_uint32), ("g_shift", c_uint32), ("g_num_workgroups", c_uint32),
                ("g_num_blocks_per_workgroup", c_uint32)]


class VrsError(RuntimeError):
    """Every failure of the reference is a std::runtime_error; this is its Python spelling."""

    def __init__(self, code: int, message: str):
        super().__init__(f"vkradixsort_amd error {code}: {message}")
        self.code = code
        self.message = message


class DistTransport(ctypes.Structure):
    """vrs_dist_transport: the wire of the multi-GPU step as a table of functions (include/vkradixsort_amd_dist.h)."""
    _fields_ = [("user", c_void_p), ("all_gather", c_void_p), ("all_reduce", c_void_p), ("group_start", c_void_p),
                ("send", c_void_p), ("recv", c_void_p), ("group_end", c_void_p), ("error_string", c_void_p)]


class CompactOutputs(ctypes.Structure):
    """vrs_compact_outputs: what vrs_compact_emit writes (include/vkradixsort_amd_ops.h "K15")."""
    _fields_ = [("num_selected", c_uint64), ("flat", c_void_p), ("coords", c_void_p), ("coords_layout", c_int), ("ndim", c_uint32),
                ("shape", c_uint32 * 8), ("gather_values", c_void_p), ("gather_out", c_void_p), ("value_bytes", c_uint32),
                ("row_elems", c_uint32), ("scatter_input", c_void_p), ("scatter_source", c_void_p), ("scatter_out", c_void_p)]


class CompactHostOutputs(ctypes.Structure):
    """vrs_compact_host_outputs: the same on host pointers, for vrs_compact_host."""
    _fields_ = [("flat", c_void_p), ("coords", c_void_p), ("coords_layout", c_int), ("ndim", c_uint32), ("shape", c_uint32 * 8),
                ("gather_values", c_void_p), ("gather_out", c_void_p), ("value_bytes", c_uint32), ("row_elems", c_uint32),
                ("scatter_input", c_void_p), ("scatter_source", c_void_p), ("scatter_source_elems", c_uint64), ("scatter_out", c_void_p)]


MSD_COUNT_WORDS = 16384 + 8 * 256 + 64
MSD_SHIFT_WORD = 16384 + 8 * 256

HEADERS = [Path(__file__).resolve().parent.parent / "include" / name for name in ("vkradixsort_amd.h", "vkradixsort_amd_ops.h", "vkradixsort_amd_dist.h", "vkradixsort_amd_tune.h")]

# every symbol the four headers declare, per header and in the header's order: (name, restype, argtypes)
_SIGNATURES = {
    "vkradixsort_amd.h": [
        ("vrs_device_count", c_int, [POINTER(c_int)]),
        ("vrs_context_create", c_int, [c_int, POINTER(c_void_p)]),
        ("vrs_context_create_on_stream", c_int, [c_int, c_void_p, POINTER(c_void_p)]),
        ("vrs_context_destroy", c_int, [c_void_p]),
        ("vrs_last_error", c_char_p, [c_void_p]),
        ("vrs_context_stream", c_void_p, [c_void_p]),
        ("vrs_context_device", c_int, [c_void_p]),
        ("vrs_device_info", c_int, [c_void_p, c_char_p, c_size_t, POINTER(c_int), POINTER(c_uint64)]),
        ("vrs_context_trim_scratch", c_int, [c_void_p, POINTER(c_uint64)]),
        ("vrs_buffer_create", c_int, [c_void_p, c_size_t, POINTER(c_void_p)]),
        ("vrs_buffer_wrap", c_int, [c_void_p, c_void_p, c_size_t, POINTER(c_void_p)]),
        ("vrs_buffer_release", c_int, [c_void_p]),
        ("vrs_buffer_upload", c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
        ("vrs_buffer_download", c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
        ("vrs_buffer_copy", c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
        ("vrs_buffer_device_ptr", c_void_p, [c_void_p]),
        ("vrs_buffer_size_bytes", c_size_t, [c_void_p]),
        ("vrs_global_invocation_size", c_uint32, [c_uint32, c_uint32]),
        ("vrs_workgroup_count", c_uint32, [c_uint32, c_uint32]),
        ("vrs_multi_radixsort_histograms", c_int, [c_void_p, c_void_p, c_void_p, POINTER(PushConstants)]),
        ("vrs_multi_radixsort", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(PushConstants)]),
        ("vrs_multi_radixsort_pairs", c_int,
         [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(PushConstants)]),
        ("vrs_multi_radixsort_digit_offsets", c_int, [c_void_p, c_void_p]),
        ("vrs_multi_radixsort_histograms_u64", c_int, [c_void_p, c_void_p, c_void_p, POINTER(PushConstants)]),
        ("vrs_multi_radixsort_u64", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(PushConstants)]),
        ("vrs_multi_radixsort_pairs_u64", c_int,
         [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(PushConstants)]),
        ("vrs_queue_wait_idle", c_int, [c_void_p]),
        ("vrs_single_radixsort", c_int, [c_void_p, c_void_p, c_void_p, c_uint32]),
        ("vrs_sort_keys_u32", c_int, [c_void_p, c_void_p, c_void_p, c_uint32]),
        ("vrs_sort_settle", c_int, [c_void_p]),
        ("vrs_sort_pending", c_int, [c_void_p]),
        ("vrs_sort_pairs_u32", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32]),
        ("vrs_sort_keys_u64", c_int, [c_void_p, c_void_p, c_void_p, c_uint32]),
        ("vrs_sort_pairs_u64", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32]),
        ("vrs_transform_keys", c_int, [c_void_p, c_void_p, c_uint32, c_int]),
        ("vrs_verify_keys_u32", c_int, [c_void_p, c_void_p, c_uint32, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
        ("vrs_version", c_char_p, []),
    ],
    "vkradixsort_amd_ops.h": [
        ("vrs_sort_segments_u32", c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32]),
        ("vrs_sort_segments_pairs_u32", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32]),
        ("vrs_segmented_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
        ("vrs_segment_tier_for", c_int, [c_uint32, c_uint32, c_uint32, c_int, c_uint32, POINTER(c_int), POINTER(c_uint32), POINTER(c_uint32)]),
        ("vrs_sort_segments_u64", c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32]),
        ("vrs_sort_segments_pairs_u64", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32]),
        ("vrs_segment_tier_for_u64", c_int, [c_uint32, c_uint32, c_uint32, c_int, c_uint32, POINTER(c_int), POINTER(c_uint32), POINTER(c_uint32)]),
        ("vrs_sort_rank_keys", c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_int, c_int, c_void_p, c_void_p]),
        ("vrs_sort_restore", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_uint32, c_int, c_int, c_void_p, c_void_p]),
        ("vrs_sort_rank_bytes", c_int, [c_int, POINTER(c_int)]),
        ("vrs_topk_segments", c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_uint32, c_int, c_int, c_void_p, c_void_p, c_void_p]),
        ("vrs_topk_scratch_bytes", c_int, [c_uint32, c_uint32, c_uint32, c_int, POINTER(c_uint64)]),
        ("vrs_topk_tier_for", c_int, [c_uint32, c_uint32, c_uint32, c_uint32, POINTER(c_int), POINTER(c_uint32), POINTER(c_uint32)]),
        ("vrs_topk_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
        ("vrs_select_segments", c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_int, c_int, c_uint32, c_int, c_void_p, c_void_p, c_void_p]),
        ("vrs_select_scratch_bytes", c_int, [c_uint32, c_uint32, c_int, POINTER(c_uint64)]),
        ("vrs_select_tier_for", c_int, [c_uint32, c_uint32, c_uint32, c_int, c_uint32, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_int)]),
        ("vrs_select_target_for", c_int, [c_int, c_uint32, c_uint32, c_uint32, c_int, POINTER(c_uint32), POINTER(c_int)]),
        ("vrs_select_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
        ("vrs_quantile_segments", c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_int, POINTER(c_double), c_uint32, c_int, c_int, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p]),
        ("vrs_quantile_scratch_bytes", c_int, [c_uint32, c_uint32, c_int, POINTER(c_uint64)]),
        ("vrs_quantile_target_for", c_int, [c_int, c_int, c_double, c_uint32, c_uint32, c_int, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_double), POINTER(c_int)]),
        ("vrs_quantile_level_for", c_int, [c_int, c_int, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_int)]),
        ("vrs_quantile_host", c_int, [c_void_p, c_uint32, c_void_p, c_uint32, c_int, POINTER(c_double), c_uint32, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
        ("vrs_quantile_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
        ("vrs_search_sorted", c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, c_int, c_int, c_void_p, c_void_p, c_void_p]),
        ("vrs_search_tier_for", c_int, [c_uint32, c_uint32, c_uint32, c_uint32, c_int, c_uint32, c_uint32, c_uint32, POINTER(c_int)]),
        ("vrs_search_scratch_bytes", c_int, [c_uint32, c_uint32, c_int, c_int, c_int, POINTER(c_uint64)]),
        ("vrs_search_plan", c_int, [c_void_p, c_uint32, c_uint32, c_uint32, c_uint32, c_int, c_int, POINTER(c_int), POINTER(c_uint64)]),
        ("vrs_search_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
        ("vrs_bin_count", c_int, [c_void_p, c_void_p, c_uint32, c_int, c_int, c_double, c_double, c_uint32, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                  c_void_p]),
        ("vrs_bin_count_tier_for", c_int, [c_uint32, c_uint32, c_uint32, POINTER(c_int)]),
        ("vrs_bin_count_scratch_bytes", c_int, [c_uint32, c_int, c_int, POINTER(c_uint64)]),
        ("vrs_bin_count_plan", c_int, [c_void_p, c_uint32, c_int, c_int, POINTER(c_int), POINTER(c_uint64)]),
        ("vrs_bin_count_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64)]),
        ("vrs_bin_linear_host", c_int, [c_void_p, c_uint64, c_int, c_double, c_double, c_uint32, c_void_p]),
        ("vrs_segment_reduce", c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_int, c_void_p, c_void_p, c_uint32, c_int, c_void_p, c_void_p, c_void_p]),
        ("vrs_segment_reduce_scratch_bytes", c_int, [c_uint32, c_uint32, c_uint32, c_int, c_uint32, POINTER(c_uint64)]),
        ("vrs_segment_reduce_map_for", c_int, [c_uint32, c_uint32, c_uint32, POINTER(c_int)]),
        ("vrs_segment_reduce_levels_for", c_int, [c_uint32, c_uint32, POINTER(c_uint32)]),
        ("vrs_segment_reduce_host", c_int, [c_void_p, c_uint64, c_uint32, c_int, c_void_p, c_void_p, c_uint32, c_int, c_void_p, c_uint32, c_uint32, c_void_p]),
        ("vrs_segment_reduce_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
        ("vrs_scan_rows", c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
        ("vrs_scan_tier_for", c_int, [c_uint32, c_uint32, c_uint32, c_int, c_int, c_int, c_uint32, c_uint32, POINTER(c_int)]),
        ("vrs_scan_levels_for", c_int, [c_uint32, c_uint32, POINTER(c_uint32)]),
        ("vrs_scan_depth_for", c_int, [c_uint32, c_uint32, c_uint32, POINTER(c_uint32)]),
        ("vrs_scan_scratch_bytes", c_int, [c_uint32, c_uint32, c_uint32, c_int, c_int, c_int, c_uint32, c_uint32, POINTER(c_uint64)]),
        ("vrs_scan_rows_host", c_int, [c_void_p, c_uint32, c_uint32, c_uint32, c_int, c_int, c_int, c_uint32, c_void_p, c_void_p]),
        ("vrs_scan_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
        ("vrs_compact_count", c_int, [c_void_p, c_void_p, c_uint64, c_int, c_void_p, c_void_p, POINTER(c_uint64)]),
        ("vrs_compact_emit", c_int, [c_void_p, c_void_p, c_uint64, c_int, c_void_p, POINTER(CompactOutputs)]),
        ("vrs_compact_tiles_for", c_int, [c_uint64, c_uint32, POINTER(c_uint32)]),
        ("vrs_compact_scratch_bytes", c_int, [c_uint64, c_uint32, POINTER(c_uint64)]),
        ("vrs_compact_divide", c_int, [c_uint32, c_uint32, POINTER(c_uint32), POINTER(c_uint32)]),
        ("vrs_compact_host", c_int, [c_void_p, c_uint64, c_int, POINTER(CompactHostOutputs), POINTER(c_uint64)]),
        ("vrs_compact_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
        ("vrs_run_length_encode", c_int, [c_void_p, c_void_p, c_uint32, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
        ("vrs_run_length_encode_scratch_bytes", c_int, [c_uint32, c_int, c_int, POINTER(c_uint64)]),
        ("vrs_unique", c_int, [c_void_p, c_void_p, c_uint32, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
        ("vrs_unique_scratch_bytes", c_int, [c_uint32, c_int, c_int, POINTER(c_uint64)]),
    ],
    "vkradixsort_amd_dist.h": [
        ("vrs_sort_keys_u32_ranged", c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_uint32]),
        ("vrs_range_partition", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_uint32]),
        ("vrs_multi_radixsort_digit_offsets_device", c_int, [c_void_p, c_void_p]),
        ("vrs_multi_radixsort_offsets_hook", c_int, [c_void_p, c_void_p, c_void_p]),
        ("vrs_msd_partition_u32", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32]),
        ("vrs_msd_partition_signal_u32", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p]),
        ("vrs_msd_finish_u32", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_uint32]),
        ("vrs_msd_finish_grouped_u32", c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_uint32, c_uint32]),
        ("vrs_msd_finish_grouped_counts_u32", c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, POINTER(c_uint32)]),
        ("vrs_msd_finish_grouped_split_u32", c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_uint32, c_uint32, POINTER(c_uint32), POINTER(c_uint32)]),
        ("vrs_msd_finish_status", c_int, [c_void_p, POINTER(c_int)]),
        ("vrs_msd_finish_ticket", c_int, [c_void_p, POINTER(c_uint32)]),
        ("vrs_msd_finish_status_at", c_int, [c_void_p, c_uint32, POINTER(c_int)]),
        ("vrs_dist_create", c_int, [c_void_p, c_void_p, c_int, c_int, c_uint32, c_int, POINTER(c_void_p)]),
        ("vrs_dist_create_with_transport", c_int, [c_void_p, c_void_p, c_int, c_int, c_uint32, c_int, POINTER(c_void_p)]),
        ("vrs_dist_destroy", c_int, [c_void_p]),
        ("vrs_dist_sort_keys_u32", c_int, [c_void_p, c_void_p, c_uint32, POINTER(c_void_p), POINTER(c_uint32)]),
        ("vrs_dist_plan_splitters", c_int, [POINTER(c_uint64), c_int, POINTER(c_uint32)]),
        ("vrs_dist_plan_sampled_splitters", c_int, [POINTER(c_uint32), POINTER(c_uint64), c_int, c_uint32, c_int, POINTER(c_uint32)]),
        ("vrs_dist_last_error", c_char_p, [c_void_p]),
        ("vrs_dist_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
        ("vrs_dist_grouped_rounds", c_int, [c_void_p, POINTER(c_uint64)]),
        ("vrs_dist_splitter_steps", c_int, [c_void_p, POINTER(c_uint64)]),
        ("vrs_dist_loopback_create", c_int, [c_int, POINTER(c_void_p)]),
        ("vrs_dist_loopback_create_host", c_int, [c_int, POINTER(c_void_p)]),
        ("vrs_dist_loopback_transport", c_int, [c_void_p, c_int, c_void_p]),
        ("vrs_dist_loopback_destroy", c_int, [c_void_p]),
        ("vrs_dist_loopback_set_wire", c_int, [c_void_p, c_double, c_double]),
    ],
    "vkradixsort_amd_tune.h": [
        ("vrs_profile_enable", c_int, [c_void_p, c_int]),
        ("vrs_profile_enable_mask", c_int, [c_void_p, c_uint32]),
        ("vrs_profile_reset", c_int, [c_void_p]),
        ("vrs_profile_query", c_int, [c_void_p, c_int, POINTER(c_uint64), POINTER(c_double)]),
        ("vrs_profile_query_launch", c_int, [c_void_p, c_int, c_uint64, POINTER(c_double)]),
        ("vrs_one_call_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
        ("vrs_one_call_relaunched_passes", c_int, [c_void_p, POINTER(c_uint64)]),
        ("vrs_one_call_hybrid_sorts", c_int, [c_void_p, POINTER(c_uint64)]),
        ("vrs_one_call_hybrid_recounts", c_int, [c_void_p, POINTER(c_uint64)]),
        ("vrs_sort_form_for", c_int, [c_uint32, c_int, c_int, POINTER(ctypes.c_int64), c_int, POINTER(c_int), POINTER(ctypes.c_int64)]),
        ("vrs_one_call_pool_sorts", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64)]),
        ("vrs_pool_form_shape", c_int, [c_uint32, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint64)]),
        ("vrs_pool_form_shape_ex", c_int, [c_uint32, c_int, c_int, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint64)]),
        ("vrs_one_call_pool_retries", c_int, [c_void_p, POINTER(c_uint64)]),
        ("vrs_one_call_pool_no_memory", c_int, [c_void_p, POINTER(c_uint64)]),
        ("vrs_one_call_pool_layouts", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64)]),
        ("vrs_rank_mode", c_int, [c_void_p]),
        ("vrs_set_tuning", c_int, [c_void_p, c_int, c_int]),
        ("vrs_debug_download_offsets", c_int, [c_void_p, c_void_p, c_size_t]),
        ("vrs_debug_atomic_rank_selftest", c_int, [c_void_p, c_uint32, c_uint32, POINTER(c_uint64)]),
        ("vrs_debug_xcc_placement", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_int)]),
    ],
}

EXPORTED_SYMBOLS = [s[0] for sigs in _SIGNATURES.values() for s in sigs]

_lib = None


def _preload_torch_hip_runtime() -> None:
    """One HIP runtime per process.  The PyTorch-ROCm wheel bundles its own libamdhip64.so (same SONAME as
    /opt/rocm's).  If this library pulled in the system copy first and torch were imported afterwards, the
    process would hold two runtimes and torch would report "No HIP GPUs are available".  So when torch is
    installed, map ITS runtime first (without importing torch); the SONAME match makes our library bind to it."""
    import importlib.util
    import os
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def load_library() -> ctypes.CDLL:
    """dlopen the in-tree library and type every entry point.  Raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback.")
    _preload_torch_hip_runtime()
    lib = ctypes.CDLL(str(LIB_PATH))
    for name, restype, argtypes in (sig for sigs in _SIGNATURES.values() for sig in sigs):
        fn = getattr(lib, name)  # AttributeError if the headers and the library ever diverge
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(ctx_handle, rc: int) -> None:
    if rc != VRS_OK:
        msg = load_library().vrs_last_error(ctx_handle)
        raise VrsError(rc, msg.decode() if msg else "unknown error")


def query_u64(name: str, *args) -> int:
    """The uint64 that the no-device query `name` (a *_scratch_bytes function) writes after its arguments; raises VrsError on failure."""
    out = ctypes.c_uint64()
    check(None, getattr(load_library(), name)(*args, ctypes.byref(out)))
    return out.value


def device_count() -> int:
    n = c_int(0)
    rc = load_library().vrs_device_count(byref(n))
    return n.value if rc == VRS_OK else 0
