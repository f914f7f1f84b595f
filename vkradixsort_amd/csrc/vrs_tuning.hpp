// vrs_tuning.hpp -- the one home of the tuning settings (vrs_set_tuning; include/vkradixsort_amd_tune.h documents every VRS_TUNE_* key):
// the struct that holds them, every default a named constant, and one table row per key -- the member the key stores into, how the
// int becomes that member, the accepted range and the refusal.  Pure host code without a HIP call: host/test/tuning_host.cpp walks it.
#pragma once
#include <climits>
#include <cstdint>

#include "vkradixsort_amd_tune.h"
#include "vrs_compact_order.hpp"
#include "vrs_kernels.h"
#include "vrs_scan_order.hpp"
#include "vrs_search.hpp"
#include "vrs_select.hpp"

namespace vrs {

// the defaults and bounds that no feature header names
constexpr bool kXcdRemapDefault = true, kFusedPrefixDefault = true, kFusedPlanDefault = false, kMisplaceDefault = false, kHybridDefault = true,
               kAsyncDefault = true, kPoolReuseDefault = true, kPoolReuseRoomsDefault = true;
constexpr uint32_t kOneCallDefaultMinKeys = 1u << 13;  // measured: the one-read form wins from the single-launch threshold on (profiles/r02_one_call_crossover.csv)
constexpr uint32_t kSingleDefaultMaxKeys = 4096u;      // measured crossover (profiles/r02_small_n_crossover.csv)
constexpr uint32_t kGroupsDefault = 0u, kGroupsMax = 32u;  // 0 = by size
constexpr uint32_t kLookbackDefaultSpinBudget = 4096u, kPlanWaitDefaultMs = 60000u;
constexpr int kHoldTileDefault = -1;  // off
constexpr uint32_t kHybridDefaultMinKeys = 0u;  // the measured crossovers per kind of sort: 1.3e7 bare uint32 keys (profiles/labs/r03_hybrid_by_size.txt), 2.5e7 pairs, 2e7 64-bit keys (profiles/labs/r02_*)
constexpr int kThreeWayMax = 2;  // the settings that are 0 never, 1 adaptive, 2 always (VRS_TUNE_MSD_RESERVE: 1 and 2 mean the same)
constexpr int kFastCountDefault = 1, kReserveDefault = 1, kPoolDefault = 1, kPoolPairsDefault = 1;
constexpr int kPoolPairsPackedDefault = -1, kPoolPairsPackedMax = 1;  // -1 by size, 0 never, 1 always
constexpr uint32_t kPoolDefaultMinKeys = 1u << 22;  // default AND floor: with one wave per small bucket the form beats the LSD passes from there on (labs/r05_pool_form.txt section 6)
constexpr int kPoolBitsMin = 6, kPoolBitsMax = 8;  // bits either pass of the pool form may sort by
constexpr int kPoolTopBitsDefault = 7;  // 7 + 7 bits: the first pass, which reads cold input, writes 64-key segments instead of 32-key ones (pairs -2.4 %, 10^7 keys -2.5 %, 10^8 keys -1 %)
constexpr int kPoolSubBitsDefault = 0;  // by size (pool_shape)
constexpr int kXccProbeBlocks = 4096, kXccRotateMax = 7;  // the placement probe's grid; places its result can be rotated by

// Every value a VRS_TUNE_* key stores, and nothing else (VRS_TUNE_SCATTER_VARIANT and _RANK_MODE live in vrs::ScatterLaunch, the debug
// keys of the placement probe and VRS_TUNE_DEBUG_POOL_NO_MEMORY act on the context's state).
struct Tuning {
    bool xcd_remap = kXcdRemapDefault;
    bool fused_prefix = kFusedPrefixDefault;
    // one-call sorts
    uint32_t one_call_min_keys = kOneCallDefaultMinKeys;
    uint32_t single_max_keys = kSingleDefaultMaxKeys;
    bool fused_plan = kFusedPlanDefault;
    uint32_t groups = kGroupsDefault;
    uint32_t spin_budget = kLookbackDefaultSpinBudget;
    int hold_tile = kHoldTileDefault;  // test hook
    bool misplace = kMisplaceDefault;  // test hook
    bool async = kAsyncDefault;        // conditional: create_context turns it off on a borrowed stream
    uint32_t plan_wait_ms = kPlanWaitDefaultMs;
    // hybrid form; hybrid_min_keys: a set value v means v keys, 5/8 v pairs, v/2 64-bit keys
    bool hybrid = kHybridDefault;
    int fast_count = kFastCountDefault;
    uint32_t hybrid_min_keys = kHybridDefaultMinKeys;
    int reserve = kReserveDefault;
    // pool form
    int pool = kPoolDefault;
    int pool_top_bits = kPoolTopBitsDefault;
    int pool_pairs = kPoolPairsDefault;
    int pool_pairs_packed = kPoolPairsPackedDefault;
    uint32_t pool_min_keys = kPoolDefaultMinKeys;
    int pool_sub_bits = kPoolSubBitsDefault;
    // VRS_TUNE_MSD_POOL_REUSE_LAYOUT: a sort of the same size and key floor as the context's last TAKEN pool sort runs its first pass in
    // the regions that sort's sample laid out.  Nothing is trusted: a region that does not fit, a key outside the kept range flag the
    // sort as ever; a refusal forgets the layout and the re-run samples.  reuse_rooms: the buckets' slack regions are kept with them
    bool pool_reuse = kPoolReuseDefault, pool_reuse_rooms = kPoolReuseRoomsDefault;
    // the newer operations
    uint32_t seg_one_call_min_keys = kSegDefaultOneCallMinKeys;
    uint32_t topk_grid_min_keys = kTopkDefaultGridMinKeys;
    uint32_t select_grid_min_keys = kSelDefaultGridMinKeys;  // vrs_quantile_segments reads the selection's two as well
    uint32_t select_compact_divisor = kSelDefaultCompactDivisor;
    uint32_t search_lds_bytes = kSearchDefaultLdsBytes;
    uint32_t search_table_min_queries = kSearchDefaultTableMinQueries;
    uint32_t search_index_min_queries = kSearchDefaultIndexMinQueries;
    uint32_t bincount_lds_bytes = kBinCountDefaultLdsBytes;
    uint32_t reduce_chunk_rows = kReduceChunkDefault;
    uint32_t reduce_lane_rows = kReduceLaneRowsDefault;
    uint32_t scan_tile_rows = kScanTileDefault;
    uint32_t scan_single_pass_min_rows = kScanSinglePassMinRowsDefault;
    uint32_t scan_spin_budget = kScanSpinBudgetDefault;
    uint32_t compact_tile_elems = kCompactTileDefault;
};

// One row per key.  At most one of the three members is set; none: vrs_set_tuning's own case for the key does what there is to do.
struct TuneRow {
    int key;
    bool Tuning::*flag;     // stored as value != 0
    uint32_t Tuning::*u32;  // stored by a cast
    int Tuning::*i32;       // stored as it is, or (as_01) as value != 0 ? 1 : 0
    bool as_01;
    int min, max, multiple;  // accepted: min .. max (INT_MIN / INT_MAX: no bound), a multiple of `multiple` ...
    bool (*among)(int);      // ... and, where set, only the values of the range this says yes to
    const char *refusal;
};
constexpr TuneRow tune_flag(int key, bool Tuning::*m) { return {key, m, nullptr, nullptr, false, INT_MIN, INT_MAX, 1, nullptr, nullptr}; }
constexpr TuneRow tune_u32(int key, uint32_t Tuning::*m, const char *refusal, int min = 0, int max = INT_MAX, int multiple = 1, bool (*among)(int) = nullptr) {
    return {key, nullptr, m, nullptr, false, min, max, multiple, among, refusal};
}
constexpr TuneRow tune_int(int key, int Tuning::*m, const char *refusal, int min, int max, bool (*among)(int) = nullptr) {
    return {key, nullptr, nullptr, m, false, min, max, 1, among, refusal};
}
constexpr TuneRow tune_check(int key, const char *refusal, int min, int max) { return {key, nullptr, nullptr, nullptr, false, min, max, 1, nullptr, refusal}; }

static_assert(8 % kStreams == 0, "every accepted VRS_TUNE_DIGIT_TABLE_GROUPS (8, 16, 32) must be a multiple of the stream count");
constexpr bool tune_groups_ok(int v) { return v == 0 || v == 8 || v == 16 || v == static_cast<int>(kGroupsMax); }
constexpr bool tune_sub_bits_ok(int v) { return v == 0 || v >= kPoolBitsMin; }

constexpr TuneRow kTuneTable[] = {  // in the order of the keys' values: row k is key k's (asserted below)
    tune_flag(VRS_TUNE_XCD_REMAP, &Tuning::xcd_remap),
    tune_check(VRS_TUNE_SCATTER_VARIANT, nullptr, INT_MIN, INT_MAX),
    tune_flag(VRS_TUNE_FUSED_PREFIX, &Tuning::fused_prefix),
    tune_check(VRS_TUNE_RANK_MODE, "rank mode must be 0 (auto), 1 (ballot) or 2 (atomic)", 0, kThreeWayMax),
    tune_u32(VRS_TUNE_ONE_CALL_MIN_KEYS, &Tuning::one_call_min_keys, "one-call threshold must be >= 0"),
    tune_flag(VRS_TUNE_DEBUG_MISPLACE_STREAMS, &Tuning::misplace),
    tune_u32(VRS_TUNE_LOOKBACK_SPIN_BUDGET, &Tuning::spin_budget, "spin budget must be >= 0"),
    tune_int(VRS_TUNE_DEBUG_HOLD_TILE, &Tuning::hold_tile, nullptr, INT_MIN, INT_MAX),
    tune_u32(VRS_TUNE_DIGIT_TABLE_GROUPS, &Tuning::groups, "digit table groups must be 0 (by size), 8, 16 or 32", 0, kGroupsMax, 1, tune_groups_ok),
    tune_u32(VRS_TUNE_SINGLE_MAX_KEYS, &Tuning::single_max_keys, "single-launch threshold must be >= 0"),
    tune_flag(VRS_TUNE_FUSED_PLAN, &Tuning::fused_plan),
    tune_flag(VRS_TUNE_HYBRID, &Tuning::hybrid),
    tune_u32(VRS_TUNE_HYBRID_MIN_KEYS, &Tuning::hybrid_min_keys, "hybrid threshold must be >= 0"),
    tune_int(VRS_TUNE_HYBRID_FAST_COUNT, &Tuning::fast_count, "fast count mode must be 0, 1 or 2", 0, kThreeWayMax),
    tune_flag(VRS_TUNE_ASYNC_SORT, &Tuning::async),
    tune_u32(VRS_TUNE_PLAN_WAIT_MS, &Tuning::plan_wait_ms, "the plan wait limit must be >= 0 ms"),
    tune_int(VRS_TUNE_MSD_RESERVE, &Tuning::reserve, "MSD reservation must be 0 (never) or 1 / 2 (bare keys of the hybrid form)", 0, kThreeWayMax),
    tune_int(VRS_TUNE_MSD_POOL, &Tuning::pool, "the pool form must be 0 (never), 1 (adaptive) or 2 (always tried)", 0, kThreeWayMax),
    tune_u32(VRS_TUNE_MSD_POOL_MIN_KEYS, &Tuning::pool_min_keys, "the pool form takes 2^22 keys or more", kPoolDefaultMinKeys),
    tune_check(VRS_TUNE_DEBUG_XCC_STRAY_BLOCK, "the probe has 4096 blocks (a negative value probes again without a stray one)", INT_MIN, kXccProbeBlocks - 1),
    tune_int(VRS_TUNE_MSD_POOL_SUB_BITS, &Tuning::pool_sub_bits, "the pool form's second pass sorts by 6, 7 or 8 bits (0 = by size)", 0, kPoolBitsMax,
             tune_sub_bits_ok),
    tune_check(VRS_TUNE_DEBUG_XCC_ROTATE, "rotate the probed placement by 0 .. 7 places", 0, kXccRotateMax),
    tune_flag(VRS_TUNE_MSD_POOL_REUSE_LAYOUT, &Tuning::pool_reuse),
    {VRS_TUNE_MSD_POOL_PAIRS, nullptr, nullptr, &Tuning::pool_pairs, true, INT_MIN, INT_MAX, 1, nullptr, nullptr},  // (the one as_01 row)
    tune_int(VRS_TUNE_MSD_POOL_TOP_BITS, &Tuning::pool_top_bits, "the pool form's first pass sorts by 6, 7 (the default) or 8 bits", kPoolBitsMin, kPoolBitsMax),
    tune_check(VRS_TUNE_DEBUG_POOL_NO_MEMORY, "allocations left to fail: 0 or more", 0, INT_MAX),
    tune_int(VRS_TUNE_MSD_POOL_PAIRS_PACKED, &Tuning::pool_pairs_packed, "the pairs' packed local sort: -1 (by size), 0 (never) or 1 (always)",
             kPoolPairsPackedDefault, kPoolPairsPackedMax),
    tune_u32(VRS_TUNE_SEGMENT_ONE_CALL_MIN_KEYS, &Tuning::seg_one_call_min_keys, "the segmented sorts' one-call threshold must be >= 0"),
    tune_u32(VRS_TUNE_TOPK_GRID_MIN_KEYS, &Tuning::topk_grid_min_keys, "the top-k grid tier's threshold must be >= 0"),
    tune_u32(VRS_TUNE_SEARCH_LDS_BYTES, &Tuning::search_lds_bytes, "the search's LDS capacity must be 0 .. 163840 bytes", 0, kSearchLdsMaxBytes),
    tune_u32(VRS_TUNE_SEARCH_TABLE_MIN_QUERIES, &Tuning::search_table_min_queries, "the search's table threshold must be >= 0"),
    tune_u32(VRS_TUNE_SEARCH_INDEX_MIN_QUERIES, &Tuning::search_index_min_queries, "the search's index threshold must be >= 0"),
    tune_u32(VRS_TUNE_BINCOUNT_LDS_BYTES, &Tuning::bincount_lds_bytes, "the counting kernels' LDS capacity must be 0 .. 163840 bytes", 0, kBinCountLdsMaxBytes),
    tune_u32(VRS_TUNE_SELECT_GRID_MIN_KEYS, &Tuning::select_grid_min_keys, "the selection's grid tier threshold must be >= 0"),
    tune_u32(VRS_TUNE_SELECT_COMPACT_DIVISOR, &Tuning::select_compact_divisor, "the selection's compaction divisor must be >= 0"),
    tune_u32(VRS_TUNE_REDUCE_CHUNK_ROWS, &Tuning::reduce_chunk_rows, "the reduction's chunk must be 64 .. 4096 rows", kReduceChunkMin, kReduceChunkMax),
    tune_u32(VRS_TUNE_REDUCE_LANE_ROWS, &Tuning::reduce_lane_rows, "the reduction's lane map takes 0 .. 64 rows", 0, kReduceLaneRowsMax),
    tune_u32(VRS_TUNE_SCAN_TILE_ROWS, &Tuning::scan_tile_rows, "the scan's tile must be a multiple of 256 in 256 .. 8192 rows", kScanTileMin, kScanTileMax, kScanTileMin),
    tune_u32(VRS_TUNE_SCAN_SINGLE_PASS_MIN_ROWS, &Tuning::scan_single_pass_min_rows, "the scan's single pass starts at 0 (never) or more rows"),
    tune_u32(VRS_TUNE_SCAN_SPIN_BUDGET, &Tuning::scan_spin_budget, "the scan's spin budget must be 0 .. 1048576 polls", 0, kScanSpinBudgetMax),
    tune_u32(VRS_TUNE_COMPACT_TILE_ELEMS, &Tuning::compact_tile_elems, "the compaction's tile must be a multiple of 4096 in 4096 .. 65536 elements",
             kCompactTileMin, kCompactTileMax, kCompactChunk),
};
constexpr int kTuneKeys = static_cast<int>(sizeof(kTuneTable) / sizeof(kTuneTable[0]));
constexpr bool tune_table_in_key_order() {
    for (int k = 0; k < kTuneKeys; ++k)
        if (kTuneTable[k].key != k) return false;
    return true;
}
static_assert(tune_table_in_key_order(), "kTuneTable[k] must be the row of the key whose value is k");

inline const TuneRow *tuning_row(int key) { return key >= 0 && key < kTuneKeys ? &kTuneTable[key] : nullptr; }

// nullptr: `value` is accepted for `key`; else what vrs_last_error says after the refusal
inline const char *tuning_refusal(int key, int value) {
    const TuneRow *r = tuning_row(key);
    if (!r) return "unknown tuning key";
    const bool ok = value >= r->min && value <= r->max && value % r->multiple == 0 && (!r->among || r->among(value));
    return ok ? nullptr : r->refusal;
}

// the row's store of an ACCEPTED value (nothing for a key without a member)
inline void tuning_store(Tuning &t, int key, int value) {
    const TuneRow &r = *tuning_row(key);
    if (r.flag) t.*r.flag = value != 0;
    if (r.u32) t.*r.u32 = static_cast<uint32_t>(value);
    if (r.i32) t.*r.i32 = r.as_01 ? (value != 0 ? 1 : 0) : value;
}

}  // namespace vrs
