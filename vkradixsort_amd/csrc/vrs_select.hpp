// vrs_select.hpp -- what the one-rank selection's kernels (vrs_select.hip) and their host side (vrs_capi_select.hip) share: the tier of a
// segment (exported as vrs_select_tier_for; the clamp is top-k's), the target rule (vrs_select_target_for), the levels' digits, the rank
// map (vrs_sort_rank.hpp's, cut to the dtype's bits), the scratch layout and the launch wrapper.  Internal.
#pragma once
#include <algorithm>

#include "vrs_sort_rank.hpp"
#include "vrs_topk.hpp"

namespace vrs {

constexpr uint32_t kSelLdsBytes = 32768u;                  // the LDS tier's ranks: 8192 of up to 4 bytes, 4096 of 8 bytes
constexpr uint32_t kSelDefaultGridMinKeys = 1u << 17;      // VRS_TUNE_SELECT_GRID_MIN_KEYS default: top-k's crossover, not measured here (DESIGN "K12")
constexpr uint32_t kSelDefaultCompactDivisor = 16u;        // VRS_TUNE_SELECT_COMPACT_DIVISOR default (not measured either)
// (the multi-rank selection, vrs_quantile.hpp, reads both keys too: the same tiers, and its sieve counts the keys of all live groups)
constexpr uint32_t kSelAreaPerTile = kTopkTile / 16u;      // ranks of the compacted area per 16384-key tile of a grid slot
constexpr uint32_t kSelSlotFloor = 8192u;                  // a grid slot is longer than this whatever the width: n / 8193 slots at the most
constexpr int kSelKth = 0, kSelMedian = 1, kSelNanMedian = 2;  // vrs_select_mode
constexpr int kSelDescending = 1;                              // VRS_SELECT_DESCENDING
constexpr int kSelUnsigned = 0, kSelSigned = 1, kSelFloat = 2;  // how a dtype's bits rank
constexpr uint32_t kSelNoShift = 0xFFu;                    // SelState::shift before the first level: every key matches

__host__ __device__ inline uint32_t select_lds_cap(int dtype) { return kSelLdsBytes / static_cast<uint32_t>(sort_rank_bytes(dtype)); }
__host__ __device__ inline int select_kind(int dtype) { return sort_dtype_float(dtype) ? kSelFloat : dtype == kSortU8 ? kSelUnsigned : kSelSigned; }
__host__ __device__ inline int select_levels(int bits) { return (bits + 10) / 11; }

// the digit of level `level` (0 = the top one) of a rank of `bits` significant bits: at most 11 bits, taken from the top
// (8: 8 | 16: 11, 5 | 32: 11, 11, 10 | 64: 11 x 5, 9)
__host__ __device__ inline void select_level(int bits, int level, uint32_t *shift, uint32_t *mask) {
    const int left = bits - 11 * level;  // bits not yet consumed
    const int width = left >= 11 ? 11 : left;
    *shift = static_cast<uint32_t>(left - width);
    *mask = (1u << width) - 1u;
}

// [cb, ce) clamped exactly as top-k (and the segmented sorts) clamp, and its tier.  grid_min_keys == 0: never the grid tier.
__host__ __device__ inline int select_tier(uint32_t b, uint32_t e, uint32_t n, int dtype, uint32_t grid_min_keys, uint32_t *cb, uint32_t *ce) {
    (void)topk_tier(b, e, n, 0u, cb, ce);
    const uint32_t len = *ce - *cb;
    if (len <= select_lds_cap(dtype)) return kTopkTierLds;
    if (grid_min_keys != 0u && len >= grid_min_keys) return kTopkTierGrid;
    return kTopkTierBlock;
}

// Which entry j (0-based) of the segment's stable ascending order of r a mode asks for; false: none (the segment gets 0xFFFFFFFF).
// nans: keys of the NaN class (the largest rank; the smallest when descending) -- MEDIAN: a segment with any NaN answers its first NaN;
// NANMEDIAN: the lower median of the other keys, the first NaN when there are no others.
__host__ __device__ inline bool select_target(int mode, uint32_t k, uint32_t len, uint32_t nans, bool descending, uint32_t *j) {
    *j = 0u;
    if (len == 0u) return false;
    if (mode == kSelKth) {
        if (k == 0u || k > len) return false;
        *j = k - 1u;
        return true;
    }
    const uint32_t first_nan = descending ? 0u : len - nans, first_other = descending ? nans : 0u;
    if (mode == kSelMedian) *j = nans == 0u ? (len - 1u) / 2u : first_nan;
    else *j = nans < len ? first_other + (len - nans - 1u) / 2u : first_nan;
    return true;
}

// r(x) cut to the B bits that vary: sort_rank's map (its complement when descending sets the bits above B of a narrow dtype)
template <typename R, int B>
__host__ __device__ inline R select_rank(R u, int kind, R inf_bits, bool descending) {
    constexpr R sign = static_cast<R>(1) << (B - 1), ones = sign | (sign - 1);
    const R r = kind == kSelFloat    ? sort_rank<R, B, true, false>(u, inf_bits, descending)
                : kind == kSelSigned ? sort_rank<R, B, false, true>(u, inf_bits, descending)
                                     : sort_rank<R, B, false, false>(u, inf_bits, descending);
    return r & ones;
}

// How far the selection of one segment has got: the answer is the need-th key in index order among those whose bits from `shift` up
// equal prefix's.  R: uint32_t or uint64_t.
template <typename R>
struct SelState {
    R prefix;
    uint32_t shift, need, done;
};

// one grid-tier segment of a call (the prefix is kept in 64 bits for both rank widths)
struct SelSlot {
    uint32_t seg, b, len, tile_base;
    uint32_t tiles, valid, ok, nans;  // ok: the mode has a target in this segment; nans: counted by the first level's walk
    uint32_t state, ccount, cursor;   // 0: streams src | 1: compacts after this level | 2: compacted before; ranks in its area; the copy's cursor
    uint32_t shift, need, done;
    unsigned long long prefix;
};
static_assert(sizeof(SelSlot) == 64, "one slot per 64 bytes");

// the scratch buffer's layout for (n, S, dtype): the same function sizes it (vrs_select_scratch_bytes) and cuts it (the call)
struct SelLayout {
    size_t control, slots, hist, tiles, list, area, bytes;
    uint32_t slot_cap, tile_cap;
};
inline SelLayout select_layout(uint32_t n, uint32_t num_segments, int dtype) {
    auto up = [](size_t x) { return (x + 255u) & ~static_cast<size_t>(255u); };
    SelLayout L{};
    L.slot_cap = std::min(std::min(num_segments, n / (kSelSlotFloor + 1u)), kTopkMaxSlots);
    L.tile_cap = L.slot_cap ? n / kTopkTile + L.slot_cap : 0u;
    size_t at = 0;
    L.control = at;
    at += up(sizeof(TopkControl));
    L.slots = at;
    at += up(static_cast<size_t>(L.slot_cap) * sizeof(SelSlot));
    L.hist = at;
    at += up(static_cast<size_t>(L.slot_cap) * kTopkBins * 4u);
    L.tiles = at;
    at += up(static_cast<size_t>(L.tile_cap) * 4u);
    L.list = at;
    at += up(static_cast<size_t>(num_segments) * 4u);
    L.area = at;  // kSelAreaPerTile ranks per tile: slot s owns those of its tiles
    at += up(static_cast<size_t>(L.tile_cap) * kSelAreaPerTile * static_cast<size_t>(sort_rank_bytes(dtype)));
    L.bytes = at;
    return L;
}

struct SelectArgs {
    const void *src;
    const uint32_t *offsets;
    uint32_t n, num_segments, k, grid_min_keys, compact_divisor;
    int dtype, mode, flags;
    void *out_values;
    uint32_t *out_indices;  // may be null
    char *scratch;
    unsigned long long *stats;  // [4] cumulative segments per tier, and grid slots that compacted (the context's)
};

hipError_t launch_select(hipStream_t stream, const SelectArgs &a, const SelLayout &L);

}  // namespace vrs
