// vrs_topk.hpp -- what the top-k selection's kernels (vrs_topk.hip) and their host side (vrs_capi_topk.hip) share: the classification of a
// segment (exported as vrs_topk_tier_for; the clamp is segment_tier's), the rank map, the selection state, the scratch layout and the launch
// wrapper.  Internal.
#pragma once
#include <algorithm>

#include "vrs_key_order.hpp"
#include "vrs_segmented.hpp"
#include "vrs_sort_rank.hpp"

namespace vrs {

constexpr uint32_t kTopkLdsCap = 8192u;            // longest segment of the LDS tier: one 256-thread workgroup holds its ranks in LDS (32 KB)
constexpr uint32_t kTopkDefaultGridMinKeys = 1u << 17;  // VRS_TUNE_TOPK_GRID_MIN_KEYS default (DESIGN "K7": the crossover of the two streaming tiers)
constexpr uint32_t kTopkSortCap = 4096u;           // VRS_TOPK_SORTED up to this k: the survivors are sorted in LDS by topk_sort_small
constexpr uint32_t kTopkTile = 16384u;             // keys per tile of the BLOCK and GRID tiers (1024 threads x 16)
constexpr uint32_t kTopkMaxSlots = 4096u;          // grid-tier segments per call; more (only overlapping ranges reach it) take the BLOCK kernel
constexpr uint32_t kTopkBins = 2048u;
constexpr uint32_t kTopkLdsBytes = 32768u;         // the LDS tier's ranks: 8192 of up to 4 bytes, 4096 of 8 bytes (the one-rank selection's too)
constexpr int kTopkTierLds = 0, kTopkTierBlock = 1, kTopkTierGrid = 2;
constexpr int kTopkU32 = 0, kTopkI32 = 1, kTopkF32 = 2;
constexpr int kTopkDtypeBase = 0x100;              // VRS_TOPK_DTYPE(d): key_type 0x100 | d, an element of vrs_sort_dtype d ranked in torch's order
constexpr int kTopkLargest = 1, kTopkSorted = 2, kTopkRank64 = 16;
constexpr uint32_t kTopkNoShift = 0xFFu;           // TopkSel::shift before the first level: every key matches

__host__ __device__ inline bool topk_key_type_known(int key_type) {
    return key_type == kTopkU32 || key_type == kTopkI32 || key_type == kTopkF32 ||
           ((key_type & ~0xFF) == kTopkDtypeBase && sort_dtype_known(key_type & 0xFF));
}
__host__ __device__ inline bool topk_key_type_torch(int key_type) { return (key_type & kTopkDtypeBase) != 0; }
// bytes of one element of `keys` and `out_keys`, of one rank, and the longest segment of the LDS tier (kTopkLdsBytes of ranks)
__host__ __device__ inline uint32_t topk_elem_bytes(int key_type) {
    return topk_key_type_torch(key_type) ? static_cast<uint32_t>(sort_dtype_bytes(key_type & 0xFF)) : 4u;
}
__host__ __device__ inline uint32_t topk_rank_bytes(int key_type) { return topk_elem_bytes(key_type) == 8u ? 8u : 4u; }
__host__ __device__ inline uint32_t topk_lds_cap(int key_type) { return kTopkLdsBytes / topk_rank_bytes(key_type); }

// [cb, ce) clamped exactly as the segmented sorts clamp, and its tier for an LDS tier of up to lds_cap keys.  grid_min_keys == 0: never
// the grid tier.
__host__ __device__ inline int topk_tier_cap(uint32_t b, uint32_t e, uint32_t n, uint32_t lds_cap, uint32_t grid_min_keys, uint32_t *cb,
                                             uint32_t *ce) {
    (void)segment_tier(b, e, n, false, 0u, cb, ce);
    const uint32_t len = *ce - *cb;
    if (len <= lds_cap) return kTopkTierLds;
    if (grid_min_keys != 0u && len >= grid_min_keys) return kTopkTierGrid;
    return kTopkTierBlock;
}
// the tier of the three 32-bit key types (vrs_topk_tier_for)
__host__ __device__ inline int topk_tier(uint32_t b, uint32_t e, uint32_t n, uint32_t grid_min_keys, uint32_t *cb, uint32_t *ce) {
    return topk_tier_cap(b, e, n, kTopkLdsCap, grid_min_keys, cb, ce);
}

// r(x) of the three 32-bit key types: ascending r is the order the selection takes the keys in (VRS_KEYS_FLOAT32_TO_SORTABLE for
// floats; ~ for the largest)
__host__ __device__ inline uint32_t topk_rank(uint32_t x, int key_type, bool largest) {
    const uint32_t r = key_type == kTopkI32 ? key_from_signed(x) : key_type == kTopkF32 ? key_from_float(x) : x;
    return largest ? ~r : r;
}
__host__ __device__ inline uint32_t topk_unrank(uint32_t r, int key_type, bool largest) {
    if (largest) r = ~r;
    return key_type == kTopkI32 ? signed_from_key(r) : key_type == kTopkF32 ? float_from_key(r) : r;
}

// How far the selection of one segment has got: the selected set is every key whose bits of r from `shift` up are below prefix's, then
// the first `need` keys in index order whose bits from there up equal prefix's.  shift == kTopkNoShift: nothing fixed yet (every key
// matches).  R: the rank's type, uint32_t or uint64_t.
template <typename R>
struct TopkSel {
    R prefix;
    uint32_t shift, lt, need, done;
};
template <typename R>
__host__ __device__ inline TopkSel<R> topk_sel_init(uint32_t len, uint32_t m) {
    return TopkSel<R>{static_cast<R>(0), kTopkNoShift, 0u, m, m == len ? 1u : 0u};  // k >= L: every key, nothing to select
}

// one grid-tier segment of a call (the selection's prefix is kept in 64 bits for both rank widths)
struct TopkSlot {
    uint32_t seg, b, len, m;
    uint32_t tile_base, tiles, valid, pad;
    TopkSel<unsigned long long> sel;
    uint32_t pad2[2];
};
static_assert(sizeof(TopkSlot) == 64, "one slot per 64 bytes");

// per-call counters at the head of the scratch buffer (zeroed by every call)
struct TopkControl {
    uint32_t lds_count, block_count;  // the LDS tier's list grows from the front of `list`, the BLOCK tier's from the back
    unsigned long long grid_packed;   // grid slots taken (low 32 bits) | tiles taken (high 32 bits)
};

// the scratch buffer's layout for (n, S, k, flags): the same function sizes it (vrs_topk_scratch_bytes) and cuts it (the call)
struct TopkLayout {
    size_t control, list, slots, hist, tiles, sort, bytes;  // byte offsets; sort == bytes: no sort area
    uint32_t slot_cap, tile_cap;
    bool big_sort;  // VRS_TOPK_SORTED with k > kTopkSortCap: the survivors go through vrs_sort_segments_pairs_u32 / _u64 in the sort area
};
// flags & kTopkRank64: the sort area holds 8-byte ranks
inline TopkLayout topk_layout(uint32_t n, uint32_t num_segments, uint32_t k, int flags) {
    auto up = [](size_t x) { return (x + 255u) & ~static_cast<size_t>(255u); };
    TopkLayout L{};
    L.slot_cap = std::min(std::min(num_segments, n / (kTopkLdsCap + 1u)), kTopkMaxSlots);
    L.tile_cap = L.slot_cap ? n / kTopkTile + L.slot_cap : 0u;
    L.big_sort = (flags & kTopkSorted) != 0 && k > kTopkSortCap;
    const size_t sk = static_cast<size_t>(num_segments) * k;
    size_t at = 0;
    L.control = at;
    at += up(sizeof(TopkControl));
    L.slots = at;
    at += up(static_cast<size_t>(L.slot_cap) * sizeof(TopkSlot));
    L.hist = at;
    at += up(static_cast<size_t>(L.slot_cap) * kTopkBins * 4u);
    L.tiles = at;
    at += up(static_cast<size_t>(L.tile_cap) * 8u);
    if (L.big_sort) {  // keys, keys_tmp, values, values_tmp of S * k entries; the list lives in keys_tmp until the sort needs it
        const size_t rb = (flags & kTopkRank64) != 0 ? 8u : 4u;
        L.sort = at;
        L.list = at + sk * rb;
        at += sk * (2u * rb + 8u);
    } else {
        L.list = at;
        at += up(static_cast<size_t>(num_segments) * 4u);
        L.sort = at;
    }
    L.bytes = at;
    return L;
}

struct TopkArgs {
    const void *keys;  // n elements of topk_elem_bytes(key_type) bytes
    const uint32_t *offsets;
    uint32_t n, num_segments, k, grid_min_keys;
    uint32_t lds_cap;  // topk_lds_cap(key_type)
    int key_type, flags;
    void *out_keys;         // num_segments * k elements of the keys' width
    uint32_t *out_indices;  // may be null
    uint32_t *positions;    // where the emission writes the positions: out_indices, or topk_sort_positions when the sort needs them and
                            // the call has none; null: nowhere
    char *scratch;
    unsigned long long *stats;  // [3] cumulative segments per tier (the context's)
};

// everything up to the emitted (unsorted) result; then, with VRS_TOPK_SORTED and k <= kTopkSortCap, the sort of every segment's survivors
hipError_t launch_topk(hipStream_t stream, const TopkArgs &a, const TopkLayout &L);
inline uint32_t *topk_sort_positions(const TopkArgs &a, const TopkLayout &L) {
    const size_t sk = static_cast<size_t>(a.num_segments) * a.k;
    return reinterpret_cast<uint32_t *>(a.scratch + L.sort + 2u * sk * topk_rank_bytes(a.key_type));
}
// VRS_TOPK_SORTED with k > kTopkSortCap: the survivors' ranks and positions into the sort area, the sort's offsets into out_keys (before)
// and the sorted ranks back as keys (after vrs_sort_segments_*).  VRS_TOPK_DTYPE: the emission writes the positions to `positions`
// (out_indices, or the sort area's values when that is null -- topk_sort_positions) and the keys come back as the own bits at them.
hipError_t launch_topk_sort_prep(hipStream_t stream, const TopkArgs &a, const TopkLayout &L);
hipError_t launch_topk_sort_back(hipStream_t stream, const TopkArgs &a, const TopkLayout &L);

}  // namespace vrs
