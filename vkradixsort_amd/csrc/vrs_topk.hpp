// vrs_topk.hpp -- what the top-k selection's kernels (vrs_topk.hip) and their host side (vrs_capi_topk.hip) share: the classification of a
// segment (exported as vrs_topk_tier_for; the clamp is segment_tier's), the rank map, the selection state, the scratch layout and the launch
// wrapper.  Internal.
#pragma once
#include <algorithm>

#include "vrs_key_order.hpp"
#include "vrs_segmented.hpp"

namespace vrs {

constexpr uint32_t kTopkLdsCap = 8192u;            // longest segment of the LDS tier: one 256-thread workgroup holds its ranks in LDS (32 KB)
constexpr uint32_t kTopkDefaultGridMinKeys = 1u << 17;  // VRS_TUNE_TOPK_GRID_MIN_KEYS default (DESIGN "K7": the crossover of the two streaming tiers)
constexpr uint32_t kTopkSortCap = 4096u;           // VRS_TOPK_SORTED up to this k: the survivors are sorted in LDS by topk_sort_small
constexpr uint32_t kTopkTile = 16384u;             // keys per tile of the BLOCK and GRID tiers (1024 threads x 16)
constexpr uint32_t kTopkMaxSlots = 4096u;          // grid-tier segments per call; more (only overlapping ranges reach it) take the BLOCK kernel
constexpr uint32_t kTopkBins = 2048u;
constexpr int kTopkLevels = 3;                     // digits of 11, 11 and 10 bits from the top
constexpr int kTopkTierLds = 0, kTopkTierBlock = 1, kTopkTierGrid = 2;
constexpr int kTopkU32 = 0, kTopkI32 = 1, kTopkF32 = 2;
constexpr int kTopkLargest = 1, kTopkSorted = 2;

__host__ __device__ inline uint32_t topk_level_shift(int level) { return level == 0 ? 21u : level == 1 ? 10u : 0u; }
__host__ __device__ inline uint32_t topk_level_mask(int level) { return level == 2 ? 1023u : 2047u; }

// [cb, ce) clamped exactly as the segmented sorts clamp, and its tier.  grid_min_keys == 0: never the grid tier.
__host__ __device__ inline int topk_tier(uint32_t b, uint32_t e, uint32_t n, uint32_t grid_min_keys, uint32_t *cb, uint32_t *ce) {
    (void)segment_tier(b, e, n, false, 0u, cb, ce);
    const uint32_t len = *ce - *cb;
    if (len <= kTopkLdsCap) return kTopkTierLds;
    if (grid_min_keys != 0u && len >= grid_min_keys) return kTopkTierGrid;
    return kTopkTierBlock;
}

// r(x): ascending r is the order the selection takes the keys in (VRS_KEYS_FLOAT32_TO_SORTABLE for floats; ~ for the largest)
__host__ __device__ inline uint32_t topk_rank(uint32_t x, int key_type, bool largest) {
    const uint32_t r = key_type == kTopkI32 ? key_from_signed(x) : key_type == kTopkF32 ? key_from_float(x) : x;
    return largest ? ~r : r;
}
__host__ __device__ inline uint32_t topk_unrank(uint32_t r, int key_type, bool largest) {
    if (largest) r = ~r;
    return key_type == kTopkI32 ? signed_from_key(r) : key_type == kTopkF32 ? float_from_key(r) : r;
}

// How far the selection of one segment has got: the selected set is every key whose top (32 - shift) bits of r are below prefix's, then
// the first `need` keys in index order whose top bits equal prefix's.  shift == 32: nothing fixed yet (every key matches).
struct TopkSel {
    uint32_t prefix, shift, lt, need, done;
};
__host__ __device__ inline TopkSel topk_sel_init(uint32_t len, uint32_t m) {
    return TopkSel{0u, 32u, 0u, m, m == len ? 1u : 0u};  // k >= L: every key, nothing to select
}

// one grid-tier segment of a call
struct TopkSlot {
    uint32_t seg, b, len, m;
    uint32_t tile_base, tiles, valid, pad;
    TopkSel sel;
    uint32_t pad2[3];
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
    bool big_sort;  // VRS_TOPK_SORTED with k > kTopkSortCap: the survivors go through vrs_sort_segments_pairs_u32 in the sort area
};
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
        L.sort = at;
        L.list = at + sk * 4u;
        at += sk * 16u;
    } else {
        L.list = at;
        at += up(static_cast<size_t>(num_segments) * 4u);
        L.sort = at;
    }
    L.bytes = at;
    return L;
}

struct TopkArgs {
    const uint32_t *keys;
    const uint32_t *offsets;
    uint32_t n, num_segments, k, grid_min_keys;
    int key_type, flags;
    uint32_t *out_keys, *out_indices;  // out_indices may be null
    char *scratch;
    unsigned long long *stats;  // [3] cumulative segments per tier (the context's)
};

// everything up to the emitted (unsorted) result; then, with VRS_TOPK_SORTED and k <= kTopkSortCap, the sort of every segment's survivors
hipError_t launch_topk(hipStream_t stream, const TopkArgs &a, const TopkLayout &L);
// VRS_TOPK_SORTED with k > kTopkSortCap: the survivors' ranks and positions into the sort area, the sort's offsets into out_keys (before)
// and the sorted ranks back as keys (after vrs_sort_segments_*)
hipError_t launch_topk_sort_prep(hipStream_t stream, const TopkArgs &a, const TopkLayout &L);
hipError_t launch_topk_sort_back(hipStream_t stream, const TopkArgs &a, const TopkLayout &L);

}  // namespace vrs
