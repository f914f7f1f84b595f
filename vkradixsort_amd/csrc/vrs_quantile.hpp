// vrs_quantile.hpp -- what the multi-rank selection's kernels (vrs_quantile.hip) and their host side (vrs_capi_quantile.hip) share: the
// level table (exported as vrs_quantile_level_for), the per-segment state of up to 16 targets, the scratch layout and the launch wrapper.
// The tiers, the clamp, the rank map and the grid bookkeeping are vrs_select.hpp's and vrs_topk.hpp's.  Internal.
#pragma once
#include "vrs_quantile_order.hpp"
#include "vrs_select.hpp"

namespace vrs {

constexpr uint32_t kQuantTopBits = 11u;   // level 0: one histogram of 2048 bins over every key (and the NaN count)
constexpr uint32_t kQuantSubBits = 8u;    // later levels: 256 bins per live group, 16 groups in 16 KB of LDS
constexpr uint32_t kQuantSubBins = 1u << kQuantSubBits;
constexpr uint32_t kQuantHistWords = kQuantMaxTargets * kQuantSubBins;  // 4096 words: also holds level 0's 2048 bins
static_assert(kQuantHistWords >= kTopkBins, "level 0's histogram lives where the groups' do");

// levels of a rank of `bits` bits (32: 11, 8, 8, 5 | 64: 11, 8 x 6, 5)
__host__ __device__ constexpr int quantile_levels(int bits) { return 1 + (bits - static_cast<int>(kQuantTopBits) + static_cast<int>(kQuantSubBits) - 1) / static_cast<int>(kQuantSubBits); }
// the digit of level `level` (0 = the top one): 11 bits, then 8 at a time, the last level what is left
__host__ __device__ inline void quantile_level(int bits, int level, uint32_t *shift, uint32_t *mask) {
    if (level == 0) {
        *shift = static_cast<uint32_t>(bits) - kQuantTopBits;
        *mask = (1u << kQuantTopBits) - 1u;
        return;
    }
    const int left = bits - static_cast<int>(kQuantTopBits) - static_cast<int>(kQuantSubBits) * (level - 1);  // bits not yet consumed
    const int width = left >= static_cast<int>(kQuantSubBits) ? static_cast<int>(kQuantSubBits) : left;
    *shift = static_cast<uint32_t>(left - width);
    *mask = (1u << width) - 1u;
}

// How far the selection of one segment has got.  Its M distinct target entries, ascending: target m is the need[m]-th smallest of the
// keys whose bits from `shift` up equal prefix[m]'s.  Targets with one prefix are one group (groups ascend with the targets):
// gprefix[g] is group g's prefix >> shift, what a key's r >> shift is compared with.
struct QuantState {
    uint32_t M, G, shift, live;  // live: keys the G groups hold together (what a sieve would copy)
    uint32_t entry[kQuantMaxTargets];  // the target entries themselves (what the outputs look their values up by)
    uint32_t need[kQuantMaxTargets];
    uint32_t group[kQuantMaxTargets];
    unsigned long long prefix[kQuantMaxTargets];
    unsigned long long gprefix[kQuantMaxTargets];
};

// one grid-tier segment of a call
struct QuantSlot {
    uint32_t seg, b, len, tile_base;
    uint32_t tiles, valid, ok, nans;  // ok: the segment has an answer (known after level 0); nans: counted by the first level's walk
    uint32_t state, ccount, cursor;   // 0: streams src | 1: sieves after this level | 2: sieved before; ranks in its area; the copy's cursor
    uint32_t pad;
    QuantState q;
};
static_assert(sizeof(QuantSlot) % 64 == 0, "slots keep 64-byte lines");

// the scratch buffer's layout for (n, S, dtype): the same function sizes it (vrs_quantile_scratch_bytes) and cuts it (the call)
struct QuantLayout {
    size_t control, slots, hist, list, area, bytes;
    uint32_t slot_cap, tile_cap;
};
inline QuantLayout quantile_layout(uint32_t n, uint32_t num_segments, int dtype) {
    auto up = [](size_t x) { return (x + 255u) & ~static_cast<size_t>(255u); };
    QuantLayout L{};
    L.slot_cap = std::min(std::min(num_segments, n / (kSelSlotFloor + 1u)), kTopkMaxSlots);
    L.tile_cap = L.slot_cap ? n / kTopkTile + L.slot_cap : 0u;
    size_t at = 0;
    L.control = at;
    at += up(sizeof(TopkControl));
    L.slots = at;
    at += up(static_cast<size_t>(L.slot_cap) * sizeof(QuantSlot));
    L.hist = at;
    at += up(static_cast<size_t>(L.slot_cap) * kQuantHistWords * 4u);
    L.list = at;
    at += up(static_cast<size_t>(num_segments) * 4u);
    L.area = at;  // kSelAreaPerTile ranks per tile: slot s owns those of its tiles
    at += up(static_cast<size_t>(L.tile_cap) * kSelAreaPerTile * static_cast<size_t>(sort_rank_bytes(dtype)));
    L.bytes = at;
    return L;
}

struct QuantileArgs {
    const void *src;
    const uint32_t *offsets;
    uint32_t n, num_segments, num_q, grid_min_keys, compact_divisor;
    int dtype, interpolation, flags;
    double q[kQuantMaxTargets];
    void *out_values, *out_lower, *out_upper, *out_weight;  // [num_segments, num_q] of dtype; all but out_values may be null
    char *scratch;
    unsigned long long *stats;  // [4] cumulative segments per tier, and grid slots that sieved (the context's)
};

hipError_t launch_quantile(hipStream_t stream, const QuantileArgs &a, const QuantLayout &L);

}  // namespace vrs
