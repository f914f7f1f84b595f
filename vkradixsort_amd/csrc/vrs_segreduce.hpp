// vrs_segreduce.hpp -- what the segmented reduction's kernels (vrs_segreduce.hip) and their host side (vrs_capi_segreduce.hip) share: the
// control block, the work items, the scratch layout with its bounds and the launch wrapper.  The order itself: vrs_reduce_order.hpp.  Internal.
#pragma once
#include <algorithm>

#include "vrs_reduce_order.hpp"

namespace vrs {

// what the classify kernel counts (zero on entry)
struct ReduceControl {
    uint32_t lane_count, fail_count;         // the lane list grows from the front of `list`, the segments that found no room from its back
    uint32_t item_count[kReduceMaxLevels];   // chunk items reserved per level (may pass the level's capacity: readers clamp)
    uint32_t part_rows[kReduceMaxLevels];    // partial rows reserved in the buffer level k reads (k >= 1)
};

// one chunk: rows [src, src + len) of what its level reads, reduced into row `dst` of the next level's partials, or -- final -- into
// segment dst's row of `out`
struct ReduceItem {
    uint32_t src, len_final, dst, unused;    // len_final: len | final << 31
};
static_assert(sizeof(ReduceItem) == 16, "one item per 16 bytes");
constexpr uint32_t kReduceItemFinal = 0x80000000u;

// The scratch buffer's layout for (n, C, S, dtype, CH): the same function sizes it (vrs_segment_reduce_scratch_bytes) and cuts it (the
// call).  With segments that do not overlap, level k reads rows[k] rows at the most (rows[0] = n), of which at most rows[k] / (CH + 1)
// segments are longer than a chunk; every segment present at a level takes one item, and one more per CH rows:
//     items[k] <= rows[k] / CH + present[k],   rows[k + 1] <= rows[k] / CH + long[k],   present[k + 1] = long[k] = min(present[k], rows[k] / (CH + 1))
// Every term is a floor of something that grows with n, so the bound never shrinks as n grows.
struct ReduceLayout {
    size_t control, list, items[kReduceMaxLevels], parts[kReduceMaxLevels], bytes;  // byte offsets (parts[0] is unused)
    uint32_t levels, item_cap[kReduceMaxLevels], part_cap[kReduceMaxLevels];
};
inline ReduceLayout reduce_layout(uint32_t n, uint32_t C, uint32_t num_segments, int dtype, uint32_t CH) {
    auto up = [](size_t x) { return (x + 255u) & ~static_cast<size_t>(255u); };
    const size_t acc_bytes = sort_dtype_bytes(dtype) == 8 ? 8u : 4u;
    ReduceLayout L{};
    L.levels = reduce_levels(n, CH);
    size_t at = 0;
    L.control = at;
    at += up(sizeof(ReduceControl));
    L.list = at;
    at += up(static_cast<size_t>(num_segments) * 4u);
    uint64_t rows = n, present = num_segments;
    for (uint32_t k = 0; k < L.levels; ++k) {
        L.part_cap[k] = static_cast<uint32_t>(rows);  // (rows[1] <= 2 n / CH: 32 bits hold it)
        if (k != 0u) {
            L.parts[k] = at;
            at += up(static_cast<size_t>(rows) * C * acc_bytes);
        }
        L.item_cap[k] = static_cast<uint32_t>(std::min<uint64_t>(rows / CH + present + 1u, 0xFFFFFFFFull));
        L.items[k] = at;
        at += up(static_cast<size_t>(L.item_cap[k]) * sizeof(ReduceItem));
        const uint64_t longer = std::min<uint64_t>(present, rows / (CH + 1u));
        rows = rows / CH + longer;
        present = longer;
    }
    L.bytes = at;
    return L;
}

struct SegReduceArgs {
    const void *values;       // n rows of C elements of the dtype
    const uint32_t *order;    // NULL, or n row numbers: reduction row i is values row order[i] (an entry beyond n - 1 reads row n - 1)
    const uint32_t *offsets;  // num_segments + 1
    const void *init;         // NULL, or num_segments rows
    void *out;                // num_segments rows
    char *scratch;
    uint32_t n, C, num_segments, chunk_rows, lane_rows;
    int dtype, op;
    unsigned long long *stats;  // [4] cumulative chunks per map and the deepest level count (the context's)
};

hipError_t launch_segment_reduce(hipStream_t stream, const SegReduceArgs &a, const ReduceLayout &L, uint32_t compute_units);

}  // namespace vrs
