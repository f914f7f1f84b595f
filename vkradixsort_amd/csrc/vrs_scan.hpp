// vrs_scan.hpp -- what the prefix scan's kernels (vrs_scan.hip) and their host side (vrs_capi_scan.hip) share: the scratch layout and the
// launch wrapper.  The order itself: vrs_scan_order.hpp.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include "vrs_scan_order.hpp"

namespace vrs {

// The scratch buffer's layout for (S, L, C, accumulator, T, tier): the same function sizes it (vrs_scan_scratch_bytes) and cuts it.
//   tile tier:     nothing
//   three launch:  A(k) for every level (S x words(k) x C accumulators), then P (S x tiles x C)
//   single pass:   the ticket, then one 64-bit status word per A(k)_m (S x words(k))
struct ScanLayout {
    size_t ticket, level[kScanMaxLevels], prefix, bytes;  // byte offsets
    uint32_t words[kScanMaxLevels], tiles, levels;
};
inline ScanLayout scan_layout(uint32_t S, uint32_t L, uint32_t C, int out_dtype, int op, uint32_t T, int tier) {
    auto up = [](size_t x) { return (x + 255u) & ~static_cast<size_t>(255u); };
    ScanLayout l{};
    l.tiles = scan_tiles(L, T);
    l.levels = scan_levels(L, T);
    if (tier == kScanTierTile || S == 0u || L == 0u) return l;
    const size_t each = tier == kScanTierSinglePass ? 8u : static_cast<size_t>(C) * scan_acc_bytes(out_dtype, op);
    size_t at = 0;
    if (tier == kScanTierSinglePass) at += 256u;  // (the ticket at offset 0)
    for (uint32_t k = 0; k < l.levels; ++k) {
        l.words[k] = scan_level_words(l.tiles, k);
        l.level[k] = at;
        at += up(static_cast<size_t>(S) * l.words[k] * each);
    }
    if (tier == kScanTierThreeLaunch) {
        l.prefix = at;
        at += up(static_cast<size_t>(S) * l.tiles * each);
    }
    l.bytes = at;
    return l;
}

struct ScanArgs {
    const void *values;  // [S, L, C] of dtype
    void *out;           // [S, L, C] of out_dtype
    int64_t *indices;    // [S, L, C] for MAX and MIN
    char *scratch;
    uint32_t S, L, C, T;
    int dtype, out_dtype, op, tier;
    uint32_t spin_budget;
    unsigned long long *takeovers;  // the context's counter of words a waiting wave computed itself
};

hipError_t launch_scan_rows(hipStream_t stream, const ScanArgs &a, const ScanLayout &l, uint32_t compute_units);

}  // namespace vrs
