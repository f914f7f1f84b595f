// vrs_segmented.hpp -- what the segmented sorts' kernels (vrs_segmented.hip) and their host side (vrs_capi_segmented.hip) share: the
// classification of a segment (the same function on both sides, exported as vrs_segment_tier_for), the work lists the classifying
// kernel fills, and the launch wrappers.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vrs {

// capacities of the LDS tiers: those of the hybrid form's local sorts (vrs_msd_hybrid.hip: kWaveCap, kLeanBigCap, kLocalCapBig)
constexpr uint32_t kSegWaveCap = 1789u;
constexpr uint32_t kSegBlockCapKeys = 14333u;
constexpr uint32_t kSegBlockCapPairs = 13312u;
constexpr uint32_t kSegDefaultOneCallMinKeys = 1u << 20;
// 64-bit keys (vrs_sort_segments_u64 / _pairs_u64): the block tier takes the capacities of the hybrid form's 64-bit local sorts
// (vrs_msd_hybrid.hip: kLocalCapBig, kLocalCapPairsU64), the wave tier the 32-bit one's register bytes at 8 bytes per key (64 x 14)
constexpr uint32_t kSegWaveCapU64 = 896u;
constexpr uint32_t kSegBlockCapKeysU64 = 13312u;
constexpr uint32_t kSegBlockCapPairsU64 = 6656u;

__host__ __device__ inline uint32_t seg_wave_cap(bool wide) { return wide ? kSegWaveCapU64 : kSegWaveCap; }
__host__ __device__ inline uint32_t seg_block_cap(bool wide, bool pairs) {
    return wide ? (pairs ? kSegBlockCapPairsU64 : kSegBlockCapKeysU64) : (pairs ? kSegBlockCapPairs : kSegBlockCapKeys);
}

// public tiers (vrs_segment_tier_for's *tier, the four statistics counters)
constexpr int kSegTierWave = 0, kSegTierBlock = 1, kSegTierGlobal = 2, kSegTierOneCall = 3;

// The work lists: a public tier is split by length into the workgroup shapes that sort it.
enum SegList : int {
    kSegListWaveSmall = 0,  // 2 .. 256: one wave, 4 keys per lane
    kSegListWave = 1,       // .. 1789: one wave, 28 keys per lane (64-bit: .. 896, 14 per lane)
    kSegListBlockSmall = 2, // .. 4096: 256 threads x 16
    kSegListBlock = 3,      // .. 14333 keys: 512 x 28 / 13312 pairs: 1024 x 13 (64-bit: 13312 keys: 1024 x 13 / 6656 pairs: 512 x 13)
    kSegListGlobal = 4,     // one 1024-thread workgroup per segment, LSD through keys_tmp
    kSegListOneCall = 5,    // the host runs vrs_sort_keys_u32 / vrs_sort_pairs_u32 on views
    kSegLists = 6
};
constexpr uint32_t kSegWaveSmallCap = 256u, kSegBlockSmallCap = 4096u;

// [min(b, n), min(max(b, e), n)) and its tier.  one_call_min_keys == 0: never the one-call tier.  wide: 64-bit keys.
__host__ __device__ inline int segment_tier(uint32_t b, uint32_t e, uint32_t n, bool pairs, uint32_t one_call_min_keys, uint32_t *cb,
                                            uint32_t *ce, bool wide = false) {
    const uint32_t lo = b < n ? b : n;
    const uint32_t hi_raw = e > b ? e : b;
    const uint32_t hi = hi_raw < n ? hi_raw : n;
    *cb = lo;
    *ce = hi;
    const uint32_t len = hi - lo;
    if (len <= seg_wave_cap(wide)) return kSegTierWave;
    if (len <= seg_block_cap(wide, pairs)) return kSegTierBlock;
    if (one_call_min_keys != 0u && len >= one_call_min_keys) return kSegTierOneCall;
    return kSegTierGlobal;
}

// the list a segment of `len` keys of tier `tier` goes to; -1: nothing to sort (0 or 1 key)
__host__ __device__ inline int segment_list(int tier, uint32_t len) {
    if (len <= 1u) return -1;
    switch (tier) {
        case kSegTierWave: return len <= kSegWaveSmallCap ? kSegListWaveSmall : kSegListWave;
        case kSegTierBlock: return len <= kSegBlockSmallCap ? kSegListBlockSmall : kSegListBlock;
        case kSegTierGlobal: return kSegListGlobal;
        default: return kSegListOneCall;
    }
}

// device memory of a context's segmented sorts: counts[] is zeroed before every classification, stats[] only when it is made
struct SegControl {
    uint32_t count[8];
    unsigned long long stats[4];
};
struct SegLists {
    uint2 *list[kSegLists];  // (begin, end) of each segment, clamped
    uint32_t cap[kSegLists]; // entries each list holds: a count beyond it (overlapping malformed ranges) is cut to it
};

// keys / keys_tmp: uint32 (key_bytes 4) or uint64 (key_bytes 8) keys; values / values_tmp: uint32 payloads or NULL
hipError_t launch_segmented(hipStream_t stream, void *keys, void *keys_tmp, uint32_t *values, uint32_t *values_tmp, uint32_t n,
                            const uint32_t *offsets, uint32_t num_segments, uint32_t one_call_min_keys, SegControl *control,
                            const SegLists &lists, const uint32_t grid[kSegLists], uint32_t *host_list, uint32_t stamp, int key_bytes);

}  // namespace vrs
