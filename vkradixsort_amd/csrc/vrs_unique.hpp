// vrs_unique.hpp -- what the run-length encoding and unique kernels (vrs_unique.hip) and their host side (vrs_capi_unique.hip) share:
// the tile shape, the look-back status word, the rank maps, the scratch layouts and the launch wrappers.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "vrs_key_order.hpp"

namespace vrs {

constexpr uint32_t kRleThreads = 256u;                    // 4 waves
constexpr uint32_t kRleItems = 16u;                       // 64-key chunks per wave
constexpr uint32_t kRleTile = kRleThreads * kRleItems;    // 4096 keys per tile, either key width
constexpr uint32_t kRleSpinBudget = 4096u;                // polls of an unpublished status word before a tile counts that tile's heads itself
// look-back status word of a tile (64 bits, zeroed before every launch): bits 63:62 = 0 unpublished / 1 the tile's own head count /
// 2 the inclusive count of every head up to and including the tile; bits 31:0 = the count (R <= n < 2^32)
constexpr unsigned long long kRleAggregate = 1ull << 62, kRleInclusive = 2ull << 62;

constexpr int kUniqueU32 = 0, kUniqueI32 = 1, kUniqueF32 = 2, kUniqueU64 = 3, kUniqueI64 = 4, kUniqueF64 = 5;
constexpr int kUniqueInverse = 1, kUniqueCounts = 2;  // vrs_unique_scratch_bytes flags
constexpr int kRleCounts = 1;                         // vrs_run_length_encode_scratch_bytes flag

__host__ __device__ inline int unique_key_bytes(int key_type) { return key_type >= kUniqueU64 ? 8 : 4; }

// r(x): ascending r is ascending x (two's complement for I*, the IEEE-754 total order for F*, VRS_KEYS_FLOAT32_TO_SORTABLE widened)
__host__ __device__ inline uint32_t unique_rank(uint32_t x, int key_type) {
    return key_type == kUniqueI32 ? key_from_signed(x) : key_type == kUniqueF32 ? key_from_float(x) : x;
}
__host__ __device__ inline uint32_t unique_unrank(uint32_t r, int key_type) {
    return key_type == kUniqueI32 ? signed_from_key(r) : key_type == kUniqueF32 ? float_from_key(r) : r;
}
__host__ __device__ inline uint64_t unique_rank(uint64_t x, int key_type) {
    return key_type == kUniqueI64 ? key_from_signed(x) : key_type == kUniqueF64 ? key_from_float(x) : x;
}
__host__ __device__ inline uint64_t unique_unrank(uint64_t r, int key_type) {
    return key_type == kUniqueI64 ? signed_from_key(r) : key_type == kUniqueF64 ? float_from_key(r) : r;
}

inline size_t rle_up(size_t x) { return (x + 255u) & ~static_cast<size_t>(255u); }
__host__ __device__ inline uint32_t rle_tiles(uint32_t n) { return static_cast<uint32_t>((static_cast<uint64_t>(n) + kRleTile - 1u) / kRleTile); }
// the status block at the head of either scratch layout: the tile ticket (16 bytes) and one status word per tile, one memset
inline size_t rle_status_bytes(uint32_t n) { return rle_up(16u + 8u * static_cast<size_t>(rle_tiles(n))); }

// vrs_run_length_encode's scratch: the status block, then (kRleCounts) the run offsets for a caller who wants counts but no offsets
struct RleLayout {
    size_t status, offsets, bytes;  // offsets == bytes: no offsets area
};
inline RleLayout rle_layout(uint32_t n, int flags) {
    RleLayout L{};
    if (n == 0u) return L;
    L.status = 0;
    L.offsets = rle_status_bytes(n);
    L.bytes = L.offsets + ((flags & kRleCounts) ? rle_up((static_cast<size_t>(n) + 1u) * 4u) : 0u);
    return L;
}

// vrs_unique's scratch: the status block, the mapped keys and the sort's partner buffer, (inverse) the iota payloads and their partner,
// (counts) the run offsets
struct UniqueLayout {
    size_t status, keys, keys_tmp, vals, vals_tmp, offsets, bytes;
};
inline UniqueLayout unique_layout(uint32_t n, int key_type, int flags) {
    UniqueLayout L{};
    if (n == 0u) return L;
    const size_t kb = static_cast<size_t>(n) * unique_key_bytes(key_type), vb = static_cast<size_t>(n) * 4u;
    size_t at = rle_status_bytes(n);
    L.keys = at;
    at += rle_up(kb);
    L.keys_tmp = at;
    at += rle_up(kb);
    L.vals = L.vals_tmp = at;
    if (flags & kUniqueInverse) {
        L.vals_tmp = at + rle_up(vb);
        at += 2u * rle_up(vb);
    }
    L.offsets = at;
    if (flags & kUniqueCounts) at += rle_up((static_cast<size_t>(n) + 1u) * 4u);
    L.bytes = at;
    return L;
}

struct RleArgs {
    const void *keys;     // n keys of key_bytes each (vrs_unique: the sorted ranks)
    uint32_t n;
    int key_bytes;
    int key_type;         // unique: the rank map out_keys undoes; -1: run-length encoding (keys written as read)
    const uint32_t *idx;  // unique with an inverse: the sorted iota payloads (out_run_ids[idx[i]] = run of i); else null
    void *out_keys;       // R keys, or null
    uint32_t *out_offsets;  // R + 1, or null (the counts read it: the scratch's area when the caller wants counts but no offsets)
    uint32_t *out_counts;   // R, or null
    uint32_t *out_run_ids;  // n, or null
    uint32_t *out_num_runs;  // 1
    char *status;         // rle_status_bytes(n) bytes, zeroed by the launch
};

// the encode (one pass over the keys, decoupled look-back across tiles) and, with out_counts, the counts from the offsets; n > 0
hipError_t launch_rle(hipStream_t stream, const RleArgs &a);
// counts[j] = offsets[j + 1] - offsets[j] for j < R (a.out_offsets, a.out_num_runs, a.out_counts; the grid from a.n)
hipError_t launch_rle_counts(hipStream_t stream, const RleArgs &a);
// vrs_unique: keys -> rank-mapped keys in `mapped`, iota payloads in `vals` (null: none); n > 0
hipError_t launch_unique_map(hipStream_t stream, const void *keys, uint32_t n, int key_type, void *mapped, uint32_t *vals);

}  // namespace vrs
