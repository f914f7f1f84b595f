// vrs_bincount.hpp -- what the counting kernels (vrs_bincount.hip) and their host side (vrs_capi_bincount.hip) share: the modes, the
// tiers and the function that picks one (exported as vrs_bin_count_tier_for), the linear rule that turns a float into a bin (device
// and host: the same function), the scratch layout and the launch wrapper.  Internal.
#pragma once
#include <algorithm>

#include "vrs_sort_rank.hpp"

namespace vrs {

constexpr int kBinIndex = 0, kBinLinear = 1;                       // VRS_BIN_INDEX, VRS_BIN_LINEAR
constexpr int kBinCountTierLds = 0, kBinCountTierGlobal = 1, kBinCountTiers = 2;  // VRS_BINCOUNT_LDS, VRS_BINCOUNT_GLOBAL
constexpr int kBinNoWeights = -1;                                  // VRS_BIN_NO_WEIGHTS
constexpr uint32_t kBinNone = 0xFFFFFFFFu;                         // "this element has no bin" (num_bins < 2^32: never a bin)
constexpr uint32_t kBinCountThreads = 1024u, kBinCountLoadBytes = 16u;
constexpr uint32_t kBinCountTileBytes = kBinCountThreads * kBinCountLoadBytes;  // of elements, per workgroup and step of its loop
constexpr uint32_t kBinCountLdsMaxBytes = 160u * 1024u;            // what a workgroup can claim at all
constexpr uint32_t kBinCountDefaultLdsBytes = 64u * 1024u;         // VRS_TUNE_BINCOUNT_LDS_BYTES: a first setting (two workgroups per CU), not a measured one

__host__ __device__ inline bool bin_index_dtype(int dtype) { return dtype >= kSortI8 && dtype <= kSortI64; }
__host__ __device__ inline bool bin_linear_dtype(int dtype) { return dtype >= kSortF16 && dtype <= kSortF64; }
__host__ __device__ inline bool bin_weight_dtype(int dtype) { return dtype == kSortF32 || dtype == kSortF64; }
__host__ __device__ inline bool bin_count_out_dtype(int dtype) { return dtype == kSortI64 || bin_linear_dtype(dtype); }
// bytes of one counter: 4 for counts and float32 weights, 8 for float64 weights
__host__ __device__ inline uint32_t bin_counter_bytes(int weight_dtype) { return weight_dtype == kSortF64 ? 8u : 4u; }

// The tier of a call: the counters of every bin fit lds_bytes (0: never), or they are the accumulation buffer itself.
__host__ __device__ inline int bin_count_tier(uint32_t num_bins, uint32_t counter_bytes, uint32_t lds_bytes) {
    return static_cast<uint64_t>(num_bins) * counter_bytes <= std::min(lds_bytes, kBinCountLdsMaxBytes) ? kBinCountTierLds : kBinCountTierGlobal;
}

// The 16 bits of a float16 / bfloat16 as the float32 of the same value.
__host__ __device__ inline float bin_widen_f16(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<float>(__builtin_bit_cast(_Float16, h));
#else
    const uint32_t sign = static_cast<uint32_t>(h & 0x8000u) << 16, exp = (h >> 10) & 0x1Fu, man = h & 0x3FFu;
    uint32_t u;
    if (exp == 0x1Fu) {
        u = sign | 0x7F800000u | (man << 13);
    } else if (exp != 0u) {
        u = sign | ((exp + 112u) << 23) | (man << 13);
    } else {  // zero or subnormal: man * 2^-24, exact in float32
        const float f = static_cast<float>(man) * 5.9604644775390625e-8f;
        u = sign | __builtin_bit_cast(uint32_t, f);
    }
    return __builtin_bit_cast(float, u);
#endif
}
__host__ __device__ inline float bin_widen_bf16(uint16_t h) { return __builtin_bit_cast(float, static_cast<uint32_t>(h) << 16); }

// THE linear rule (torch.histc's): bin = (int)((x - lo) * num_bins / (hi - lo)) in F, the three operations in this order, each rounded
// on its own; bin == num_bins becomes num_bins - 1; x < lo, x > hi and NaN have no bin.  (A quotient that rounding carries beyond
// num_bins is clamped too: the result is below num_bins whatever the range.)  *side: -1 for x < lo, +1 for x > hi, 0 otherwise.
// The entry points refuse a range whose width hi - lo is not finite in F (lo = -3e38, hi = 3e38 in float32): q would be 0 or NaN for
// every element.
template <typename F>
__host__ __device__ inline uint32_t bin_linear(F x, F lo, F hi, uint32_t num_bins, int *side) {
    *side = x < lo ? -1 : x > hi ? 1 : 0;
    if (!(x >= lo && x <= hi)) return kBinNone;
    const F moved = x - lo;
    const F scaled = moved * static_cast<F>(num_bins);
    const F q = scaled / (hi - lo);
    if (!(q < static_cast<F>(4294967296.0))) return num_bins - 1u;  // (a product that overflows F: inf, never converted)
    const unsigned long long bin = static_cast<unsigned long long>(q);  // (0 <= q < 2^32)
    return bin >= num_bins ? num_bins - 1u : static_cast<uint32_t>(bin);
}

// A count as the float of `sig` significant bits nearest to it, ties to even (sig = 24: float32's own conversion); the result is
// exact in float32 for sig <= 24, so a narrowing conversion after it rounds nothing (beyond float16's range it gives inf, as it should).
__host__ __device__ inline float bin_count_rounded(uint32_t c, int sig) {
    if (c < (1u << sig)) return static_cast<float>(c);
    int top = 31;
    while (!(c >> top)) --top;
    const int shift = top + 1 - sig;
    uint32_t man = c >> shift;
    const uint32_t rem = c & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (man & 1u))) ++man;  // (man == 2^sig after the carry is exact as well)
    return static_cast<float>(man) * static_cast<float>(1ull << shift);
}

// the scratch buffer's layout: the same function sizes it (vrs_bin_count_scratch_bytes) and cuts it (the call).  The two skip counters
// first; behind them the 32-bit counters of a count whose output is not int64 (an int64 output and a weighted sum are accumulated in
// `out` itself).
struct BinCountLayout {
    size_t skip, counters, bytes;  // byte offsets
};
inline BinCountLayout bin_count_layout(uint32_t num_bins, int weight_dtype, int out_dtype) {
    BinCountLayout L{};
    L.skip = 0;
    L.counters = 256;
    L.bytes = 256;
    if (weight_dtype == kBinNoWeights && out_dtype != kSortI64) L.bytes += (static_cast<size_t>(num_bins) * 4u + 255u) & ~static_cast<size_t>(255u);
    return L;
}

struct BinCountArgs {
    const void *values;   // n elements of the dtype
    const void *weights;  // NULL, or n float32 / float64
    void *acc;            // the counters every workgroup adds to: uint32, float32 or float64, zero on entry; counter of bin b at acc[b * acc_stride]
    uint32_t *skip;       // two words, zero on entry: elements below the range, elements at or above its end
    uint32_t n, num_bins, acc_stride;
    int vec_ok;           // whole vectors may be loaded: element `shift` of the tiles below sits on a 16-byte boundary, in values and in weights
    uint32_t shift;       // the tiles cover positions [0, n + shift), element i at position i + shift: values starts `shift` elements (fewer
                          // than a vector holds) past a 16-byte boundary, and the leading positions are empty
    double lo, hi;        // linear mode
    uint32_t compute_units;
};

struct BinFinishArgs {
    const uint32_t *counters;  // NULL: nothing to convert
    void *out;
    int out_dtype;
    uint32_t num_bins;
    const uint32_t *skip;
    unsigned long long *skipped;  // NULL, or two words that take the skip counters
};

// the counting launch of one call in `tier` (lds_bytes: what the counters take there) / the conversion of its counters
hipError_t launch_bin_count(hipStream_t stream, const BinCountArgs &a, int dtype, int mode, int weight_dtype, int tier);
hipError_t launch_bin_finish(hipStream_t stream, const BinFinishArgs &a);
// workgroups launch_bin_count starts for n elements of the dtype in `tier` (what bounds the grid: the CUs, not n)
uint32_t bin_count_grid(uint32_t n, int dtype, uint32_t num_bins, int weight_dtype, int tier, uint32_t compute_units);

}  // namespace vrs
