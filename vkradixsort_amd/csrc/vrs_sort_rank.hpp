// vrs_sort_rank.hpp -- what the rank-in / restore-out kernels of the torch.sort drop-in (vrs_sort_rank.hip) and their host side
// (vrs_capi_sort_rank.hip) share: the dtypes, their widths, the rank map in torch's order and the launch wrappers.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vrs {

// vrs_sort_dtype (include/vkradixsort_amd_ops.h)
constexpr int kSortI8 = 0, kSortU8 = 1, kSortI16 = 2, kSortI32 = 3, kSortI64 = 4, kSortF16 = 5, kSortBF16 = 6, kSortF32 = 7, kSortF64 = 8;
constexpr int kSortDescending = 1;  // VRS_SORT_DESCENDING

__host__ __device__ inline bool sort_dtype_known(int dtype) { return dtype >= kSortI8 && dtype <= kSortF64; }
__host__ __device__ inline int sort_dtype_bytes(int dtype) {
    switch (dtype) {
        case kSortI8: case kSortU8: return 1;
        case kSortI16: case kSortF16: case kSortBF16: return 2;
        case kSortI64: case kSortF64: return 8;
        default: return 4;
    }
}
// ranks are uint32 for every dtype of up to 4 bytes (the narrow ones zero-extended), uint64 for int64 / float64
__host__ __device__ inline int sort_rank_bytes(int dtype) { return sort_dtype_bytes(dtype) == 8 ? 8 : 4; }
__host__ __device__ inline bool sort_dtype_float(int dtype) { return dtype >= kSortF16; }

// The rank of the B-bit pattern u (zero-extended to R) in torch's order: unsigned as is, signed with the sign bit flipped, floats by the
// IEEE-754 total order except that -0.0 takes +0.0's rank (`sign`) and every NaN the largest rank of B bits (`ones`), above +inf.
// Descending: the complement over all of R -- which changes no bit's variation within a segment.
template <typename R, int B, bool FLOAT, bool SIGNED>
__host__ __device__ inline R sort_rank(R u, R inf_bits, bool descending) {
    constexpr R sign = static_cast<R>(1) << (B - 1), ones = sign | (sign - 1);
    R r;
    if constexpr (FLOAT) {
        const R mag = u & (sign - 1);
        r = mag > inf_bits ? ones : mag == 0 ? sign : (u & sign) ? (~u & ones) : (u | sign);
    } else {
        r = SIGNED ? u ^ sign : u;
    }
    return descending ? ~r : r;
}

// The inverse for every rank but the two merged classes of a float (±0: `sign`, NaN: `ones`), which *exact = false reports: their bits
// come from the input.
template <typename R, int B, bool FLOAT, bool SIGNED>
__host__ __device__ inline R sort_unrank(R r, bool descending, bool *exact) {
    constexpr R sign = static_cast<R>(1) << (B - 1), ones = sign | (sign - 1);
    if (descending) r = ~r;
    *exact = true;
    if constexpr (FLOAT) {
        if (r == sign || r == ones) {
            *exact = false;
            return 0;
        }
        return (r & sign) ? (r ^ sign) : (~r & ones);
    } else {
        return SIGNED ? r ^ sign : r;
    }
}

// src: n elements of `dtype` as rows of row_len; ranks: n uint32 / uint64; positions: n uint32 (i mod row_len) or NULL
hipError_t launch_sort_rank(hipStream_t stream, const void *src, uint32_t n, uint32_t row_len, int dtype, bool descending, void *ranks,
                            uint32_t *positions);
// values: n elements of `dtype` or NULL; indices: n int64 or NULL; positions may be NULL only for integer dtypes without indices
hipError_t launch_sort_restore(hipStream_t stream, const void *src, const void *ranks, const uint32_t *positions, uint32_t n, uint32_t row_len,
                               int dtype, bool descending, void *values, int64_t *indices);

}  // namespace vrs
