// vrs_sort_rank.hip -- the two streaming kernels around the torch.sort drop-in's segmented sort (vrs_sort_rank_keys / vrs_sort_restore).
//   sort_rank_kernel: one read of the input, one write of its ranks (sort_rank: torch's order, the complement when descending) and of
//     each element's position in its row -- the keys and payloads the stable segmented sort then takes.
//   sort_restore_kernel: one read of the sorted ranks (and positions), one write of the values (the inverse map) and of the int64
//     indices.  An element of a float's merged class (±0.0, NaN) cannot be inverted: it reads its exact bits from the input at
//     row * row_len + position -- a gather only for those elements, which are rare.
// Both take 1024 consecutive elements per 256-thread workgroup, four per thread at a stride of 256 (every load and store coalesced).
#include "vrs_sort_rank.hpp"

namespace vrs {
namespace {

constexpr uint32_t kRankThreads = 256u, kRankItems = 4u, kRankTile = kRankThreads * kRankItems;

template <typename S, typename R, bool FLOAT, bool SIGNED>
__global__ __launch_bounds__(kRankThreads) void sort_rank_kernel(const S *__restrict__ src, uint32_t n, uint32_t row_len, R inf_bits,
                                                                 int descending, R *__restrict__ ranks, uint32_t *__restrict__ positions) {
    constexpr int B = 8 * static_cast<int>(sizeof(S));
    const uint32_t base = blockIdx.x * kRankTile + threadIdx.x;
#pragma unroll
    for (uint32_t j = 0; j < kRankItems; ++j) {
        const uint32_t i = base + j * kRankThreads;
        if (i < n) {
            ranks[i] = sort_rank<R, B, FLOAT, SIGNED>(static_cast<R>(src[i]), inf_bits, descending != 0);
            if (positions) positions[i] = i % row_len;
        }
    }
}

template <typename S, typename R, bool FLOAT, bool SIGNED>
__global__ __launch_bounds__(kRankThreads) void sort_restore_kernel(const S *__restrict__ src, const R *__restrict__ ranks,
                                                                    const uint32_t *__restrict__ positions, uint32_t n, uint32_t row_len,
                                                                    int descending, S *__restrict__ values, int64_t *__restrict__ indices) {
    constexpr int B = 8 * static_cast<int>(sizeof(S));
    const uint32_t base = blockIdx.x * kRankTile + threadIdx.x;
#pragma unroll
    for (uint32_t j = 0; j < kRankItems; ++j) {
        const uint32_t i = base + j * kRankThreads;
        if (i >= n) continue;
        const uint32_t pos = positions ? positions[i] : 0u;
        if (indices) indices[i] = static_cast<int64_t>(pos);
        if (values) {
            bool exact;
            const R u = sort_unrank<R, B, FLOAT, SIGNED>(ranks[i], descending != 0, &exact);
            // (the host refuses a float without positions; pos < row_len unless the caller's positions are not this input's)
            values[i] = exact ? static_cast<S>(u) : src[(i - i % row_len) + min(pos, row_len - 1u)];
        }
    }
}

template <typename S, typename R, bool FLOAT, bool SIGNED>
hipError_t rank_as(hipStream_t stream, const void *src, uint32_t n, uint32_t row_len, R inf_bits, bool descending, void *ranks,
                   uint32_t *positions) {
    const uint32_t blocks = static_cast<uint32_t>((static_cast<uint64_t>(n) + kRankTile - 1u) / kRankTile);
    hipLaunchKernelGGL((sort_rank_kernel<S, R, FLOAT, SIGNED>), dim3(blocks), dim3(kRankThreads), 0, stream, static_cast<const S *>(src), n,
                       row_len, inf_bits, descending ? 1 : 0, static_cast<R *>(ranks), positions);
    return hipGetLastError();
}

template <typename S, typename R, bool FLOAT, bool SIGNED>
hipError_t restore_as(hipStream_t stream, const void *src, const void *ranks, const uint32_t *positions, uint32_t n, uint32_t row_len,
                      bool descending, void *values, int64_t *indices) {
    const uint32_t blocks = static_cast<uint32_t>((static_cast<uint64_t>(n) + kRankTile - 1u) / kRankTile);
    hipLaunchKernelGGL((sort_restore_kernel<S, R, FLOAT, SIGNED>), dim3(blocks), dim3(kRankThreads), 0, stream, static_cast<const S *>(src),
                       static_cast<const R *>(ranks), positions, n, row_len, descending ? 1 : 0, static_cast<S *>(values), indices);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sort_rank(hipStream_t stream, const void *src, uint32_t n, uint32_t row_len, int dtype, bool descending, void *ranks,
                            uint32_t *positions) {
    if (n == 0u) return hipSuccess;
    switch (dtype) {
        case kSortI8: return rank_as<uint8_t, uint32_t, false, true>(stream, src, n, row_len, 0u, descending, ranks, positions);
        case kSortU8: return rank_as<uint8_t, uint32_t, false, false>(stream, src, n, row_len, 0u, descending, ranks, positions);
        case kSortI16: return rank_as<uint16_t, uint32_t, false, true>(stream, src, n, row_len, 0u, descending, ranks, positions);
        case kSortI32: return rank_as<uint32_t, uint32_t, false, true>(stream, src, n, row_len, 0u, descending, ranks, positions);
        case kSortI64: return rank_as<uint64_t, uint64_t, false, true>(stream, src, n, row_len, 0ull, descending, ranks, positions);
        case kSortF16: return rank_as<uint16_t, uint32_t, true, false>(stream, src, n, row_len, 0x7C00u, descending, ranks, positions);
        case kSortBF16: return rank_as<uint16_t, uint32_t, true, false>(stream, src, n, row_len, 0x7F80u, descending, ranks, positions);
        case kSortF32: return rank_as<uint32_t, uint32_t, true, false>(stream, src, n, row_len, 0x7F800000u, descending, ranks, positions);
        case kSortF64:
            return rank_as<uint64_t, uint64_t, true, false>(stream, src, n, row_len, 0x7FF0000000000000ull, descending, ranks, positions);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_sort_restore(hipStream_t stream, const void *src, const void *ranks, const uint32_t *positions, uint32_t n, uint32_t row_len,
                               int dtype, bool descending, void *values, int64_t *indices) {
    if (n == 0u || (!values && !indices)) return hipSuccess;
    switch (dtype) {
        case kSortI8: return restore_as<uint8_t, uint32_t, false, true>(stream, src, ranks, positions, n, row_len, descending, values, indices);
        case kSortU8: return restore_as<uint8_t, uint32_t, false, false>(stream, src, ranks, positions, n, row_len, descending, values, indices);
        case kSortI16: return restore_as<uint16_t, uint32_t, false, true>(stream, src, ranks, positions, n, row_len, descending, values, indices);
        case kSortI32: return restore_as<uint32_t, uint32_t, false, true>(stream, src, ranks, positions, n, row_len, descending, values, indices);
        case kSortI64: return restore_as<uint64_t, uint64_t, false, true>(stream, src, ranks, positions, n, row_len, descending, values, indices);
        case kSortF16:
        case kSortBF16: return restore_as<uint16_t, uint32_t, true, false>(stream, src, ranks, positions, n, row_len, descending, values, indices);
        case kSortF32: return restore_as<uint32_t, uint32_t, true, false>(stream, src, ranks, positions, n, row_len, descending, values, indices);
        case kSortF64: return restore_as<uint64_t, uint64_t, true, false>(stream, src, ranks, positions, n, row_len, descending, values, indices);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace vrs
