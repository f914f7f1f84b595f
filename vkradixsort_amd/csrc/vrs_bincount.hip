// vrs_bincount.hip -- the counting kernels of vrs_bin_count (torch.bincount / histc / histogram).
//   counter[bin(x)] += 1, or += the element's weight, for every element x that has a bin.
// One kernel, templated on how an element becomes a bin (T: the element itself, or the linear rule of vrs_bincount.hpp), on what is
// added (W: uint32_t = 1 per element, float / double = the weight) and on where the counters live:
//   LDS     every workgroup clears counters of its own in LDS, walks its tiles, and adds what is not zero to the accumulation buffer
//           with global atomics once: the global atomics of a call are at most grid x num_bins, whatever n.
//   GLOBAL  the same walk, adding straight to the accumulation buffer.
// The grid is bounded by the CUs (two workgroups of 1024 threads each; one when its counters take more than half a CU's LDS); a
// workgroup walks tiles of 16 KiB grid-stride, every thread one 16-byte vector of elements per tile (and its weights in 16-byte
// vectors; a view that starts off a 16-byte boundary has its tiles moved back to the boundary before it, see the loop).  Before an atomic, a wave whose lanes that have a bin all have the same one adds once: the popcount of those lanes (or the
// wave's sum of their weights) by one lane -- a constant input would otherwise serialise 64 lanes on one address.  All adds are
// no-return atomics; float sums therefore come in no specified order.
// Bounds: a bin is below num_bins by construction (IndexElem::bin, bin_linear), the LDS tier is taken only when num_bins counters fit
// the dynamic LDS of the launch, and elements are read below n only.
#include <atomic>
#include <type_traits>

#include "vrs_bincount.hpp"

namespace vrs {
namespace {

template <typename S_>
struct IndexElem {
    using S = S_;
    __device__ static uint32_t bin(S x, const BinCountArgs &a, int *side) {
        *side = 0;
        if constexpr (std::is_signed_v<S>) {
            if (x < 0) {
                *side = -1;
                return kBinNone;
            }
        }
        if (static_cast<unsigned long long>(x) >= a.num_bins) {
            *side = 1;
            return kBinNone;
        }
        return static_cast<uint32_t>(x);
    }
};
struct F16Elem {
    using S = uint16_t;
    __device__ static uint32_t bin(S x, const BinCountArgs &a, int *side) {
        return bin_linear<float>(bin_widen_f16(x), static_cast<float>(a.lo), static_cast<float>(a.hi), a.num_bins, side);
    }
};
struct BF16Elem {
    using S = uint16_t;
    __device__ static uint32_t bin(S x, const BinCountArgs &a, int *side) {
        return bin_linear<float>(bin_widen_bf16(x), static_cast<float>(a.lo), static_cast<float>(a.hi), a.num_bins, side);
    }
};
struct F32Elem {
    using S = float;
    __device__ static uint32_t bin(S x, const BinCountArgs &a, int *side) {
        return bin_linear<float>(x, static_cast<float>(a.lo), static_cast<float>(a.hi), a.num_bins, side);
    }
};
struct F64Elem {
    using S = double;
    __device__ static uint32_t bin(S x, const BinCountArgs &a, int *side) { return bin_linear<double>(x, a.lo, a.hi, a.num_bins, side); }
};

// N consecutive elements from p as vectors of up to 16 bytes (p is aligned to the smaller of 16 and N * sizeof(T) bytes)
template <typename T, int N>
__device__ inline void load_run(const T *p, T (&out)[N]) {
    constexpr int PER = static_cast<int>(16 / sizeof(T)) < N ? static_cast<int>(16 / sizeof(T)) : N;
    struct alignas(sizeof(T) * PER) Vec {
        T v[PER];
    };
#pragma unroll
    for (int c = 0; c < N / PER; ++c) {
        const Vec x = reinterpret_cast<const Vec *>(p)[c];
#pragma unroll
        for (int k = 0; k < PER; ++k) out[c * PER + k] = x.v[k];
    }
}

template <typename W>
__device__ inline W wave_sum(W v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

template <bool LDS, typename W>
__device__ inline void add_to(W *counter, W v) {
    if constexpr (LDS) {
        (void)__hip_atomic_fetch_add(counter, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
        (void)__hip_atomic_fetch_add(counter, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One element per lane (bin == kBinNone: none).  Called by whole waves only.
template <bool LDS, typename W>
__device__ inline void add_wave(W *counters, uint32_t stride, uint32_t bin, W w) {
    const unsigned long long have = __ballot(bin != kBinNone);
    if (have == 0ull) return;
    const int leader = __ffsll(static_cast<long long>(have)) - 1;
    const uint32_t first = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(bin), leader));
    const unsigned long long same = __ballot(bin == first);
    if (same == have) {  // (uniform) every lane that has a bin has this one: one add
        W sum;
        if constexpr (std::is_same_v<W, uint32_t>) {
            sum = static_cast<uint32_t>(__popcll(have));
        } else {
            sum = wave_sum(bin != kBinNone ? w : W(0));
        }
        if (static_cast<int>(threadIdx.x & 63u) == leader) add_to<LDS>(counters + static_cast<size_t>(first) * stride, sum);
    } else if (bin != kBinNone) {
        add_to<LDS>(counters + static_cast<size_t>(bin) * stride, w);
    }
}

template <typename T, typename W, bool LDS>
__global__ __launch_bounds__(kBinCountThreads) void bin_count_kernel(BinCountArgs a) {
    using S = typename T::S;
    constexpr bool WEIGHTED = !std::is_same_v<W, uint32_t>;
    constexpr uint32_t ITEMS = kBinCountLoadBytes / static_cast<uint32_t>(sizeof(S)), TILE = kBinCountThreads * ITEMS;
    extern __shared__ __align__(16) unsigned char bin_smem[];  // the LDS tier's counters; afterwards (both tiers) the workgroup's two skip counts
    W *lds = reinterpret_cast<W *>(bin_smem);
    W *acc = static_cast<W *>(a.acc);
    const S *values = static_cast<const S *>(a.values);
    const W *weights = static_cast<const W *>(a.weights);
    if (LDS) {
        for (uint32_t b = threadIdx.x; b < a.num_bins; b += kBinCountThreads) lds[b] = W(0);
        __syncthreads();
    }
    W *counters = LDS ? lds : acc;
    const uint32_t stride = LDS ? 1u : a.acc_stride;
    uint32_t below = 0u, above = 0u;
    // positions, not elements: element i sits at position i + shift (shift < ITEMS), so that a thread's run of ITEMS positions starts on
    // a 16-byte boundary of a view that does not (an int32 x[1:]).  The first `shift` positions hold nothing.
    const uint64_t n = a.n, shift = a.shift, tiles = (n + shift + TILE - 1u) / TILE;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t p0 = t * TILE + static_cast<uint64_t>(threadIdx.x) * ITEMS;
        const bool whole = a.vec_ok && p0 >= shift && p0 - shift + ITEMS <= n;
        S x[ITEMS];
        W w[ITEMS];
        if (whole) {
            load_run<S, ITEMS>(values + (p0 - shift), x);
            if constexpr (WEIGHTED) load_run<W, ITEMS>(weights + (p0 - shift), w);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < ITEMS; ++k) {
                const bool in = p0 + k >= shift && p0 + k - shift < n;
                x[k] = in ? values[p0 + k - shift] : S(0);
                if constexpr (WEIGHTED) w[k] = in ? weights[p0 + k - shift] : W(0);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < ITEMS; ++k) {
            int side = 0;
            const uint32_t bin = whole || (p0 + k >= shift && p0 + k - shift < n) ? T::bin(x[k], a, &side) : kBinNone;
            below += side < 0 ? 1u : 0u;
            above += side > 0 ? 1u : 0u;
            if constexpr (WEIGHTED) {
                add_wave<LDS, W>(counters, stride, bin, w[k]);
            } else {
                add_wave<LDS, W>(counters, stride, bin, 1u);
            }
        }
    }
    __syncthreads();
    if (LDS) {  // what this workgroup counted, to the accumulation buffer: the counters that are not zero only
        for (uint32_t b = threadIdx.x; b < a.num_bins; b += kBinCountThreads) {
            const W c = lds[b];
            if (c != W(0)) add_to<false>(acc + static_cast<size_t>(b) * a.acc_stride, c);
        }
        __syncthreads();
    }
    uint32_t *skip = reinterpret_cast<uint32_t *>(bin_smem);  // (the launch gives every workgroup 256 bytes at least)
    if (threadIdx.x < 2u) skip[threadIdx.x] = 0u;
    __syncthreads();
    if (below != 0u) add_to<true>(&skip[0], below);
    if (above != 0u) add_to<true>(&skip[1], above);
    __syncthreads();
    if (threadIdx.x < 2u && skip[threadIdx.x] != 0u) add_to<false>(&a.skip[threadIdx.x], skip[threadIdx.x]);
}

// the 32-bit counters as the output's dtype, each the correctly rounded count; the skip counters to where the caller wants them
__global__ __launch_bounds__(256) void bin_finish_kernel(BinFinishArgs a) {
    if (a.skipped && blockIdx.x == 0u && threadIdx.x < 2u) a.skipped[threadIdx.x] = a.skip[threadIdx.x];
    if (!a.counters) return;
    const uint64_t step = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t b = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; b < a.num_bins; b += step) {
        const uint32_t c = a.counters[b];
        switch (a.out_dtype) {
            case kSortF16: static_cast<_Float16 *>(a.out)[b] = static_cast<_Float16>(bin_count_rounded(c, 11)); break;
            case kSortBF16: static_cast<uint16_t *>(a.out)[b] = static_cast<uint16_t>(__builtin_bit_cast(uint32_t, bin_count_rounded(c, 8)) >> 16); break;
            case kSortF32: static_cast<float *>(a.out)[b] = static_cast<float>(c); break;
            case kSortF64: static_cast<double *>(a.out)[b] = static_cast<double>(c); break;
            default: break;
        }
    }
}

uint32_t lds_bytes_of(uint32_t num_bins, uint32_t counter_bytes, int tier) {
    if (tier != kBinCountTierLds) return 256u;
    return std::max<uint32_t>((num_bins * counter_bytes + 255u) & ~255u, 256u);
}

template <typename T, typename W>
hipError_t launch_as(hipStream_t stream, const BinCountArgs &a, int dtype, int weight_dtype, int tier) {
    const uint32_t lds = lds_bytes_of(a.num_bins, static_cast<uint32_t>(sizeof(W)), tier);
    const uint32_t grid = bin_count_grid(a.n, dtype, a.num_bins, weight_dtype, tier, a.compute_units);
    auto kernel = tier == kBinCountTierLds ? bin_count_kernel<T, W, true> : bin_count_kernel<T, W, false>;
    if (lds > 64u * 1024u) {  // (the LDS tier only) beyond the default limit: raised once per instantiation and device, to all a workgroup can claim
        static std::atomic<uint64_t> raised{0};  // one bit per device ordinal below 64
        int device = 0;
        hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess) return e;
        const uint64_t bit = device >= 0 && device < 64 ? 1ull << device : 0ull;
        if (!(raised.load(std::memory_order_relaxed) & bit)) {
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kBinCountLdsMaxBytes));
            if (e != hipSuccess) return e;
            raised.fetch_or(bit, std::memory_order_relaxed);
        }
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBinCountThreads), lds, stream, a);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_weighted(hipStream_t stream, const BinCountArgs &a, int dtype, int weight_dtype, int tier) {
    switch (weight_dtype) {
        case kBinNoWeights: return launch_as<T, uint32_t>(stream, a, dtype, weight_dtype, tier);
        case kSortF32: return launch_as<T, float>(stream, a, dtype, weight_dtype, tier);
        case kSortF64: return launch_as<T, double>(stream, a, dtype, weight_dtype, tier);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

uint32_t bin_count_grid(uint32_t n, int dtype, uint32_t num_bins, int weight_dtype, int tier, uint32_t compute_units) {
    const uint64_t tile = kBinCountTileBytes / static_cast<uint32_t>(sort_dtype_bytes(dtype));
    const uint64_t tiles = (static_cast<uint64_t>(n) + tile - 1u) / tile;
    const uint32_t lds = lds_bytes_of(num_bins, bin_counter_bytes(weight_dtype), tier);
    const uint32_t resident = (compute_units ? compute_units : 256u) * (lds > kBinCountLdsMaxBytes / 2u ? 1u : 2u);
    return static_cast<uint32_t>(std::max<uint64_t>(std::min<uint64_t>(tiles, resident), 1u));
}

hipError_t launch_bin_count(hipStream_t stream, const BinCountArgs &a, int dtype, int mode, int weight_dtype, int tier) {
    if (mode == kBinIndex) {
        switch (dtype) {
            case kSortI8: return launch_weighted<IndexElem<int8_t>>(stream, a, dtype, weight_dtype, tier);
            case kSortU8: return launch_weighted<IndexElem<uint8_t>>(stream, a, dtype, weight_dtype, tier);
            case kSortI16: return launch_weighted<IndexElem<int16_t>>(stream, a, dtype, weight_dtype, tier);
            case kSortI32: return launch_weighted<IndexElem<int32_t>>(stream, a, dtype, weight_dtype, tier);
            case kSortI64: return launch_weighted<IndexElem<int64_t>>(stream, a, dtype, weight_dtype, tier);
            default: return hipErrorInvalidValue;
        }
    }
    switch (dtype) {
        case kSortF16: return launch_weighted<F16Elem>(stream, a, dtype, weight_dtype, tier);
        case kSortBF16: return launch_weighted<BF16Elem>(stream, a, dtype, weight_dtype, tier);
        case kSortF32: return launch_weighted<F32Elem>(stream, a, dtype, weight_dtype, tier);
        case kSortF64: return launch_weighted<F64Elem>(stream, a, dtype, weight_dtype, tier);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_bin_finish(hipStream_t stream, const BinFinishArgs &a) {
    const uint32_t blocks = a.counters ? static_cast<uint32_t>(std::min<uint64_t>((static_cast<uint64_t>(a.num_bins) + 255u) / 256u, 4096u)) : 1u;
    hipLaunchKernelGGL(bin_finish_kernel, dim3(blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace vrs
