// vrs_scan.hip -- the prefix scan's SUM and PROD (the kernels of vrs_scan_kernels.hpp over the accumulator types) and its single pass.
//   scan_single_pass_kernel<X, NC>: C == 1, 4-byte accumulators.  One launch; every workgroup takes one ticket, which is four consecutive
//     tiles, one per wave, so the tiles start in order.  A wave loads its tile's rows once (up to NC chunks of 256, 16 bytes per lane and
//     load), keeps them in registers, publishes A(0)_j in a 64-bit status word that is its own flag, gathers the words its P_j is made
//     of (scan_lookback_wave: bounded polling, then it computes a missing word itself), and writes P_j (+) incl: 8 bytes per float32
//     element.  Every published word is a function of the input alone, so the result does not depend on which wave was early, and a
//     group's word goes out as soon as the level below it is read: no word waits for a word of its own level.  (Tried and dropped: a
//     ticket of 32 consecutive tiles walked in rounds -- every workgroup then waits for the one before it; workgroups that stay and
//     stride over the tiles -- one that is not resident holds everyone up until the budgets run out.)
#include "vrs_scan_kernels.hpp"

namespace vrs {
namespace {

// tile g of the call (tile g % tiles of segment g / tiles), by one wave
template <class X, uint32_t NC>
__device__ __forceinline__ void scan_single_pass_tile(const ScanArgs &a, const ScanWords &sw, uint32_t g, uint32_t tiles, uint32_t lane) {
    using Acc = typename X::Acc;
    const auto *in = static_cast<const typename X::In *>(a.values);
    auto *out = static_cast<typename X::Out *>(a.out);
    const uint32_t s = g / tiles, j = g % tiles;
    const uint32_t n = min(a.T, a.L - j * a.T), chunks = (n + kScanChunk - 1u) / kScanChunk;
    const size_t e0 = static_cast<size_t>(s) * a.L + static_cast<size_t>(j) * a.T;
    const bool vec = scan_vec_ok<X>(in, out, nullptr, e0);

    ScanHeld<X, NC> h;
#pragma unroll
    for (uint32_t q = 0; q < NC; ++q)
        if (q < chunks) scan_load_rows<X>(in, e0, n, 0, q, lane, vec, a.op, h.x[q]);
    const Acc mine = scan_tile_flat_hold<X, NC>(a.op, chunks, lane, h);

    // A(0)_m of this segment from its rows, for a word that was not published in time
    auto tile0 = [&](uint32_t m) {
        const uint32_t rows = min(a.T, a.L - m * a.T);
        const size_t first = static_cast<size_t>(s) * a.L + static_cast<size_t>(m) * a.T;
        const bool wide = scan_vec_ok<X>(in, nullptr, nullptr, first);
        auto load = [&](uint32_t q, Acc(&x)[kScanLaneRows]) { scan_load_rows<X>(in, first, rows, 0, q, lane, wide, a.op, x); };
        auto none = [](uint32_t, const Acc(&)[kScanLaneRows]) {};
        return scan_tile_flat_wave<X, 0>(a.op, rows, lane, X::identity(a.op), load, none);
    };
    const Acc P = scan_lookback_wave<X>(a.op, sw, s, j, lane, mine, tile0);

#pragma unroll
    for (uint32_t q = 0; q < NC; ++q) {
        if (q < chunks) {
            Acc o[kScanLaneRows];
            scan_tile_flat_release<X, NC>(a.op, q, P, h, o);
            scan_store_rows<X>(out, nullptr, e0, n, q, lane, vec, o);
        }
    }
}

template <class X, uint32_t NC>
__global__ __launch_bounds__(kThreads) void scan_single_pass_kernel(ScanArgs a, ScanWords sw, uint32_t *ticket, uint32_t tiles) {
    __shared__ uint32_t s_ticket;
    if (threadIdx.x == 0u) s_ticket = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const uint64_t g = static_cast<uint64_t>(s_ticket) * kWaves + (threadIdx.x >> 6);
    if (g < static_cast<uint64_t>(a.S) * tiles) scan_single_pass_tile<X, NC>(a, sw, static_cast<uint32_t>(g), tiles, lane_id());  // (S x L is below 2^32)
}

template <class X>
hipError_t launch_single_pass(hipStream_t stream, const ScanArgs &a, const ScanLayout &l) {
    hipError_t e = hipMemsetAsync(a.scratch, 0, l.bytes, stream);
    if (e != hipSuccess) return e;
    ScanWords sw{};
    for (uint32_t k = 0; k < l.levels; ++k) {
        sw.level[k] = reinterpret_cast<unsigned long long *>(a.scratch + l.level[k]);
        sw.words[k] = l.words[k];
    }
    sw.K = l.levels;
    sw.budget = a.spin_budget;
    sw.takeovers = a.takeovers;
    uint32_t *ticket = reinterpret_cast<uint32_t *>(a.scratch + l.ticket);
    const uint64_t tiles_all = static_cast<uint64_t>(a.S) * l.tiles;
    const uint32_t chunks = a.T / kScanChunk;
    const dim3 grid(static_cast<uint32_t>((tiles_all + kWaves - 1u) / kWaves)), block(kThreads);
    if (chunks <= 2u) hipLaunchKernelGGL((scan_single_pass_kernel<X, 2>), grid, block, 0, stream, a, sw, ticket, l.tiles);
    else if (chunks <= 8u) hipLaunchKernelGGL((scan_single_pass_kernel<X, 8>), grid, block, 0, stream, a, sw, ticket, l.tiles);
    else hipLaunchKernelGGL((scan_single_pass_kernel<X, 32>), grid, block, 0, stream, a, sw, ticket, l.tiles);
    return hipGetLastError();
}

template <class X>
hipError_t launch_arith(hipStream_t stream, const ScanArgs &a, const ScanLayout &l, uint32_t compute_units) {
    if constexpr (sizeof(typename X::Acc) == 4u)
        if (a.tier == kScanTierSinglePass) return launch_single_pass<X>(stream, a, l);
    return launch_scan_as<X>(stream, a, l, compute_units);
}

}  // namespace

hipError_t launch_scan_rows(hipStream_t stream, const ScanArgs &a, const ScanLayout &l, uint32_t compute_units) {
    if (a.op >= kScanMax) return launch_scan_pairs(stream, a, l, compute_units);
    if (a.out_dtype == kSortI64) {
        switch (a.dtype) {
            case kSortI8: return launch_arith<ScanArith<ReduceI64, int8_t>>(stream, a, l, compute_units);
            case kSortU8: return launch_arith<ScanArith<ReduceI64, uint8_t>>(stream, a, l, compute_units);
            case kSortI16: return launch_arith<ScanArith<ReduceI64, int16_t>>(stream, a, l, compute_units);
            case kSortI32: return launch_arith<ScanArith<ReduceI64, int32_t>>(stream, a, l, compute_units);
            default: return launch_arith<ScanArith<ReduceI64, int64_t>>(stream, a, l, compute_units);
        }
    }
    switch (a.out_dtype) {
        case kSortI32: return launch_arith<ScanArith<ReduceI32, int32_t>>(stream, a, l, compute_units);
        case kSortF16: return launch_arith<ScanArith<ReduceF16, uint16_t>>(stream, a, l, compute_units);
        case kSortBF16: return launch_arith<ScanArith<ReduceBF16, uint16_t>>(stream, a, l, compute_units);
        case kSortF32: return launch_arith<ScanArith<ReduceF32, float>>(stream, a, l, compute_units);
        default: return launch_arith<ScanArith<ReduceF64, double>>(stream, a, l, compute_units);
    }
}

}  // namespace vrs
