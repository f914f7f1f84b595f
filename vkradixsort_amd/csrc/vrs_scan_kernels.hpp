// vrs_scan_kernels.hpp -- the prefix scan's kernels as templates over an algebra X of vrs_scan_order.hpp; vrs_scan.hip instantiates them
// for SUM and PROD (and holds the single pass), vrs_scan_pairs.hip for MAX and MIN.  What is combined with what is decided by the functions
// of vrs_scan_order.hpp alone; here are only addresses, loads and stores.  Internal.
//   scan_flat_kernel<X, MODE>     C == 1: one wave per tile, chunk after chunk (16-byte loads where the tile's first row allows).
//                                 MODE 0 writes A(0), 1 writes out for L <= T, 2 writes P (+) incl
//   scan_columns_kernel<X, MODE>  C > 1: one lane per (segment, tile, column), neighbouring lanes on neighbouring columns
//   scan_levels_kernel<X>         A(k) from A(k-1), one lane per word;  scan_prefix_kernel<X>: every P_j, one lane per tile and column
//   The grid-stride loops count in 64 bits: S * L * C may pass 2^32.
#pragma once
#include "vrs_scan.hpp"

#include "vrs_device.hpp"

#include <algorithm>

namespace vrs {

template <typename E>
struct alignas(4 * sizeof(E)) ScanVec {
    E v[kScanLaneRows];
};

// whether the four rows of every lane of a tile that starts at element e0 can move as one vector
template <class X>
__device__ __forceinline__ bool scan_vec_ok(const typename X::In *in, const typename X::Out *out, const int64_t *idx, size_t e0) {
    uintptr_t bad = reinterpret_cast<uintptr_t>(in + e0) % sizeof(ScanVec<typename X::In>);
    if (out) bad |= reinterpret_cast<uintptr_t>(out + e0) % sizeof(ScanVec<typename X::Out>);
    if (X::kPairs && idx) bad |= reinterpret_cast<uintptr_t>(idx + e0) % sizeof(ScanVec<int64_t>);
    return bad == 0u;
}

// the lane's four rows of chunk q of a tile of n rows whose first row is element e0 and row row0 of its segment
template <class X>
__device__ __forceinline__ void scan_load_rows(const typename X::In *in, size_t e0, uint32_t n, int64_t row0, uint32_t q, uint32_t lane, bool vec, int op,
                                               typename X::Acc (&x)[kScanLaneRows]) {
    const uint32_t r = q * kScanChunk + lane * kScanLaneRows;
    if (vec && r + kScanLaneRows <= n) {
        const ScanVec<typename X::In> got = *reinterpret_cast<const ScanVec<typename X::In> *>(in + e0 + r);
#pragma unroll
        for (uint32_t k = 0; k < kScanLaneRows; ++k) x[k] = X::load(got.v[k], row0 + r + k);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < kScanLaneRows; ++k) x[k] = r + k < n ? X::load(in[e0 + r + k], row0 + r + k) : X::identity(op);
    }
}
template <class X>
__device__ __forceinline__ void scan_store_rows(typename X::Out *out, int64_t *idx, size_t e0, uint32_t n, uint32_t q, uint32_t lane, bool vec,
                                                const typename X::Acc (&o)[kScanLaneRows]) {
    const uint32_t r = q * kScanChunk + lane * kScanLaneRows;
    if (vec && r + kScanLaneRows <= n) {
        ScanVec<typename X::Out> values;
        ScanVec<int64_t> rows;
#pragma unroll
        for (uint32_t k = 0; k < kScanLaneRows; ++k) X::store(values.v, rows.v, k, o[k]);
        *reinterpret_cast<ScanVec<typename X::Out> *>(out + e0 + r) = values;
        if constexpr (X::kPairs) *reinterpret_cast<ScanVec<int64_t> *>(idx + e0 + r) = rows;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < kScanLaneRows; ++k)
            if (r + k < n) X::store(out, idx, e0 + r + k, o[k]);
    }
}

template <class X, int MODE>
__global__ __launch_bounds__(kThreads) void scan_flat_kernel(ScanArgs a, typename X::Acc *A0, const typename X::Acc *P, uint32_t tiles) {
    using Acc = typename X::Acc;
    const auto *in = static_cast<const typename X::In *>(a.values);
    auto *out = static_cast<typename X::Out *>(a.out);
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t total = static_cast<uint64_t>(a.S) * tiles;
    const size_t stride = static_cast<size_t>(gridDim.x) * kWaves;
    for (uint64_t g = blockIdx.x * kWaves + wave; g < total; g += stride) {
        const uint32_t s = static_cast<uint32_t>(g / tiles), j = static_cast<uint32_t>(g % tiles);
        const uint32_t n = min(a.T, a.L - j * a.T);
        const size_t e0 = static_cast<size_t>(s) * a.L + static_cast<size_t>(j) * a.T;
        const int64_t row0 = static_cast<int64_t>(j) * a.T;
        const bool vec = scan_vec_ok<X>(in, MODE != 0 ? out : nullptr, a.indices, e0);
        auto load = [&](uint32_t q, Acc(&x)[kScanLaneRows]) { scan_load_rows<X>(in, e0, n, row0, q, lane, vec, a.op, x); };
        auto emit = [&](uint32_t q, const Acc(&o)[kScanLaneRows]) { scan_store_rows<X>(out, a.indices, e0, n, q, lane, vec, o); };
        Acc before = X::identity(a.op);
        if constexpr (MODE == 2) before = P[g];
        const Acc aggregate = scan_tile_flat_wave<X, MODE>(a.op, n, lane, before, load, emit);
        if constexpr (MODE == 0)
            if (lane == 0u) A0[g] = aggregate;
    }
}

template <class X, int MODE>
__global__ __launch_bounds__(kThreads) void scan_columns_kernel(ScanArgs a, typename X::Acc *A0, const typename X::Acc *P, uint32_t tiles) {
    using Acc = typename X::Acc;
    const auto *in = static_cast<const typename X::In *>(a.values);
    auto *out = static_cast<typename X::Out *>(a.out);
    const uint64_t total = static_cast<uint64_t>(a.S) * tiles * a.C;
    const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; g < total; g += stride) {
        const uint32_t c = static_cast<uint32_t>(g % a.C);
        const uint64_t sj = g / a.C;
        const uint32_t s = static_cast<uint32_t>(sj / tiles), j = static_cast<uint32_t>(sj % tiles);
        const uint32_t n = min(a.T, a.L - j * a.T);
        const size_t base = (static_cast<size_t>(s) * a.L + static_cast<size_t>(j) * a.T) * a.C + c;
        const int64_t row0 = static_cast<int64_t>(j) * a.T;
        auto row = [&](uint32_t r) { return X::load(in[base + static_cast<size_t>(r) * a.C], row0 + r); };
        auto emit = [&](uint32_t r, Acc v) { X::store(out, a.indices, base + static_cast<size_t>(r) * a.C, v); };
        Acc before = X::identity(a.op);
        if constexpr (MODE == 2) before = P[g];
        const Acc aggregate = scan_tile_columns<X, MODE>(a.op, n, before, row, emit);
        if constexpr (MODE == 0) A0[g] = aggregate;
    }
}

// level k's complete groups from level k - 1: S x full x C words
template <class X>
__global__ __launch_bounds__(kThreads) void scan_levels_kernel(const typename X::Acc *below, typename X::Acc *level, uint32_t S, uint32_t C, uint32_t words_below,
                                                               uint32_t words, uint32_t full, int op) {
    const uint64_t total = static_cast<uint64_t>(S) * full * C;
    const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; g < total; g += stride) {
        const uint32_t c = static_cast<uint32_t>(g % C);
        const uint64_t sm = g / C;
        const uint32_t s = static_cast<uint32_t>(sm / full), m = static_cast<uint32_t>(sm % full);
        const size_t first = (static_cast<size_t>(s) * words_below + static_cast<size_t>(m) * kScanFan) * C + c;
        level[(static_cast<size_t>(s) * words + m) * C + c] = scan_fold<X>(op, kScanFan, [&](uint32_t i) { return below[first + static_cast<size_t>(i) * C]; });
    }
}

template <typename Acc>
struct ScanLevels {
    const Acc *level[kScanMaxLevels];
    uint32_t words[kScanMaxLevels];
};
template <class X>
__global__ __launch_bounds__(kThreads) void scan_prefix_kernel(ScanLevels<typename X::Acc> d, typename X::Acc *P, uint32_t S, uint32_t C, uint32_t tiles, uint32_t K,
                                                               int op) {
    const uint64_t total = static_cast<uint64_t>(S) * tiles * C;
    const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; g < total; g += stride) {
        const uint32_t c = static_cast<uint32_t>(g % C);
        const uint64_t sj = g / C;
        const uint32_t s = static_cast<uint32_t>(sj / tiles), j = static_cast<uint32_t>(sj % tiles);
        P[g] = scan_tile_prefix<X>(op, j, K, [&](uint32_t k, uint32_t m) { return d.level[k][(static_cast<size_t>(s) * d.words[k] + m) * C + c]; });
    }
}

inline uint32_t scan_grid(uint64_t items, uint32_t per_block, uint32_t cap) {
    return static_cast<uint32_t>(std::max<uint64_t>(std::min<uint64_t>((items + per_block - 1u) / per_block, cap), 1u));
}

// the tile tier and the three-launch form for one algebra
template <class X>
hipError_t launch_scan_as(hipStream_t stream, const ScanArgs &a, const ScanLayout &l, uint32_t compute_units) {
    using Acc = typename X::Acc;
    const uint32_t cap = std::max(compute_units, 64u) * 32u;  // the kernels stride over what is left
    const uint64_t tiles_all = static_cast<uint64_t>(a.S) * l.tiles, lanes_all = tiles_all * a.C;
    const dim3 flat(scan_grid(tiles_all, kWaves, cap)), columns(scan_grid(lanes_all, kThreads, cap)), block(kThreads);
    if (a.tier == kScanTierTile) {
        if (a.C == 1u) hipLaunchKernelGGL((scan_flat_kernel<X, 1>), flat, block, 0, stream, a, nullptr, nullptr, l.tiles);
        else hipLaunchKernelGGL((scan_columns_kernel<X, 1>), columns, block, 0, stream, a, nullptr, nullptr, l.tiles);
        return hipGetLastError();
    }
    ScanLevels<Acc> d{};
    Acc *level[kScanMaxLevels] = {};
    for (uint32_t k = 0; k < l.levels; ++k) {
        d.level[k] = level[k] = reinterpret_cast<Acc *>(a.scratch + l.level[k]);
        d.words[k] = l.words[k];
    }
    Acc *P = reinterpret_cast<Acc *>(a.scratch + l.prefix);
    if (a.C == 1u) hipLaunchKernelGGL((scan_flat_kernel<X, 0>), flat, block, 0, stream, a, level[0], nullptr, l.tiles);
    else hipLaunchKernelGGL((scan_columns_kernel<X, 0>), columns, block, 0, stream, a, level[0], nullptr, l.tiles);
    for (uint32_t k = 1; k < l.levels; ++k) {
        const uint32_t full = l.tiles >> (kScanFanBits * k);
        if (full == 0u) break;
        hipLaunchKernelGGL((scan_levels_kernel<X>), dim3(scan_grid(static_cast<uint64_t>(a.S) * full * a.C, kThreads, cap)), block, 0, stream, level[k - 1u], level[k],
                           a.S, a.C, l.words[k - 1u], l.words[k], full, a.op);
    }
    hipLaunchKernelGGL((scan_prefix_kernel<X>), columns, block, 0, stream, d, P, a.S, a.C, l.tiles, l.levels, a.op);
    if (a.C == 1u) hipLaunchKernelGGL((scan_flat_kernel<X, 2>), flat, block, 0, stream, a, nullptr, P, l.tiles);
    else hipLaunchKernelGGL((scan_columns_kernel<X, 2>), columns, block, 0, stream, a, nullptr, P, l.tiles);
    return hipGetLastError();
}

hipError_t launch_scan_pairs(hipStream_t stream, const ScanArgs &a, const ScanLayout &l, uint32_t compute_units);  // vrs_scan_pairs.hip

}  // namespace vrs
