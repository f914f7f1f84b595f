// vrs_unique.hip -- run-length encoding (vrs_run_length_encode) and the encode half of unique (vrs_unique), plus unique's rank map.
//   rle_kernel: one pass over the keys.  Tiles of 4096 keys are taken in order from a ticket; wave w of a tile walks 16 chunks of 64
//     consecutive keys.  Head of i: i == 0 || k[i] != k[i-1] (the key in front of a lane comes by shuffle, in front of a wave from
//     memory); a chunk's heads are one __ballot, a lane's rank among them mbcnt.  The heads in front of the tile come by decoupled
//     look-back over one 64-bit status word per tile ({flag, count}: the word is its own flag, agent-scope atomics, no fence).
//     Every element writes its run id, every head its run's key and start.
//   rle_counts_kernel: counts[j] = offsets[j + 1] - offsets[j] for j < R, R read on the device; the grid is sized from n.
//   unique_map_kernel: keys -> ranks (and the iota payloads the sort carries for the inverse).
//   The grid-stride loops count in 64 bits: a 32-bit i + stride wraps to a small value still below a bound near 2^32 (a hang).
#include "vrs_unique.hpp"

#include "vrs_device.hpp"

#include <algorithm>

namespace vrs {
namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the heads among keys [lo, hi) (lo < hi <= n), counted by one wave straight from the keys: the give-up path of the look-back
template <typename K>
__device__ uint32_t count_heads(const K *keys, uint32_t lo, uint32_t hi, uint32_t lane) {
    uint32_t c = 0;
    for (uint64_t at = lo; at < hi; at += 64u) {
        const uint64_t i = at + lane;
        const bool head = i < hi && (i == 0u || keys[i] != keys[i - 1u]);
        c += static_cast<uint32_t>(__popcll(__ballot(head)));
    }
    return c;
}

// heads in front of `tile`, by the calling wave: windows of 64 predecessors, nearest first, summed up to the nearest inclusive word.  A
// window with an unpublished word in that range is polled again, at most kRleSpinBudget times; then the wave counts the nearest
// unpublished tile's heads from the keys and goes on behind it (the same count, slowly: progress never depends on another workgroup).
template <typename K>
__device__ uint32_t rle_lookback(const unsigned long long *status, uint32_t tile, const K *keys, uint32_t n, uint32_t lane) {
    uint32_t excl = 0, spins = 0;
    int pos = static_cast<int>(tile) - 1;
    while (pos >= 0) {
        const int p = pos - static_cast<int>(lane);
        const unsigned long long w = p >= 0 ? __hip_atomic_load(status + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kRleInclusive;
        const uint64_t inc = __ballot((w >> 62) == 2u), unpub = __ballot((w >> 62) == 0u);
        const uint64_t need = inc ? (2ull << __builtin_ctzll(inc)) - 1ull : ~0ull;  // lanes up to the nearest inclusive word
        if (unpub & need) {
            if (++spins < kRleSpinBudget) {
                __builtin_amdgcn_s_sleep(1);
                continue;
            }
            const int l = __builtin_ctzll(unpub & need);
            excl += wave_sum(static_cast<int>(lane) < l ? static_cast<uint32_t>(w) : 0u);
            const uint32_t lo = static_cast<uint32_t>(pos - l) * kRleTile;
            excl += count_heads(keys, lo, min(n, lo + kRleTile), lane);
            pos -= l + 1;
            spins = 0;
            continue;
        }
        excl += wave_sum(((need >> lane) & 1u) ? static_cast<uint32_t>(w) : 0u);
        if (inc) break;
        pos -= 64;
    }
    return excl;
}

// one tile; FULL: all of its 4096 keys lie below n (no bounds checks in the item loops)
template <typename K, bool FULL>
__device__ __forceinline__ void rle_tile(const RleArgs &a, uint32_t tile, uint32_t *s_prefix, uint32_t *s_wave) {
    const K *keys = static_cast<const K *>(a.keys);
    auto *status = reinterpret_cast<unsigned long long *>(a.status + 16);
    const uint32_t n = a.n, lane = lane_id(), wave = threadIdx.x >> 6;
    const uint32_t base = tile * kRleTile + wave * (kRleItems * 64u);  // first key of my wave (may lie beyond n in the last tile)
    // the tail tile: which of my items lie below n, as bits of one VGPR (not 16 exec masks live through the tile); its loads clamp
    uint32_t below = 0xFFFFu;
    if (!FULL) {
#pragma unroll
        for (uint32_t j = 0; j < kRleItems; ++j) below &= ~((base + j * 64u + lane < n ? 0u : 1u) << j);
        asm volatile("" : "+v"(below));
    }
    auto valid = [&](uint32_t j) { return FULL || ((below >> j) & 1u) != 0u; };

    K key[kRleItems];
#pragma unroll
    for (uint32_t j = 0; j < kRleItems; ++j) key[j] = keys[FULL ? base + j * 64u + lane : min(base + j * 64u + lane, n - 1u)];
    const K before = (lane == 0u && base != 0u && (FULL || base <= n)) ? keys[base - 1u] : K(0);

    // incl[j]: heads of my wave up to and including my key of chunk j
    uint32_t incl[kRleItems], heads = 0, run = 0;
#pragma unroll
    for (uint32_t j = 0; j < kRleItems; ++j) {
        const uint32_t i = base + j * 64u + lane;
        K prev = __shfl_up(key[j], 1u);
        const K wrap = j == 0u ? before : __shfl(key[j - 1u], 63);
        if (lane == 0u) prev = wrap;
        const bool head = valid(j) && (i == 0u || key[j] != prev);
        const uint64_t m = __ballot(head);
        incl[j] = run + count_below(m) + (head ? 1u : 0u);
        asm volatile("" : "+v"(incl[j]));  // computed here, kept in a VGPR: not 16 ballot masks kept alive in SGPRs until the stores
        run += static_cast<uint32_t>(__popcll(m));
        heads |= (head ? 1u : 0u) << j;
    }
    asm volatile("" : "+v"(heads));  // the stores test these bits, not 16 head masks kept alive in SGPRs
    if (lane == 0u) s_wave[wave] = run;
    __syncthreads();
    uint32_t wave_excl = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kRleThreads / 64u; ++w) {
        wave_excl += w < wave ? s_wave[w] : 0u;
        total += s_wave[w];
    }
    if (wave == 0u) {
        uint32_t prefix = 0;
        if (tile == 0u) {
            if (lane == 0u) __hip_atomic_store(status, kRleInclusive | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (lane == 0u) __hip_atomic_store(status + tile, kRleAggregate | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            prefix = rle_lookback(status, tile, keys, n, lane);
            if (lane == 0u) __hip_atomic_store(status + tile, kRleInclusive | (prefix + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0u) *s_prefix = prefix;
    }
    __syncthreads();
    const uint32_t first = *s_prefix + wave_excl - 1u;  // + incl = run id
    if (tile == rle_tiles(n) - 1u && threadIdx.x == 0u) {
        const uint32_t R = *s_prefix + total;
        *a.out_num_runs = R;
        if (a.out_offsets) a.out_offsets[R] = n;
    }
    if (a.out_run_ids) {
        if (a.idx) {  // unique: the inverse, through the sorted positions
#pragma unroll
            for (uint32_t j = 0; j < kRleItems; ++j)
                if (valid(j)) a.out_run_ids[a.idx[base + j * 64u + lane]] = first + incl[j];
        } else {
#pragma unroll
            for (uint32_t j = 0; j < kRleItems; ++j)
                if (valid(j)) a.out_run_ids[base + j * 64u + lane] = first + incl[j];
        }
    }
    if (heads != 0u) {
        K *out_keys = static_cast<K *>(a.out_keys);
#pragma unroll
        for (uint32_t j = 0; j < kRleItems; ++j) {
            if ((heads >> j) & 1u) {  // (a head is a valid element)
                const uint32_t r = first + incl[j];
                if (out_keys) out_keys[r] = a.key_type >= 0 ? unique_unrank(key[j], a.key_type) : key[j];
                if (a.out_offsets) a.out_offsets[r] = base + j * 64u + lane;
            }
        }
    }
}

template <typename K>
__global__ __launch_bounds__(kRleThreads) void rle_kernel(RleArgs a) {
    __shared__ uint32_t s_tile, s_prefix, s_wave[kRleThreads / 64u];
    if (threadIdx.x == 0u) s_tile = __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(a.status), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const uint32_t tile = s_tile;
    if (static_cast<uint64_t>(tile + 1u) * kRleTile <= a.n)
        rle_tile<K, true>(a, tile, &s_prefix, s_wave);
    else
        rle_tile<K, false>(a, tile, &s_prefix, s_wave);
}

__global__ __launch_bounds__(256) void rle_counts_kernel(const uint32_t *offsets, const uint32_t *num_runs, uint32_t *counts) {
    const uint32_t R = *num_runs;
    for (size_t j = blockIdx.x * 256u + threadIdx.x; j < R; j += gridDim.x * 256u) counts[j] = offsets[j + 1u] - offsets[j];
}

template <typename K>
__global__ __launch_bounds__(256) void unique_map_kernel(const K *keys, uint32_t n, int key_type, K *mapped, uint32_t *vals) {
    for (size_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        mapped[i] = unique_rank(keys[i], key_type);
        if (vals) vals[i] = static_cast<uint32_t>(i);
    }
}

uint32_t stride_grid(uint32_t n, uint32_t per_block) { return static_cast<uint32_t>(std::min<uint64_t>((static_cast<uint64_t>(n) + per_block - 1u) / per_block, 8192u)); }

}  // namespace

hipError_t launch_rle(hipStream_t stream, const RleArgs &a) {
    hipError_t e = hipMemsetAsync(a.status, 0, rle_status_bytes(a.n), stream);
    if (e != hipSuccess) return e;
    if (a.key_bytes == 8)
        hipLaunchKernelGGL(rle_kernel<uint64_t>, dim3(rle_tiles(a.n)), dim3(kRleThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(rle_kernel<uint32_t>, dim3(rle_tiles(a.n)), dim3(kRleThreads), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.out_counts) {
        hipLaunchKernelGGL(rle_counts_kernel, dim3(stride_grid(a.n, 1024u)), dim3(256), 0, stream, a.out_offsets, a.out_num_runs, a.out_counts);
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_unique_map(hipStream_t stream, const void *keys, uint32_t n, int key_type, void *mapped, uint32_t *vals) {
    const dim3 grid(stride_grid(n, 1024u));
    if (unique_key_bytes(key_type) == 8)
        hipLaunchKernelGGL(unique_map_kernel<uint64_t>, grid, dim3(256), 0, stream, static_cast<const uint64_t *>(keys), n, key_type,
                           static_cast<uint64_t *>(mapped), vals);
    else
        hipLaunchKernelGGL(unique_map_kernel<uint32_t>, grid, dim3(256), 0, stream, static_cast<const uint32_t *>(keys), n, key_type,
                           static_cast<uint32_t *>(mapped), vals);
    return hipGetLastError();
}

}  // namespace vrs
