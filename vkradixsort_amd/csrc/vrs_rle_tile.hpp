// vrs_rle_tile.hpp -- the run-length encode's tile and its look-back (device code), with the key source a template parameter: what
// vrs_unique.hip (keys compared as words) and vrs_unique_rows.hip (rows: a top key per element, the columns behind it fetched only for
// a pair whose top keys are equal) instantiate.  Internal; see vrs_unique.hip for the kernel's description.
//   A source S has: Key (uint32_t / uint64_t, what a lane keeps per element and the shuffles carry); load(i) -> the Key of element i;
//   head(key, prev, i) -> element i (> 0) starts a run, given its Key and the one in front; kPlain: the heads' Keys are the run's keys
//   (written to out_keys by the tile itself; a row source's rows go out by a launch of their own).
#pragma once
#include "vrs_unique.hpp"

#include "vrs_device.hpp"

namespace vrs {

template <typename K>
struct RlePlainSource {
    using Key = K;
    static constexpr bool kPlain = true;
    const K *keys;
    __device__ __forceinline__ K load(uint32_t i) const { return keys[i]; }
    __device__ __forceinline__ bool head(K key, K prev, uint32_t) const { return key != prev; }
};

__device__ __forceinline__ uint32_t rle_wave_sum(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the heads among keys [lo, hi) (lo < hi <= n), counted by one wave straight from the keys: the give-up path of the look-back
template <typename S>
__device__ uint32_t count_heads(const S &src, uint32_t lo, uint32_t hi, uint32_t lane) {
    uint32_t c = 0;
    for (uint64_t at = lo; at < hi; at += 64u) {
        const uint64_t i = at + lane;
        const bool head = i < hi && (i == 0u || src.head(src.load(static_cast<uint32_t>(i)), src.load(static_cast<uint32_t>(i - 1u)), static_cast<uint32_t>(i)));
        c += static_cast<uint32_t>(__popcll(__ballot(head)));
    }
    return c;
}

// heads in front of `tile`, by the calling wave: windows of 64 predecessors, nearest first, summed up to the nearest inclusive word.  A
// window with an unpublished word in that range is polled again, at most kRleSpinBudget times; then the wave counts the nearest
// unpublished tile's heads from the keys and goes on behind it (the same count, slowly: progress never depends on another workgroup).
template <typename S>
__device__ uint32_t rle_lookback(const unsigned long long *status, uint32_t tile, const S &src, uint32_t n, uint32_t lane) {
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
            excl += rle_wave_sum(static_cast<int>(lane) < l ? static_cast<uint32_t>(w) : 0u);
            const uint32_t lo = static_cast<uint32_t>(pos - l) * kRleTile;
            excl += count_heads(src, lo, min(n, lo + kRleTile), lane);
            pos -= l + 1;
            spins = 0;
            continue;
        }
        excl += rle_wave_sum(((need >> lane) & 1u) ? static_cast<uint32_t>(w) : 0u);
        if (inc) break;
        pos -= 64;
    }
    return excl;
}

// one tile; FULL: all of its 4096 keys lie below n (no bounds checks in the item loops)
template <typename S, bool FULL>
__device__ __forceinline__ void rle_tile(const RleArgs &a, const S &src, uint32_t tile, uint32_t *s_prefix, uint32_t *s_wave) {
    using K = typename S::Key;
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
    for (uint32_t j = 0; j < kRleItems; ++j) key[j] = src.load(FULL ? base + j * 64u + lane : min(base + j * 64u + lane, n - 1u));
    const K before = (lane == 0u && base != 0u && (FULL || base <= n)) ? src.load(base - 1u) : K(0);

    // incl[j]: heads of my wave up to and including my key of chunk j
    uint32_t incl[kRleItems], heads = 0, run = 0;
#pragma unroll
    for (uint32_t j = 0; j < kRleItems; ++j) {
        const uint32_t i = base + j * 64u + lane;
        K prev = __shfl_up(key[j], 1u);
        const K wrap = j == 0u ? before : __shfl(key[j - 1u], 63);
        if (lane == 0u) prev = wrap;
        const bool head = valid(j) && (i == 0u || src.head(key[j], prev, i));
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
            prefix = rle_lookback(status, tile, src, n, lane);
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
                if constexpr (S::kPlain) {
                    if (out_keys) out_keys[r] = a.key_type >= 0 ? unique_unrank(key[j], a.key_type) : key[j];
                }
                if (a.out_offsets) a.out_offsets[r] = base + j * 64u + lane;
            }
        }
    }
}

// the kernel's body: a tile from the ticket, full or the tail
template <typename S>
__device__ __forceinline__ void rle_block(const RleArgs &a, const S &src) {
    __shared__ uint32_t s_tile, s_prefix, s_wave[kRleThreads / 64u];
    if (threadIdx.x == 0u) s_tile = __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(a.status), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const uint32_t tile = s_tile;
    if (static_cast<uint64_t>(tile + 1u) * kRleTile <= a.n)
        rle_tile<S, true>(a, src, tile, &s_prefix, s_wave);
    else
        rle_tile<S, false>(a, src, tile, &s_prefix, s_wave);
}

}  // namespace vrs
