// vrs_segmented.hip -- the segmented sorts (vrs_sort_segments_u32 / _pairs_u32 and their 64-bit forms vrs_sort_segments_u64 / _pairs_u64):
// many independent segments of one buffer sorted by one sequence of launches whose shapes do not depend on the segments.  Every kernel
// below is one template over the key type; the 64-bit forms differ in the LDS tiers' capacities (vrs_segmented.hpp) and in the digits.
//   classify: one read of the offsets; every segment gets its tier (segment_tier, the function vrs_segment_tier_for exports) and a
//     place in the work list of the workgroup shape that sorts it; per-tier counters for vrs_segmented_stats.
//   LDS tiers: one workgroup per listed segment (grids of the list's capacity, workgroups beyond the count leave at once).  The
//     segment is read once into registers, sorted by ceil(varying bits / 9) 9-bit local_pass'es from bit 0 (varying bits: the OR of
//     k ^ k_first over the segment; a constant segment is left as it is) and written once: 8 bytes of HBM traffic per key, 16 per pair
//     (64-bit keys: 16 and 24).
//   global tier: one 1024-thread workgroup per segment, LSD through keys_tmp: one counting read of all four (eight) digits, then a stable
//     tile-by-tile scatter per digit that is not the same for every key, and the copy home after an odd number of passes.
//   publish: the one-call tier's list goes to pinned host memory, stamped last; the host sorts those segments with the one-call sort.
#include "vrs_segmented.hpp"

#include "vrs_local_sort.hpp"

namespace vrs {
namespace {

__global__ __launch_bounds__(256) void segmented_classify_kernel(const uint32_t *__restrict__ offsets, uint32_t num_segments, uint32_t n,
                                                                 int pairs, uint32_t one_call_min_keys, SegControl *__restrict__ control,
                                                                 SegLists lists, int wide) {
    __shared__ uint32_t s_cnt[kSegLists], s_base[kSegLists], s_stat[4];
    const uint32_t tid = threadIdx.x;
    if (tid < kSegLists) s_cnt[tid] = 0u;
    if (tid < 4u) s_stat[tid] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + tid;
    int list = -1;
    uint32_t pos = 0, cb = 0, ce = 0;
    if (i < num_segments) {
        const int tier = segment_tier(offsets[i], offsets[i + 1u], n, pairs != 0, one_call_min_keys, &cb, &ce, wide != 0);
        atomicAdd(&s_stat[tier], 1u);
        list = segment_list(tier, ce - cb);
        if (list >= 0) pos = atomicAdd(&s_cnt[list], 1u);
    }
    __syncthreads();
    if (tid < kSegLists && s_cnt[tid] != 0u) s_base[tid] = atomicAdd(&control->count[tid], s_cnt[tid]);
    if (tid < 4u && s_stat[tid] != 0u) atomicAdd(&control->stats[tid], static_cast<unsigned long long>(s_stat[tid]));
    __syncthreads();
    if (list >= 0) {
        const uint32_t at = s_base[list] + pos;
        if (at < lists.cap[list]) lists.list[list][at] = make_uint2(cb, ce);  // (beyond: ranges that overlap -- malformed offsets)
    }
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
    return (static_cast<uint64_t>(wave_or(static_cast<uint32_t>(v >> 32))) << 32) | wave_or(static_cast<uint32_t>(v));
}
__device__ __forceinline__ uint32_t bit_width(uint32_t v) { return 32u - static_cast<uint32_t>(__clz(v)); }
__device__ __forceinline__ uint32_t bit_width(uint64_t v) { return 64u - static_cast<uint32_t>(__clzll(v)); }

// One listed segment of up to THREADS * ITEMS keys (pairs) sorted in LDS by its varying bits.  K: uint32_t or uint64_t.
template <typename K, int THREADS, int ITEMS, bool PAIRS, int LIST>
__global__ __launch_bounds__(THREADS) void segmented_lds_sort_kernel(K *__restrict__ keys, uint32_t *__restrict__ values,
                                                                     const SegControl *__restrict__ control, SegLists lists) {
    constexpr int WAVES = THREADS / 64, CAP = THREADS * ITEMS;
    __shared__ K s_keys[CAP];
    __shared__ uint32_t s_vals[PAIRS ? CAP : 1];
    __shared__ uint32_t s_hist[WAVES * 512];
    __shared__ uint32_t s_tmp[WAVES];
    const uint32_t count = min(control->count[LIST], lists.cap[LIST]);
    if (blockIdx.x >= count) return;
    const uint2 range = lists.list[LIST][blockIdx.x];
    const uint32_t b = range.x, n = range.y - range.x;
    if (n < 2u || n > static_cast<uint32_t>(CAP)) return;  // (the classification never lists such a segment)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t seg = wave * (ITEMS * 64) + lane;
    const K *src = keys + b;
    K key[ITEMS];
    uint32_t val[PAIRS ? ITEMS : 1];
    // positions >= n take the last key (they are never ranked nor stored; the OR below stays that of the segment)
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t idx = seg + i * 64;
        key[i] = src[idx < n ? idx : n - 1u];
    }
    if constexpr (PAIRS) {
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t idx = seg + i * 64;
            val[i] = values[b + (idx < n ? idx : n - 1u)];
        }
    }
    const K k0 = src[0];
    K diff = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) diff |= key[i] ^ k0;
    diff = wave_or(diff);
    if constexpr (WAVES > 1) {  // (through s_keys: the first pass writes it only behind two barriers, when every wave has read this)
        if (lane == 0u) s_keys[wave] = diff;
        __syncthreads();
#pragma unroll
        for (int v = 0; v < WAVES; ++v) diff |= s_keys[v];
    }
    if (diff == 0u) return;  // a constant segment: nothing to sort, nothing to store
    const uint32_t width = bit_width(diff);
    uint32_t shift = 0;
    if constexpr (!PAIRS) {  // bare keys: ties of the first digit in any order (the later passes or equality tell them apart)
        local_pass<THREADS, ITEMS, 9, false, false, K>(key, val, s_keys, nullptr, s_hist, s_tmp, 0u, n);
        shift = 9u;
    }
    for (; shift < width; shift += 9u) local_pass<THREADS, ITEMS, 9, PAIRS, true, K>(key, val, s_keys, s_vals, s_hist, s_tmp, shift, n);
    K *dst = keys + b;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t idx = seg + i * 64;
        if (idx < n) dst[idx] = key[i];
    }
    if constexpr (PAIRS) {
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t idx = seg + i * 64;
            if (idx < n) values[b + idx] = val[i];
        }
    }
}

// One listed segment of any length sorted by one workgroup through keys_tmp (stable).  K: uint32_t (four digits) or uint64_t (eight).
template <typename K, bool PAIRS>
__global__ __launch_bounds__(1024) void segmented_global_sort_kernel(K *__restrict__ keys, K *__restrict__ keys_tmp,
                                                                     uint32_t *__restrict__ values, uint32_t *__restrict__ values_tmp,
                                                                     const SegControl *__restrict__ control, SegLists lists) {
    constexpr int THREADS = 1024, ITEMS = 8, TILE = THREADS * ITEMS, WAVES = THREADS / 64, DIGITS = static_cast<int>(sizeof(K));
    __shared__ K s_keys[TILE];
    __shared__ uint32_t s_vals[PAIRS ? TILE : 1];
    __shared__ uint32_t s_hist[WAVES * 256];
    __shared__ uint32_t s_tmp[WAVES];
    __shared__ uint32_t s_cnt[DIGITS * 256];
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_same[DIGITS];  // digit j is the same in every key: its pass is the identity
    const uint32_t count = min(control->count[kSegListGlobal], lists.cap[kSegListGlobal]);
    if (blockIdx.x >= count) return;
    const uint2 range = lists.list[kSegListGlobal][blockIdx.x];
    const uint32_t b = range.x, n = range.y - range.x;
    if (n < 2u) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
#pragma unroll
    for (int c = 0; c < DIGITS / 4; ++c) s_cnt[c * THREADS + tid] = 0u;
    if (tid < static_cast<uint32_t>(DIGITS)) s_same[tid] = 0u;
    __syncthreads();
    for (size_t idx = tid; idx < n; idx += THREADS) {  // (64-bit here and below: a 32-bit idx + THREADS wraps below n near 2^32)
        const K k = keys[b + idx];
#pragma unroll
        for (int j = 0; j < DIGITS; ++j) atomicAdd(&s_cnt[j * 256 + static_cast<uint32_t>((k >> (8 * j)) & 255u)], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < DIGITS / 4; ++c)
        if (s_cnt[c * THREADS + tid] == n) s_same[(c * THREADS + tid) >> 8] = 1u;
    __syncthreads();
    const uint32_t seg = wave * (ITEMS * 64) + lane;
    uint32_t cur = 0;  // 0: the keys are in `keys`, 1: in `keys_tmp`
    for (uint32_t j = 0; j < static_cast<uint32_t>(DIGITS); ++j) {
        if (s_same[j] != 0u) continue;
        const uint32_t shift = 8u * j;
        if (tid < 256u) {  // where each digit's keys start in the segment
            const uint32_t c = s_cnt[j * 256u + tid];
            uint32_t incl = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_up(incl, o);
                if (lane >= static_cast<uint32_t>(o)) incl += t;
            }
            if (lane == 63u) s_tmp[wave] = incl;
            s_base[tid] = incl - c;
        }
        __syncthreads();
        if (tid < 256u) {
            uint32_t add = 0;
            for (uint32_t v = 0; v < wave; ++v) add += s_tmp[v];
            s_base[tid] += add;
        }
        __syncthreads();
        const K *kin = (cur ? keys_tmp : keys) + b;
        K *kout = (cur ? keys : keys_tmp) + b;
        const uint32_t *vin = PAIRS ? (cur ? values_tmp : values) + b : nullptr;
        uint32_t *vout = PAIRS ? (cur ? values : values_tmp) + b : nullptr;
        for (uint64_t tile0 = 0; tile0 < n; tile0 += TILE) {
            const uint32_t t0 = static_cast<uint32_t>(tile0), nt = min(static_cast<uint32_t>(TILE), n - t0);
            K key[ITEMS];
            uint32_t val[PAIRS ? ITEMS : 1];
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const uint32_t idx = seg + i * 64;
                key[i] = kin[t0 + (idx < nt ? idx : nt - 1u)];
            }
            if constexpr (PAIRS) {
#pragma unroll
                for (int i = 0; i < ITEMS; ++i) {
                    const uint32_t idx = seg + i * 64;
                    val[i] = vin[t0 + (idx < nt ? idx : nt - 1u)];
                }
            }
            // the tile grouped by the digit, stably; s_hist[d] (table 0) is then where digit d starts in the tile
            local_pass<THREADS, ITEMS, 8, PAIRS, true, K>(key, val, s_keys, s_vals, s_hist, s_tmp, shift, nt);
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const uint32_t p = seg + i * 64;
                if (p < nt) {
                    const uint32_t d = static_cast<uint32_t>(key[i] >> shift) & 255u;
                    const uint32_t at = s_base[d] + p - s_hist[d];
                    if (at < n) {  // (always, unless another workgroup rewrites the segment meanwhile: overlapping malformed ranges)
                        kout[at] = key[i];
                        if constexpr (PAIRS) vout[at] = val[i];
                    }
                }
            }
            __syncthreads();
            if (tid < 256u) s_base[tid] += (tid == 255u ? nt : s_hist[tid + 1u]) - s_hist[tid];
            __syncthreads();
        }
        cur ^= 1u;
    }
    if (cur) {  // an odd number of passes: the result is in keys_tmp
        for (size_t idx = tid; idx < n; idx += THREADS) {
            keys[b + idx] = keys_tmp[b + idx];
            if constexpr (PAIRS) values[b + idx] = values_tmp[b + idx];
        }
    }
}

__global__ __launch_bounds__(256) void segmented_publish_kernel(const SegControl *__restrict__ control, SegLists lists, uint32_t *host,
                                                                uint32_t stamp) {
    const uint32_t cnt = min(control->count[kSegListOneCall], lists.cap[kSegListOneCall]);
    for (uint32_t i = threadIdx.x; i < cnt; i += 256u) {
        const uint2 r = lists.list[kSegListOneCall][i];
        host[2u + 2u * i] = r.x;
        host[3u + 2u * i] = r.y;
    }
    if (threadIdx.x == 0u) host[1] = cnt;
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0u) __hip_atomic_store(&host[0], stamp, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <typename K, bool PAIRS>
hipError_t launch_tiers(hipStream_t stream, K *keys, K *keys_tmp, uint32_t *values, uint32_t *values_tmp, SegControl *control,
                        const SegLists &lists, const uint32_t grid[kSegLists]) {
    constexpr bool WIDE = sizeof(K) == 8;
    constexpr int WAVE_ITEMS = WIDE ? 14 : 28;
    // the block list: 32-bit keys 512 x 28, pairs 1024 x 13; 64-bit keys 1024 x 13, pairs 512 x 13
    constexpr int BLOCK_THREADS = WIDE ? (PAIRS ? 512 : 1024) : (PAIRS ? 1024 : 512), BLOCK_ITEMS = WIDE || PAIRS ? 13 : 28;
    static_assert(64 * WAVE_ITEMS >= (WIDE ? kSegWaveCapU64 : kSegWaveCap) && 256 * 16 >= kSegBlockSmallCap &&
                      static_cast<uint32_t>(BLOCK_THREADS * BLOCK_ITEMS) >= (WIDE ? (PAIRS ? kSegBlockCapPairsU64 : kSegBlockCapKeysU64)
                                                                                     : (PAIRS ? kSegBlockCapPairs : kSegBlockCapKeys)),
                  "every list's workgroup shape holds the longest segment the classification puts there");
    if (grid[kSegListWaveSmall])
        hipLaunchKernelGGL((segmented_lds_sort_kernel<K, 64, 4, PAIRS, kSegListWaveSmall>), dim3(grid[kSegListWaveSmall]), dim3(64), 0, stream,
                           keys, values, control, lists);
    if (grid[kSegListWave])
        hipLaunchKernelGGL((segmented_lds_sort_kernel<K, 64, WAVE_ITEMS, PAIRS, kSegListWave>), dim3(grid[kSegListWave]), dim3(64), 0, stream,
                           keys, values, control, lists);
    if (grid[kSegListBlockSmall])
        hipLaunchKernelGGL((segmented_lds_sort_kernel<K, 256, 16, PAIRS, kSegListBlockSmall>), dim3(grid[kSegListBlockSmall]), dim3(256), 0,
                           stream, keys, values, control, lists);
    if (grid[kSegListBlock])
        hipLaunchKernelGGL((segmented_lds_sort_kernel<K, BLOCK_THREADS, BLOCK_ITEMS, PAIRS, kSegListBlock>), dim3(grid[kSegListBlock]),
                           dim3(BLOCK_THREADS), 0, stream, keys, values, control, lists);
    if (grid[kSegListGlobal])
        hipLaunchKernelGGL((segmented_global_sort_kernel<K, PAIRS>), dim3(grid[kSegListGlobal]), dim3(1024), 0, stream, keys, keys_tmp, values,
                           values_tmp, control, lists);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_segmented(hipStream_t stream, void *keys, void *keys_tmp, uint32_t *values, uint32_t *values_tmp, uint32_t n,
                            const uint32_t *offsets, uint32_t num_segments, uint32_t one_call_min_keys, SegControl *control,
                            const SegLists &lists, const uint32_t grid[kSegLists], uint32_t *host_list, uint32_t stamp, int key_bytes) {
    hipError_t e = hipMemsetAsync(control->count, 0, sizeof(control->count), stream);
    if (e != hipSuccess) return e;
    const uint32_t blocks = static_cast<uint32_t>((static_cast<uint64_t>(num_segments) + 255u) / 256u);
    const bool pairs = values != nullptr;
    hipLaunchKernelGGL(segmented_classify_kernel, dim3(blocks), dim3(256), 0, stream, offsets, num_segments, n, pairs ? 1 : 0,
                       one_call_min_keys, control, lists, key_bytes == 8 ? 1 : 0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // (the one-call list first: the host waits for it, and the LDS tiers run while it enqueues those sorts behind them)
    if (host_list) {
        hipLaunchKernelGGL(segmented_publish_kernel, dim3(1), dim3(256), 0, stream, control, lists, host_list, stamp);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (key_bytes == 8) {
        auto *k = static_cast<uint64_t *>(keys), *kt = static_cast<uint64_t *>(keys_tmp);
        return pairs ? launch_tiers<uint64_t, true>(stream, k, kt, values, values_tmp, control, lists, grid)
                     : launch_tiers<uint64_t, false>(stream, k, kt, values, values_tmp, control, lists, grid);
    }
    auto *k = static_cast<uint32_t *>(keys), *kt = static_cast<uint32_t *>(keys_tmp);
    return pairs ? launch_tiers<uint32_t, true>(stream, k, kt, values, values_tmp, control, lists, grid)
                 : launch_tiers<uint32_t, false>(stream, k, kt, values, values_tmp, control, lists, grid);
}

}  // namespace vrs
