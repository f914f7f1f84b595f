// vrs_segmented.hip -- the segmented sorts (vrs_sort_segments_u32 / vrs_sort_segments_pairs_u32): many independent segments of one
// buffer sorted by one sequence of launches whose shapes do not depend on the segments.
//   classify: one read of the offsets; every segment gets its tier (segment_tier, the function vrs_segment_tier_for exports) and a
//     place in the work list of the workgroup shape that sorts it; per-tier counters for vrs_segmented_stats.
//   LDS tiers: one workgroup per listed segment (grids of the list's capacity, workgroups beyond the count leave at once).  The
//     segment is read once into registers, sorted by ceil(varying bits / 9) 9-bit local_pass'es from bit 0 (varying bits: the OR of
//     k ^ k_first over the segment; a constant segment is left as it is) and written once: 8 bytes of HBM traffic per key, 16 per pair.
//   global tier: one 1024-thread workgroup per segment, LSD through keys_tmp: one counting read of all four digits, then a stable
//     tile-by-tile scatter per digit that is not the same for every key, and the copy home after an odd number of passes.
//   publish: the one-call tier's list goes to pinned host memory, stamped last; the host sorts those segments with the one-call sort.
#include "vrs_segmented.hpp"

#include "vrs_local_sort.hpp"

namespace vrs {
namespace {

__global__ __launch_bounds__(256) void segmented_classify_kernel(const uint32_t *__restrict__ offsets, uint32_t num_segments, uint32_t n,
                                                                 int pairs, uint32_t one_call_min_keys, SegControl *__restrict__ control,
                                                                 SegLists lists) {
    __shared__ uint32_t s_cnt[kSegLists], s_base[kSegLists], s_stat[4];
    const uint32_t tid = threadIdx.x;
    if (tid < kSegLists) s_cnt[tid] = 0u;
    if (tid < 4u) s_stat[tid] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + tid;
    int list = -1;
    uint32_t pos = 0, cb = 0, ce = 0;
    if (i < num_segments) {
        const int tier = segment_tier(offsets[i], offsets[i + 1u], n, pairs != 0, one_call_min_keys, &cb, &ce);
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

// One listed segment of up to THREADS * ITEMS keys (pairs) sorted in LDS by its varying bits.
template <int THREADS, int ITEMS, bool PAIRS, int LIST>
__global__ __launch_bounds__(THREADS) void segmented_lds_sort_kernel(uint32_t *__restrict__ keys, uint32_t *__restrict__ values,
                                                                     const SegControl *__restrict__ control, SegLists lists) {
    constexpr int WAVES = THREADS / 64, CAP = THREADS * ITEMS;
    __shared__ uint32_t s_keys[CAP];
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
    const uint32_t *src = keys + b;
    uint32_t key[ITEMS], val[PAIRS ? ITEMS : 1];
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
    const uint32_t k0 = src[0];
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) diff |= key[i] ^ k0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) diff |= __shfl_xor(diff, o);
    if constexpr (WAVES > 1) {
        if (lane == 0u) s_tmp[wave] = diff;
        __syncthreads();
#pragma unroll
        for (int v = 0; v < WAVES; ++v) diff |= s_tmp[v];
    }
    if (diff == 0u) return;  // a constant segment: nothing to sort, nothing to store
    const uint32_t width = 32u - static_cast<uint32_t>(__clz(diff));
    uint32_t shift = 0;
    if constexpr (!PAIRS) {  // bare keys: ties of the first digit in any order (the later passes or equality tell them apart)
        local_pass<THREADS, ITEMS, 9, false, false>(key, val, s_keys, nullptr, s_hist, s_tmp, 0u, n);
        shift = 9u;
    }
    for (; shift < width; shift += 9u) local_pass<THREADS, ITEMS, 9, PAIRS, true>(key, val, s_keys, s_vals, s_hist, s_tmp, shift, n);
    uint32_t *dst = keys + b;
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

// One listed segment of any length sorted by one workgroup through keys_tmp (stable).
template <bool PAIRS>
__global__ __launch_bounds__(1024) void segmented_global_sort_kernel(uint32_t *__restrict__ keys, uint32_t *__restrict__ keys_tmp,
                                                                     uint32_t *__restrict__ values, uint32_t *__restrict__ values_tmp,
                                                                     const SegControl *__restrict__ control, SegLists lists) {
    constexpr int THREADS = 1024, ITEMS = 8, TILE = THREADS * ITEMS, WAVES = THREADS / 64;
    __shared__ uint32_t s_keys[TILE];
    __shared__ uint32_t s_vals[PAIRS ? TILE : 1];
    __shared__ uint32_t s_hist[WAVES * 256];
    __shared__ uint32_t s_tmp[WAVES];
    __shared__ uint32_t s_cnt[4 * 256];
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_same[4];  // digit j is the same in every key: its pass is the identity
    const uint32_t count = min(control->count[kSegListGlobal], lists.cap[kSegListGlobal]);
    if (blockIdx.x >= count) return;
    const uint2 range = lists.list[kSegListGlobal][blockIdx.x];
    const uint32_t b = range.x, n = range.y - range.x;
    if (n < 2u) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    s_cnt[tid] = 0u;
    if (tid < 4u) s_same[tid] = 0u;
    __syncthreads();
    for (uint32_t idx = tid; idx < n; idx += THREADS) {
        const uint32_t k = keys[b + idx];
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(&s_cnt[j * 256 + ((k >> (8 * j)) & 255u)], 1u);
    }
    __syncthreads();
    if (s_cnt[tid] == n) s_same[tid >> 8] = 1u;
    __syncthreads();
    const uint32_t seg = wave * (ITEMS * 64) + lane;
    uint32_t cur = 0;  // 0: the keys are in `keys`, 1: in `keys_tmp`
    for (uint32_t j = 0; j < 4u; ++j) {
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
        const uint32_t *kin = (cur ? keys_tmp : keys) + b;
        uint32_t *kout = (cur ? keys : keys_tmp) + b;
        const uint32_t *vin = PAIRS ? (cur ? values_tmp : values) + b : nullptr;
        uint32_t *vout = PAIRS ? (cur ? values : values_tmp) + b : nullptr;
        for (uint32_t t0 = 0; t0 < n; t0 += TILE) {
            const uint32_t nt = min(static_cast<uint32_t>(TILE), n - t0);
            uint32_t key[ITEMS], val[PAIRS ? ITEMS : 1];
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
            local_pass<THREADS, ITEMS, 8, PAIRS, true>(key, val, s_keys, s_vals, s_hist, s_tmp, shift, nt);
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const uint32_t p = seg + i * 64;
                if (p < nt) {
                    const uint32_t d = (key[i] >> shift) & 255u;
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
        for (uint32_t idx = tid; idx < n; idx += THREADS) {
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

template <bool PAIRS>
hipError_t launch_tiers(hipStream_t stream, uint32_t *keys, uint32_t *keys_tmp, uint32_t *values, uint32_t *values_tmp,
                        SegControl *control, const SegLists &lists, const uint32_t grid[kSegLists]) {
    if (grid[kSegListWaveSmall])
        hipLaunchKernelGGL((segmented_lds_sort_kernel<64, 4, PAIRS, kSegListWaveSmall>), dim3(grid[kSegListWaveSmall]), dim3(64), 0, stream, keys,
                           values, control, lists);
    if (grid[kSegListWave])
        hipLaunchKernelGGL((segmented_lds_sort_kernel<64, 28, PAIRS, kSegListWave>), dim3(grid[kSegListWave]), dim3(64), 0, stream, keys, values,
                           control, lists);
    if (grid[kSegListBlockSmall])
        hipLaunchKernelGGL((segmented_lds_sort_kernel<256, 16, PAIRS, kSegListBlockSmall>), dim3(grid[kSegListBlockSmall]), dim3(256), 0, stream,
                           keys, values, control, lists);
    if (grid[kSegListBlock]) {
        if constexpr (PAIRS)
            hipLaunchKernelGGL((segmented_lds_sort_kernel<1024, 13, true, kSegListBlock>), dim3(grid[kSegListBlock]), dim3(1024), 0, stream, keys,
                               values, control, lists);
        else
            hipLaunchKernelGGL((segmented_lds_sort_kernel<512, 28, false, kSegListBlock>), dim3(grid[kSegListBlock]), dim3(512), 0, stream, keys,
                               values, control, lists);
    }
    if (grid[kSegListGlobal])
        hipLaunchKernelGGL(segmented_global_sort_kernel<PAIRS>, dim3(grid[kSegListGlobal]), dim3(1024), 0, stream, keys, keys_tmp, values,
                           values_tmp, control, lists);
    return hipGetLastError();
}

static_assert(64 * 28 >= kSegWaveCap && 256 * 16 >= kSegBlockSmallCap && 512 * 28 >= kSegBlockCapKeys && 1024 * 13 >= kSegBlockCapPairs,
              "every list's workgroup shape holds the longest segment the classification puts there");

}  // namespace

hipError_t launch_segmented(hipStream_t stream, uint32_t *keys, uint32_t *keys_tmp, uint32_t *values, uint32_t *values_tmp, uint32_t n,
                            const uint32_t *offsets, uint32_t num_segments, uint32_t one_call_min_keys, SegControl *control,
                            const SegLists &lists, const uint32_t grid[kSegLists], uint32_t *host_list, uint32_t stamp) {
    hipError_t e = hipMemsetAsync(control->count, 0, sizeof(control->count), stream);
    if (e != hipSuccess) return e;
    const uint32_t blocks = static_cast<uint32_t>((static_cast<uint64_t>(num_segments) + 255u) / 256u);
    const bool pairs = values != nullptr;
    hipLaunchKernelGGL(segmented_classify_kernel, dim3(blocks), dim3(256), 0, stream, offsets, num_segments, n, pairs ? 1 : 0,
                       one_call_min_keys, control, lists);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // (the one-call list first: the host waits for it, and the LDS tiers run while it enqueues those sorts behind them)
    if (host_list) {
        hipLaunchKernelGGL(segmented_publish_kernel, dim3(1), dim3(256), 0, stream, control, lists, host_list, stamp);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return pairs ? launch_tiers<true>(stream, keys, keys_tmp, values, values_tmp, control, lists, grid)
                 : launch_tiers<false>(stream, keys, keys_tmp, values, values_tmp, control, lists, grid);
}

}  // namespace vrs
