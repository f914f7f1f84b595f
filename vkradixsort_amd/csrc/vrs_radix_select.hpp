// vrs_radix_select.hpp -- the device pieces the two radix selections share (vrs_topk.hip: the k first keys; vrs_select.hip: one key): the
// digit histogram's add, the pick of the digit that holds the need-th key, and the grid tier's tile -> slot search.  Internal.
#pragma once
#include "vrs_device.hpp"
#include "vrs_topk.hpp"

namespace vrs {

constexpr uint32_t kRadixSelectBins = kTopkBins;  // digits of up to 11 bits

// counts digit d of the calling lane; one add for the whole instruction when every active lane has the same digit (equal keys)
__device__ __forceinline__ void hist_add(uint32_t *s_hist, uint32_t d) {
    const uint32_t d0 = __builtin_amdgcn_readfirstlane(d);
    const uint64_t active = __ballot(1);
    if (__ballot(d == d0) == active) {
        if (count_below(active) == 0u) atomicAdd(&s_hist[d0], static_cast<uint32_t>(__popcll(active)));
    } else {
        atomicAdd(&s_hist[d], 1u);
    }
}

// Picks the digit that holds the need-th matching key (1 <= need <= keys counted): s_res = {d*, keys below it, keys at it}.
template <int THREADS>
__device__ __forceinline__ void select_digit(const uint32_t *s_hist, uint32_t need, uint32_t *s_wtot, uint32_t *s_res) {
    constexpr int PER = static_cast<int>(kRadixSelectBins) / THREADS, WAVES = THREADS / 64;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t c[PER], sum = 0;
#pragma unroll
    for (int p = 0; p < PER; ++p) {
        c[p] = s_hist[tid * PER + p];
        sum += c[p];
    }
    uint32_t incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o);
        if (lane >= static_cast<uint32_t>(o)) incl += t;
    }
    if (lane == 63u) s_wtot[wave] = incl;
    __syncthreads();
    uint32_t excl = incl - sum;
#pragma unroll
    for (int v = 0; v < WAVES; ++v) excl += static_cast<uint32_t>(v) < wave ? s_wtot[v] : 0u;
    if (excl < need && need <= excl + sum) {  // exactly one thread
        uint32_t acc = excl;
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            if (acc + c[p] >= need) {
                s_res[0] = tid * PER + p;
                s_res[1] = acc;
                s_res[2] = c[p];
                break;
            }
            acc += c[p];
        }
    }
    __syncthreads();
}

// the grid slots / virtual tiles a call's classification took, cut to what the scratch buffer holds
__device__ __forceinline__ uint32_t grid_slots(const TopkControl *ctl, uint32_t slot_cap) {
    return min(static_cast<uint32_t>(ctl->grid_packed), slot_cap);
}
__device__ __forceinline__ uint32_t grid_tiles(const TopkControl *ctl, uint32_t slot_cap, uint32_t tile_cap) {
    const uint32_t ns = grid_slots(ctl, slot_cap);
    return ns == 0u ? 0u : min(static_cast<uint32_t>(ctl->grid_packed >> 32), tile_cap);
}
// the slot whose tiles hold virtual tile t: the last slot with tile_base <= t (tile bases grow with the slot)
template <class Slot>
__device__ __forceinline__ uint32_t find_slot(const Slot *slots, uint32_t ns, uint32_t t) {
    uint32_t lo = 0, hi = ns;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) / 2u;
        if (slots[mid].tile_base <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace vrs
