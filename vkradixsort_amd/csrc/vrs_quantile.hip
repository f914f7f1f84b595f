// vrs_quantile.hip -- multi-rank selection (vrs_quantile_segments): the values of up to 16 entries of every segment's ascending order by
// radix select, carried through one sequence of reads, and the quantiles interpolated from them (vrs_quantile_order.hpp).  Values only:
// a finished target's value is the inverse rank map of its prefix, no walk looks for an index.  Templates: S, the element as the unsigned
// integer of its width (float32: uint32_t, float64: uint64_t), which is also its rank's type.
//   classify: top-k's bookkeeping -- one thread per segment; its tier (select_tier), a place on the LDS tier's list (front of one array)
//     or the BLOCK tier's (back of it), or a grid slot with a range of tiles; per-tier counters.
//   selection (quantile_level): level 0 counts the top 11 bits of every key in one histogram, and the NaN class; only then are the
//     targets known (quantile_target), sorted and deduplicated.  Each target falls into a bin; targets in one bin are one group.  A later
//     level counts, in one read of its source, the next 8 bits (the last level: what is left) of every key whose higher bits equal a live
//     group's: one histogram of 256 bins per group, 16 groups in 16 KB of LDS.  A level ends with one wave per group scanning the group's
//     histogram in place and the first wave, one lane per target, searching it and regrouping the targets by their longer prefixes.
//   LDS tier (ranks of up to 32 KB): one 256-thread workgroup per segment, ranks read once into LDS.
//   BLOCK tier: one 1024-thread workgroup per segment streaming 16384-key tiles: one read of the row per level, whatever M is.
//   GRID tier: each phase one launch over a fixed grid that walks the tiles of every grid slot, histograms in scratch.  After a level
//     whose live groups together hold at most len / VRS_TUNE_SELECT_COMPACT_DIVISOR keys (and fit the slot's area), with two levels or
//     more still to come, one walk copies the ranks of all live groups' keys into the slot's area (a ballot and one cursor atomic per
//     wave); the later levels read the copy.
// No kernel waits on another workgroup.  Loops whose bound may come near 2^32 (grid strides, a segment's tiles) count in 64 bits.
#include "vrs_quantile.hpp"

#include "vrs_radix_select.hpp"

namespace vrs {
namespace {

template <typename S>
struct FloatOf;
template <>
struct FloatOf<uint32_t> {
    using type = float;
    static constexpr uint32_t inf_bits = 0x7F800000u;
};
template <>
struct FloatOf<uint64_t> {
    using type = double;
    static constexpr uint64_t inf_bits = 0x7FF0000000000000ull;
};

template <typename S>
__device__ __forceinline__ S quant_rank(S x) {
    return select_rank<S, 8 * static_cast<int>(sizeof(S))>(x, kSelFloat, FloatOf<S>::inf_bits, false);
}
// the value of a finished prefix; the merged classes answer their canonical member: +0.0 for either zero, the quiet NaN
template <typename S>
__device__ __forceinline__ typename FloatOf<S>::type quant_value(S r) {
    using T = typename FloatOf<S>::type;
    bool exact;
    const S bits = sort_unrank<S, 8 * static_cast<int>(sizeof(S)), true, false>(r, false, &exact);
    if (!exact) return r == static_cast<S>(~static_cast<S>(0)) ? quantile_nan<T>() : static_cast<T>(0);
    return __builtin_bit_cast(T, bits);
}

// inclusive scan, in place, of the `bins` counts at h (a power of two) by one whole wave
__device__ __forceinline__ void quant_wave_scan(uint32_t *h, uint32_t bins, uint32_t lane) {
    const uint32_t per = bins > 64u ? bins / 64u : 1u, base = lane * per;
    uint32_t sum = 0;
    if (base < bins)
        for (uint32_t i = 0; i < per; ++i) sum += h[base + i];
    uint32_t incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o);
        if (lane >= static_cast<uint32_t>(o)) incl += t;
    }
    uint32_t run = incl - sum;
    if (base < bins)
        for (uint32_t i = 0; i < per; ++i) {
            run += h[base + i];
            h[base + i] = run;
        }
}

// The targets of a segment of len keys, nans of them NaN, into s, by one whole wave: lane c holds side c & 1 of q number c >> 1 (32
// candidates at the most; a single-entry mode's two sides are equal); the distinct ones, ascending, become the targets -- a candidate is
// kept when no earlier lane has its entry, and its place is the number of kept entries below it.  All in one group that matches every
// key.  false (in every lane): the segment has no answer.
template <typename T>
__device__ __forceinline__ bool quant_targets(const QuantileArgs &a, uint32_t len, uint32_t nans, QuantState &s, uint32_t lane) {
    const uint32_t cands = 2u * a.num_q;
    const bool act = lane < cands;
    uint32_t e[2] = {0u, 0u};
    T w;
    const bool ok = quantile_target<T>(a.interpolation, a.q[act ? lane >> 1 : 0u], len, nans, (a.flags & kQuantIgnoreNan) != 0, &e[0], &e[1], &w);
    if (!ok) return false;  // (the same for every q: it depends on len, nans and the flag alone)
    const uint32_t v = (lane & 1u) ? e[1] : e[0];
    bool kept = act;
    for (uint32_t j = 0; j < cands; ++j) {
        const uint32_t vj = __shfl(v, static_cast<int>(j));
        if (j < lane && vj == v) kept = false;
    }
    uint32_t at = 0;
    for (uint32_t j = 0; j < cands; ++j) {
        const uint32_t vj = __shfl(v, static_cast<int>(j));
        const int kj = __shfl(kept ? 1 : 0, static_cast<int>(j));
        if (kj && vj < v) ++at;
    }
    const uint32_t M = static_cast<uint32_t>(__popcll(__ballot(kept)));
    if (kept && at < kQuantMaxTargets) {  // (at most 16 distinct entries: num_q * sides <= 16, the call was refused otherwise)
        s.entry[at] = v;
        s.need[at] = v + 1u;
        s.prefix[at] = 0ull;
        s.group[at] = 0u;
    }
    if (lane == 0u) {
        s.M = min(M, kQuantMaxTargets);
        s.G = 1u;
        s.gprefix[0] = 0ull;
        s.shift = kSelNoShift;
        s.live = len;
    }
    return true;
}

// The digit histograms of level `level` of one tile; position p of the tile: load(p).  Level 0: every key, into bins [0, 2048); later:
// the keys whose bits from s.shift up equal a live group's, into the group's 256 bins.  Returns the calling thread's keys of the NaN
// class when `nans` asks for them.
template <int THREADS, int ITEMS, typename S, class Load>
__device__ __forceinline__ uint32_t quant_hist_tile(Load load, uint32_t cnt, const QuantState &s, int level, uint32_t shift, uint32_t mask, bool nans,
                                                    uint32_t *s_hist) {
    S r[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = i * THREADS + threadIdx.x;
        r[i] = p < cnt ? load(p) : static_cast<S>(0);
    }
    uint32_t nn = 0;
    if (level == 0) {
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t p = i * THREADS + threadIdx.x;
            if (p < cnt) {
                if (nans && r[i] == static_cast<S>(~static_cast<S>(0))) ++nn;
                hist_add(s_hist, static_cast<uint32_t>(r[i] >> shift) & mask);
            }
        }
        return nn;
    }
    const uint32_t G = s.G, pshift = s.shift;
    const S gmin = static_cast<S>(s.gprefix[0]), gmax = static_cast<S>(s.gprefix[G - 1u]);
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = i * THREADS + threadIdx.x;
        const S hi = r[i] >> pshift;
        if (p < cnt && hi >= gmin && hi <= gmax) {
            for (uint32_t g = 0; g < G; ++g)
                if (static_cast<S>(s.gprefix[g]) == hi) {
                    hist_add(s_hist, g * kQuantSubBins + (static_cast<uint32_t>(r[i] >> shift) & mask));
                    break;
                }
        }
    }
    return nn;
}

template <typename S>
__device__ __forceinline__ bool quant_match(S r, const QuantState &s) {
    const S hi = r >> s.shift;
    bool m = false;
    for (uint32_t g = 0; g < s.G; ++g) m = m || static_cast<S>(s.gprefix[g]) == hi;
    return m;
}

// After level `level`'s histograms are complete (and a barrier): every target's digit, its rank within the chosen bin and its longer
// prefix; then the groups again.  s is in LDS.  Ends with a barrier.
template <int THREADS>
__device__ __forceinline__ void quant_resolve(QuantState &s, uint32_t *s_hist, int bits, int level) {
    constexpr uint32_t WAVES = THREADS / 64;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t shift, mask;
    quantile_level(bits, level, &shift, &mask);
    const uint32_t bins = mask + 1u, G = level == 0 ? 1u : s.G, M = s.M;
    for (uint32_t g = wave; g < G; g += WAVES) quant_wave_scan(s_hist + g * kQuantSubBins, bins, lane);
    __syncthreads();
    if (wave == 0u) {  // the whole first wave: lane m is target m (M <= 16), the other lanes carry nothing
        const bool act = lane < M;
        unsigned long long p = ~0ull;  // the target's longer prefix >> shift
        uint32_t at = 0;               // keys in its chosen bin
        if (act) {
            const uint32_t *h = s_hist + (level == 0 ? 0u : s.group[lane] * kQuantSubBins);
            const uint32_t need = s.need[lane];
            uint32_t lo = 0, hi = bins - 1u;  // the first bin whose inclusive count reaches need
            while (lo < hi) {
                const uint32_t mid = (lo + hi) / 2u;
                if (h[mid] >= need) hi = mid;
                else lo = mid + 1u;
            }
            const uint32_t below = lo ? h[lo - 1u] : 0u;
            const unsigned long long np = s.prefix[lane] | (static_cast<unsigned long long>(lo) << shift);
            s.need[lane] = need - below;
            s.prefix[lane] = np;
            p = np >> shift;
            at = h[lo] - below;
        }
        // the groups again: the targets ascend, so a group begins where the prefix differs from the target's before
        const unsigned long long before = __shfl_up(p, 1);
        const bool first = act && (lane == 0u || p != before);
        const uint64_t firsts = __ballot(first);
        if (act) {
            const uint32_t g = static_cast<uint32_t>(__popcll(firsts & ((2ull << lane) - 1ull))) - 1u;
            s.group[lane] = g;
            if (first) s.gprefix[g] = p;
        }
        uint32_t live = first ? at : 0u;  // a group's keys: its chosen bin's, counted once
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) live += __shfl_xor(live, o);
        if (lane == 0u) {
            s.G = static_cast<uint32_t>(__popcll(firsts));
            s.live = live;
            s.shift = shift;
        }
    }
    __syncthreads();
}

// q number i of segment seg into the outputs: the two entries' values, the weight and the interpolated quantile; NaN everywhere for a
// segment without an answer
template <typename S>
__device__ __forceinline__ void quant_write(const QuantileArgs &a, uint32_t seg, uint32_t i, uint32_t len, uint32_t nans, bool ok, const QuantState &s) {
    using T = typename FloatOf<S>::type;
    T lo_v = quantile_nan<T>(), hi_v = lo_v, w = lo_v, v = lo_v;
    uint32_t lo, hi;
    if (ok && quantile_target<T>(a.interpolation, a.q[i], len, nans, (a.flags & kQuantIgnoreNan) != 0, &lo, &hi, &w)) {
        for (uint32_t m = 0; m < s.M; ++m) {
            if (s.entry[m] == lo) lo_v = quant_value<S>(static_cast<S>(s.prefix[m]));
            if (s.entry[m] == hi) hi_v = quant_value<S>(static_cast<S>(s.prefix[m]));
        }
        v = quantile_lerp<T>(a.interpolation, lo_v, hi_v, w);
    } else {
        w = quantile_nan<T>();
    }
    const size_t at = static_cast<size_t>(seg) * a.num_q + i;
    static_cast<T *>(a.out_values)[at] = v;
    if (a.out_lower) static_cast<T *>(a.out_lower)[at] = lo_v;
    if (a.out_upper) static_cast<T *>(a.out_upper)[at] = hi_v;
    if (a.out_weight) static_cast<T *>(a.out_weight)[at] = w;
}

__global__ __launch_bounds__(256) void quantile_classify_kernel(QuantileArgs a, TopkControl *__restrict__ ctl, uint32_t *__restrict__ list,
                                                                QuantSlot *__restrict__ slots, uint32_t slot_cap, uint32_t tile_cap) {
    __shared__ uint32_t s_stat[3];
    const uint32_t tid = threadIdx.x;
    if (tid < 3u) s_stat[tid] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + tid;
    if (i < a.num_segments) {
        uint32_t cb, ce;
        int tier = select_tier(a.offsets[i], a.offsets[i + 1u], a.n, a.dtype, a.grid_min_keys, &cb, &ce);
        atomicAdd(&s_stat[tier], 1u);
        const uint32_t len = ce - cb;
        if (tier == kTopkTierGrid) {
            const uint32_t tiles = static_cast<uint32_t>((static_cast<uint64_t>(len) + kTopkTile - 1u) / kTopkTile);  // (len + 16383 wraps near 2^32)
            const unsigned long long old = atomicAdd(&ctl->grid_packed, (static_cast<unsigned long long>(tiles) << 32) | 1ull);
            const uint32_t slot = static_cast<uint32_t>(old), base = static_cast<uint32_t>(old >> 32);
            bool valid = false;
            if (slot < slot_cap) {  // (beyond the caps: overlapping ranges, or more long segments than n / 8193; the BLOCK kernel takes them)
                valid = static_cast<uint64_t>(base) + tiles <= tile_cap;
                QuantSlot *s = &slots[slot];
                s->seg = i;
                s->b = cb;
                s->len = len;
                s->tile_base = base;
                s->tiles = tiles;
                s->valid = valid ? 1u : 0u;
                s->ok = 1u;
                s->nans = 0u;
                s->state = 0u;
                s->ccount = 0u;
                s->cursor = 0u;
                s->q.M = 0u;
                s->q.G = 1u;
                s->q.shift = kSelNoShift;
                s->q.gprefix[0] = 0ull;
            }
            if (!valid) tier = kTopkTierBlock;
        }
        if (tier == kTopkTierLds) list[atomicAdd(&ctl->lds_count, 1u)] = i;
        else if (tier == kTopkTierBlock) list[a.num_segments - 1u - atomicAdd(&ctl->block_count, 1u)] = i;
    }
    __syncthreads();
    if (tid < 3u && s_stat[tid] != 0u) atomicAdd(&a.stats[tid], static_cast<unsigned long long>(s_stat[tid]));
}

// LDS and BLOCK tiers: one workgroup per listed segment (the workgroups walk the list).  LDS: the ranks are read once into LDS.
template <typename S, int THREADS, int ITEMS, bool LDS>
__global__ __launch_bounds__(THREADS) void quantile_workgroup_kernel(QuantileArgs a, const TopkControl *__restrict__ ctl, const uint32_t *__restrict__ list) {
    using T = typename FloatOf<S>::type;
    constexpr int B = 8 * static_cast<int>(sizeof(S)), LEVELS = quantile_levels(B), TILE = THREADS * ITEMS;
    static_assert(!LDS || TILE * sizeof(S) == kSelLdsBytes, "the LDS tier's segment is one tile");
    __shared__ uint32_t s_hist[kQuantHistWords];
    __shared__ S s_r[LDS ? TILE : 1];
    __shared__ QuantState s_q;
    __shared__ uint32_t s_nans, s_ok;
    const uint32_t tid = threadIdx.x;
    const uint32_t count = LDS ? ctl->lds_count : ctl->block_count;
    for (size_t jw = blockIdx.x; jw < count; jw += gridDim.x) {
        const uint32_t j = static_cast<uint32_t>(jw);
        const uint32_t seg = LDS ? list[j] : list[a.num_segments - 1u - j];
        uint32_t b, e;
        (void)topk_tier(a.offsets[seg], a.offsets[seg + 1u], a.n, 0u, &b, &e);
        const uint32_t len = e - b;
        const S *src = static_cast<const S *>(a.src) + b;
        if (tid == 0u) {
            s_nans = 0u;
            s_ok = len != 0u ? 1u : 0u;
        }
        __syncthreads();
        if (len != 0u) {
            if constexpr (LDS) {
                uint32_t nn = 0;
                for (uint32_t p = tid; p < len; p += THREADS) {
                    const S r = quant_rank<S>(src[p]);
                    s_r[p] = r;
                    if (r == static_cast<S>(~static_cast<S>(0))) ++nn;
                }
                if (nn != 0u) atomicAdd(&s_nans, nn);
                __syncthreads();
            }
            for (int level = 0; level < LEVELS; ++level) {
                const uint32_t words = level == 0 ? kTopkBins : s_q.G * kQuantSubBins;
                for (uint32_t c = tid; c < words; c += THREADS) s_hist[c] = 0u;
                __syncthreads();
                uint32_t shift, mask, nn = 0;
                quantile_level(B, level, &shift, &mask);
                for (uint64_t tile0 = 0; tile0 < len; tile0 += TILE) {  // (64-bit: a 32-bit t0 + TILE wraps below len near 2^32)
                    const uint32_t t0 = static_cast<uint32_t>(tile0), cnt = min(static_cast<uint32_t>(TILE), len - t0);
                    if constexpr (LDS)
                        (void)quant_hist_tile<THREADS, ITEMS, S>([&](uint32_t p) { return s_r[t0 + p]; }, cnt, s_q, level, shift, mask, false, s_hist);
                    else
                        nn += quant_hist_tile<THREADS, ITEMS, S>([&](uint32_t p) { return quant_rank<S>(src[t0 + p]); }, cnt, s_q, level, shift, mask,
                                                                 level == 0, s_hist);
                }
                if (nn != 0u) atomicAdd(&s_nans, nn);
                __syncthreads();
                if (level == 0) {  // the targets: known once the first read has counted the NaN class
                    if (tid < 64u) {
                        const bool ok = quant_targets<T>(a, len, s_nans, s_q, tid);
                        if (tid == 0u) s_ok = ok ? 1u : 0u;
                    }
                    __syncthreads();
                    if (!s_ok) break;
                }
                quant_resolve<THREADS>(s_q, s_hist, B, level);
            }
        }
        if (tid < a.num_q) quant_write<S>(a, seg, tid, len, s_nans, s_ok != 0u, s_q);
        __syncthreads();  // (s_nans, s_ok and s_q are read before the next segment sets them)
    }
}

// ---- GRID tier: kernels that walk the virtual tiles [0, tiles taken) of every slot ----
constexpr int kGridThreads = 1024, kGridItems = 16;
static_assert(kGridThreads * kGridItems == static_cast<int>(kTopkTile), "a grid tile is one pass of a workgroup");
constexpr uint32_t kStateWords = sizeof(QuantState) / 4u;

__global__ __launch_bounds__(256) void quantile_grid_init_kernel(const TopkControl *__restrict__ ctl, uint32_t *__restrict__ hist, uint32_t slot_cap) {
    const uint32_t ns = grid_slots(ctl, slot_cap);
    for (size_t s = blockIdx.x; s < ns; s += gridDim.x)
        for (uint32_t c = threadIdx.x; c < kQuantHistWords; c += 256u) hist[s * kQuantHistWords + c] = 0u;
}

constexpr int kWalkHist = 0, kWalkSieve = 1;

// PHASE kWalkHist: digit histograms of level `level` (of src, or of a sieved slot's area; level 0 also counts the NaN class);
// kWalkSieve: the ranks of the live groups' keys of every slot that has just qualified, into its area
template <typename S, int PHASE>
__global__ __launch_bounds__(kGridThreads) void quantile_grid_walk_kernel(QuantileArgs a, const TopkControl *__restrict__ ctl, QuantSlot *slots,
                                                                          uint32_t *__restrict__ hist, S *__restrict__ area, uint32_t slot_cap,
                                                                          uint32_t tile_cap, int level) {
    constexpr int B = 8 * static_cast<int>(sizeof(S));
    __shared__ uint32_t s_hist[PHASE == kWalkHist ? kQuantHistWords : 1];
    __shared__ QuantState s_q;
    __shared__ uint32_t s_slot, s_nans;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t ns = grid_slots(ctl, slot_cap), total = grid_tiles(ctl, slot_cap, tile_cap);
    if constexpr (PHASE == kWalkHist) {
        for (uint32_t c = tid; c < kQuantHistWords; c += kGridThreads) s_hist[c] = 0u;
        if (tid == 0u) s_nans = 0u;
    }
    uint32_t cur = 0xFFFFFFFFu;
    bool dirty = false;
    auto flush = [&]() {  // the workgroup's counts of slot `cur` into the slot's: one atomic per non-zero bin
        __syncthreads();
        if constexpr (PHASE == kWalkHist) {
            for (uint32_t c = tid; c < kQuantHistWords; c += kGridThreads) {
                const uint32_t v = s_hist[c];
                if (v != 0u) {
                    atomicAdd(&hist[static_cast<size_t>(cur) * kQuantHistWords + c], v);
                    s_hist[c] = 0u;
                }
            }
            if (tid == 0u && s_nans != 0u) {
                atomicAdd(&slots[cur].nans, s_nans);
                s_nans = 0u;
            }
        }
        __syncthreads();
    };
    for (size_t tw = blockIdx.x; tw < total; tw += gridDim.x) {
        const uint32_t t = static_cast<uint32_t>(tw);
        if (tid == 0u) s_slot = find_slot(slots, ns, t);
        __syncthreads();
        const uint32_t s = s_slot;
        __syncthreads();
        if (s != cur) {
            if (dirty) {
                flush();
                dirty = false;
            }
            cur = s;
            if (tid < kStateWords) reinterpret_cast<uint32_t *>(&s_q)[tid] = reinterpret_cast<const uint32_t *>(&slots[s].q)[tid];
            __syncthreads();
        }
        const QuantSlot *sl = &slots[s];
        const uint32_t ti = t - sl->tile_base, len = sl->len;
        if (!sl->valid || !sl->ok || ti >= sl->tiles) continue;
        const uint32_t off = ti * kTopkTile;  // (below len)
        const S *src = static_cast<const S *>(a.src) + sl->b + off;
        auto load = [&](uint32_t p) { return quant_rank<S>(src[p]); };
        if constexpr (PHASE == kWalkHist) {
            uint32_t shift, mask;
            quantile_level(B, level, &shift, &mask);
            if (sl->state != 0u) {  // sieved: its first ccount / 16384 tiles stand for the area's
                const uint32_t have = sl->ccount;
                if (off >= have) continue;
                const S *ar = area + static_cast<size_t>(sl->tile_base) * kSelAreaPerTile + off;
                (void)quant_hist_tile<kGridThreads, kGridItems, S>([&](uint32_t p) { return ar[p]; }, min(kTopkTile, have - off), s_q, level, shift, mask,
                                                                   false, s_hist);
            } else {
                const uint32_t nn = quant_hist_tile<kGridThreads, kGridItems, S>(load, min(kTopkTile, len - off), s_q, level, shift, mask, level == 0, s_hist);
                if (nn != 0u) atomicAdd(&s_nans, nn);
            }
            dirty = true;
        } else {
            if (sl->state != 1u) continue;
            const uint32_t cnt = min(kTopkTile, len - off), room = sl->ccount;
            S *ar = area + static_cast<size_t>(sl->tile_base) * kSelAreaPerTile;
            S r[kGridItems];
#pragma unroll
            for (int i = 0; i < kGridItems; ++i) {
                const uint32_t p = i * kGridThreads + tid;
                r[i] = p < cnt ? load(p) : static_cast<S>(0);
            }
            uint32_t mine = 0, wave_total = 0;  // bit i of mine: this lane's item i is in a live group
#pragma unroll
            for (int i = 0; i < kGridItems; ++i) {
                const uint32_t p = i * kGridThreads + tid;
                const bool m = p < cnt && quant_match<S>(r[i], s_q);
                mine |= m ? 1u << i : 0u;
                wave_total += static_cast<uint32_t>(__popcll(__ballot(m)));
            }
            if (wave_total != 0u) {  // (the same in every lane of the wave)
                uint32_t base = 0;
                if (lane == 0u) base = atomicAdd(&slots[s].cursor, wave_total);
                base = __shfl(base, 0);
#pragma unroll
                for (int i = 0; i < kGridItems; ++i) {
                    const bool m = (mine >> i) & 1u;
                    const uint64_t bal = __ballot(m);
                    const uint32_t at = base + count_below(bal);
                    if (m && at < room) ar[at] = r[i];  // (at < room unless src changed under the call)
                    base += static_cast<uint32_t>(__popcll(bal));
                }
            }
        }
    }
    if (dirty) flush();
}

// One workgroup per slot: level `level`'s digits from the slot's histograms (zeroed behind it for the next level); at level 0 the
// targets from the NaN count first; after the last level the outputs.  A slot whose live groups are small enough (and fit its area)
// sieves after this level.
template <typename S>
__global__ __launch_bounds__(256) void quantile_grid_select_kernel(QuantileArgs a, const TopkControl *__restrict__ ctl, QuantSlot *__restrict__ slots,
                                                                   uint32_t *__restrict__ hist, uint32_t slot_cap, int level) {
    using T = typename FloatOf<S>::type;
    constexpr int B = 8 * static_cast<int>(sizeof(S)), LEVELS = quantile_levels(B);
    __shared__ uint32_t s_hist[kQuantHistWords];
    __shared__ QuantState s_q;
    __shared__ uint32_t s_ok;
    const uint32_t tid = threadIdx.x;
    const uint32_t ns = grid_slots(ctl, slot_cap);
    for (size_t sw = blockIdx.x; sw < ns; sw += gridDim.x) {
        QuantSlot *sl = &slots[sw];
        const uint32_t len = sl->len, nans = sl->nans, state = sl->state, seg = sl->seg, tiles = sl->tiles;
        if (!sl->valid || !sl->ok) continue;
        if (tid < kStateWords) reinterpret_cast<uint32_t *>(&s_q)[tid] = reinterpret_cast<const uint32_t *>(&sl->q)[tid];
        __syncthreads();
        if (level == 0) {
            if (tid < 64u) {
                const bool ok = quant_targets<T>(a, len, nans, s_q, tid);
                if (tid == 0u) s_ok = ok ? 1u : 0u;
            }
            __syncthreads();
        } else if (tid == 0u) {
            s_ok = 1u;
        }
        uint32_t *h = hist + sw * kQuantHistWords;
        const uint32_t words = level == 0 ? kTopkBins : s_q.G * kQuantSubBins;
        for (uint32_t c = tid; c < words; c += 256u) {
            s_hist[c] = h[c];
            h[c] = 0u;
        }
        __syncthreads();
        const bool ok = s_ok != 0u;
        if (ok) quant_resolve<256>(s_q, s_hist, B, level);
        if (!ok || level == LEVELS - 1) {
            if (tid < a.num_q) quant_write<S>(a, seg, tid, len, nans, ok, s_q);
        }
        if (tid < kStateWords) reinterpret_cast<uint32_t *>(&sl->q)[tid] = reinterpret_cast<const uint32_t *>(&s_q)[tid];
        if (tid == 0u) {
            if (!ok) {
                sl->ok = 0u;
            } else if (state == 1u) {
                sl->state = 2u;
            } else if (state == 0u && level + 2 < LEVELS && a.compact_divisor != 0u && s_q.live <= len / a.compact_divisor &&
                       s_q.live <= tiles * kSelAreaPerTile) {  // (two levels left at least: the copy costs the read it saves when one is)
                sl->state = 1u;
                sl->ccount = s_q.live;
                sl->cursor = 0u;
                atomicAdd(&a.stats[3], 1ull);
            }
        }
        __syncthreads();
    }
}

uint32_t grid_of(uint64_t work, uint32_t cap) { return static_cast<uint32_t>(std::max<uint64_t>(1u, std::min<uint64_t>(work, cap))); }

template <typename S>
hipError_t launch_quantile_as(hipStream_t stream, const QuantileArgs &a, const QuantLayout &L) {
    constexpr int B = 8 * static_cast<int>(sizeof(S)), LEVELS = quantile_levels(B), LDS_ITEMS = static_cast<int>(kSelLdsBytes / sizeof(S)) / 256;
    auto *ctl = reinterpret_cast<TopkControl *>(a.scratch + L.control);
    auto *list = reinterpret_cast<uint32_t *>(a.scratch + L.list);
    auto *slots = reinterpret_cast<QuantSlot *>(a.scratch + L.slots);
    auto *hist = reinterpret_cast<uint32_t *>(a.scratch + L.hist);
    auto *area = reinterpret_cast<S *>(a.scratch + L.area);
    hipError_t e = hipMemsetAsync(ctl, 0, sizeof(TopkControl), stream);
    if (e != hipSuccess) return e;
    const uint32_t S_ = a.num_segments;
    hipLaunchKernelGGL(quantile_classify_kernel, dim3(grid_of((static_cast<uint64_t>(S_) + 255u) / 256u, 0xFFFFFFFFu)), dim3(256), 0, stream, a, ctl, list,
                       slots, L.slot_cap, L.tile_cap);
    hipLaunchKernelGGL((quantile_workgroup_kernel<S, 256, LDS_ITEMS, true>), dim3(grid_of(S_, 8192u)), dim3(256), 0, stream, a, ctl, list);
    if (a.n > kSelLdsBytes / sizeof(S))  // (else no segment is longer than the LDS tier's cap)
        hipLaunchKernelGGL((quantile_workgroup_kernel<S, 1024, 16, false>), dim3(grid_of(S_, 1024u)), dim3(1024), 0, stream, a, ctl, list);
    if (L.slot_cap != 0u && a.grid_min_keys != 0u && a.n >= a.grid_min_keys) {
        const uint32_t walkers = grid_of(L.tile_cap, 1024u), per_slot = grid_of(L.slot_cap, 1024u);
        hipLaunchKernelGGL(quantile_grid_init_kernel, dim3(per_slot), dim3(256), 0, stream, ctl, hist, L.slot_cap);
        for (int level = 0; level < LEVELS; ++level) {
            hipLaunchKernelGGL((quantile_grid_walk_kernel<S, kWalkHist>), dim3(walkers), dim3(kGridThreads), 0, stream, a, ctl, slots, hist, area, L.slot_cap,
                               L.tile_cap, level);
            hipLaunchKernelGGL((quantile_grid_select_kernel<S>), dim3(per_slot), dim3(256), 0, stream, a, ctl, slots, hist, L.slot_cap, level);
            if (level + 2 < LEVELS && a.compact_divisor != 0u)  // (the copy is one read of src: it pays when two levels or more are left)
                hipLaunchKernelGGL((quantile_grid_walk_kernel<S, kWalkSieve>), dim3(walkers), dim3(kGridThreads), 0, stream, a, ctl, slots, hist, area,
                                   L.slot_cap, L.tile_cap, level);
        }
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_quantile(hipStream_t stream, const QuantileArgs &a, const QuantLayout &L) {
    return a.dtype == kSortF64 ? launch_quantile_as<uint64_t>(stream, a, L) : launch_quantile_as<uint32_t>(stream, a, L);
}

}  // namespace vrs
