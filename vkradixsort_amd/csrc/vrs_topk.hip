// vrs_topk.hip -- top-k selection (vrs_topk_segments): the k smallest (or largest) keys of every segment by radix select, one sequence
// of launches whose shapes do not depend on the segments.
//   classify: one thread per segment; its tier (topk_tier, the function vrs_topk_tier_for exports), a place on the LDS tier's list (front
//     of one array) or the BLOCK tier's (back of it), or a grid slot with a range of tiles; per-tier counters for vrs_topk_stats.
//   One set of kernels, templated on a traits type (TopkTraits: the element as the unsigned integer of its width, the rank's type, the
//     rank map -- the three 32-bit key types' or torch's order of a vrs_sort_dtype, VRS_TOPK_DTYPE -- and with them the significant bits,
//     the levels and the elements per 4-byte word).  An element is ranked in registers as it is read.
//   selection: digits of at most 11 bits of the rank r from the top (select_level: 11, 11 and 10 for 32 bits).  A level counts the
//     digit of every key whose higher bits match the prefix chosen so far, picks the digit d* that holds the need-th key, and stops
//     early once every matching key is needed.  Order inside a tile does not matter to a count: 1- and 2-byte elements are read there
//     as aligned 4-byte words of 4 or 2 (packed_walk), the elements of a word outside the segment masked.
//   emission: in index order, element by element -- keys below the prefix to slots [0, lt), the first `need` keys equal to it (lowest
//     index first) to [lt, m) -- so a stable sort by r of the m survivors is the stable order (equal keys stay in index order, and the
//     two groups occupy disjoint ranges of r).  The lane that emits an element fetches its own bits at its position: a NaN keeps its
//     payload and a zero its sign, which their shared ranks could not give back.
//   LDS tier (up to kTopkLdsCap keys): one 256-thread workgroup per segment, ranks read once into LDS.
//   BLOCK tier: one 1024-thread workgroup per segment streaming 16384-key tiles: one read per level and one for the emission.
//   GRID tier: each phase one launch over a fixed grid that walks the tiles of every grid slot; per-workgroup LDS histograms flushed with
//     one atomic per non-zero bin, one workgroup per slot picks the digit, a counting read and a per-slot scan order the emission.
//   sorted output (k <= kTopkSortCap): one workgroup per segment sorts (rank, slot) of its survivors in LDS (local_pass, stable, over
//     the bits that vary) and gathers their bits and positions by the slot.
// Loops whose bound may come near 2^32 (grid strides, a segment's tiles, k) count in 64 bits: a 32-bit i + step would wrap below the bound.
#include "vrs_topk.hpp"

#include "vrs_local_sort.hpp"
#include "vrs_radix_select.hpp"  // hist_add, select_digit, grid_slots, grid_tiles, find_slot
#include "vrs_topk_order.hpp"    // sel_less, sel_match, sel_apply; select_rank, select_level: torch's order and the levels' digits

namespace vrs {
namespace {

// S: the element as the unsigned integer of its width; R: its rank's type; TORCH: ranked in torch's order (VRS_TOPK_DTYPE), else by the
// call's 32-bit key type
template <typename S_, typename R_, bool TORCH_>
struct TopkTraits {
    using S = S_;
    using R = R_;
    static constexpr bool TORCH = TORCH_;
    static constexpr int BYTES = static_cast<int>(sizeof(S)), B = 8 * BYTES;  // B: the rank's significant bits
    static constexpr int LEVELS = (B + 10) / 11;                              // select_levels(B)
    static constexpr int PER = BYTES < 4 ? 4 / BYTES : 1;                     // elements per 4-byte word of the packed reads
    static constexpr int LDS_ITEMS = static_cast<int>(kTopkLdsBytes / sizeof(R)) / 256;
    static_assert(sizeof(R) == (BYTES == 8 ? 8 : 4) && (TORCH || BYTES == 4), "ranks of 4 bytes, of 8 for 8-byte elements");
};

// the call's rank map: load(p) of every kernel is rank(src[p])
template <class T>
struct TopkRank {
    using R = typename T::R;
    int kind;  // select_kind of the dtype; the key type when not TORCH
    R inf_bits;
    bool largest;
    __device__ __forceinline__ R operator()(typename T::S x) const {
        if constexpr (T::TORCH) return select_rank<R, T::B>(static_cast<R>(x), kind, inf_bits, largest);
        else return topk_rank(x, kind, largest);
    }
};
template <class T>
__device__ __forceinline__ TopkRank<T> rank_of(const TopkArgs &a) {
    using R = typename T::R;
    TopkRank<T> f;
    const int dtype = a.key_type & 0xFF;
    f.kind = T::TORCH ? select_kind(dtype) : a.key_type;
    f.inf_bits = dtype == kSortF16    ? static_cast<R>(0x7C00u)
                 : dtype == kSortBF16 ? static_cast<R>(0x7F80u)
                 : dtype == kSortF32  ? static_cast<R>(0x7F800000u)
                                      : static_cast<R>(0x7FF0000000000000ull);
    f.largest = (a.flags & kTopkLargest) != 0;
    return f;
}

template <typename R>
__device__ __forceinline__ TopkSel<R> sel_of(const TopkSel<unsigned long long> &s) {
    return TopkSel<R>{static_cast<R>(s.prefix), s.shift, s.lt, s.need, s.done};
}

// the digit histogram (shift, mask: the level's) of the keys of one tile that match the selection so far; position p of the tile: load(p)
template <int THREADS, int ITEMS, typename R, class Load>
__device__ __forceinline__ void hist_tile(Load load, uint32_t cnt, const TopkSel<R> &sel, uint32_t shift, uint32_t mask, uint32_t *s_hist) {
    R r[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = i * THREADS + threadIdx.x;
        r[i] = p < cnt ? load(p) : static_cast<R>(0);
    }
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = i * THREADS + threadIdx.x;
        if (p < cnt && sel_match(r[i], sel)) hist_add(s_hist, static_cast<uint32_t>(r[i] >> shift) & mask);
    }
}

// 1- and 2-byte elements, where their order does not matter: the segment seg[0, len) as the aligned 4-byte words that hold it, PER
// elements each.  Word w holds the elements w * PER + j - head (head: the elements of the first word in front of the segment); the
// ones outside [0, len) -- in the first and the last word -- are skipped.  Walks the words [w0, w1), U in flight per thread, and calls
// visit(element index, element) for every element inside.  The words lie within the 4-byte-aligned span of the segment, so within
// the buffer's last aligned word at the most.
template <class T>
__device__ __forceinline__ uint32_t packed_head(const typename T::S *seg) {
    return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(seg) & 3u) / T::BYTES;
}
template <class T>
__device__ __forceinline__ uint32_t packed_words(const typename T::S *seg, uint32_t len) {
    return static_cast<uint32_t>((static_cast<uint64_t>(packed_head<T>(seg)) + len + T::PER - 1u) / T::PER);
}
template <class T, int THREADS, int U, class Visit>
__device__ __forceinline__ void packed_walk(const typename T::S *seg, uint32_t len, uint32_t w0, uint32_t w1, Visit visit) {
    static_assert(T::PER > 1 && U >= 1, "elements narrower than a word");
    using S = typename T::S;
    const uint32_t head = packed_head<T>(seg);
    const uint32_t *words = reinterpret_cast<const uint32_t *>(reinterpret_cast<uintptr_t>(seg) & ~static_cast<uintptr_t>(3u));
    for (uint64_t base = w0; base < w1; base += THREADS * U) {  // (64-bit: base + THREADS * U may pass 2^32)
        uint32_t v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t w = base + u * THREADS + threadIdx.x;
            v[u] = w < w1 ? words[w] : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t w = base + u * THREADS + threadIdx.x;
            if (w >= w1) continue;
#pragma unroll
            for (int j = 0; j < T::PER; ++j) {
                const uint64_t at = w * T::PER + j;  // (element at - head)
                if (at >= head && at - head < len) visit(static_cast<uint32_t>(at - head), static_cast<S>(v[u] >> (T::B * j)));
            }
        }
    }
}


// Emits one tile in index order (position p = i * THREADS + tid; index of p: pos0 + p; its element: src[p]).  lt_base / eq_base: keys
// below / equal to the prefix in the segment's tiles before this one.  Returns this tile's two counts.
template <int THREADS, int ITEMS, typename R, typename S, class Load>
__device__ __forceinline__ uint2 emit_tile(Load load, const S *src, uint32_t cnt, uint32_t pos0, const TopkSel<R> &sel, uint32_t m, uint32_t lt_base,
                                           uint32_t eq_base, S *ok, uint32_t *oi, uint32_t *s_scan, uint32_t *s_wtot) {
    constexpr int WAVES = THREADS / 64, E = ITEMS * WAVES;
    static_assert(E % 64 == 0 && E <= THREADS, "one scanning thread per (item, wave)");
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    R r[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = i * THREADS + tid;
        r[i] = p < cnt ? load(p) : static_cast<R>(0);
    }
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = i * THREADS + tid;
        const bool lt = p < cnt && sel_less(r[i], sel), eq = p < cnt && !lt && sel_match(r[i], sel);
        const uint64_t bl = __ballot(lt), be = __ballot(eq);
        if (lane == 0u) {
            s_scan[i * WAVES + wave] = static_cast<uint32_t>(__popcll(bl));
            s_scan[E + i * WAVES + wave] = static_cast<uint32_t>(__popcll(be));
        }
    }
    __syncthreads();
    if (tid < static_cast<uint32_t>(E)) {
        const uint32_t a = s_scan[tid], b = s_scan[E + tid];
        uint32_t ia = a, ib = b;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t ta = __shfl_up(ia, o), tb = __shfl_up(ib, o);
            if (lane >= static_cast<uint32_t>(o)) {
                ia += ta;
                ib += tb;
            }
        }
        if (lane == 63u) {
            s_wtot[wave] = ia;
            s_wtot[8 + wave] = ib;
        }
        s_scan[tid] = ia - a;
        s_scan[E + tid] = ib - b;
    }
    __syncthreads();
    if (tid < static_cast<uint32_t>(E)) {
        uint32_t add_a = 0, add_b = 0;
        for (uint32_t v = 0; v < wave; ++v) {
            add_a += s_wtot[v];
            add_b += s_wtot[8 + v];
        }
        s_scan[tid] += add_a;
        s_scan[E + tid] += add_b;
    }
    __syncthreads();
    uint2 tot = make_uint2(0u, 0u);
#pragma unroll
    for (int v = 0; v < E / 64; ++v) {
        tot.x += s_wtot[v];
        tot.y += s_wtot[8 + v];
    }
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = i * THREADS + tid;
        const bool lt = p < cnt && sel_less(r[i], sel), eq = p < cnt && !lt && sel_match(r[i], sel);
        const uint64_t bl = __ballot(lt), be = __ballot(eq);
        uint32_t slot = 0xFFFFFFFFu;
        if (lt) {
            slot = lt_base + s_scan[i * WAVES + wave] + count_below(bl);
            if (slot >= sel.lt) slot = 0xFFFFFFFFu;
        } else if (eq) {
            const uint32_t er = eq_base + s_scan[E + i * WAVES + wave] + count_below(be);
            if (er < sel.need) slot = sel.lt + er;
        }
        if (slot < m) {
            ok[slot] = src[p];  // (its own bits: at most m fetches a segment)
            if (oi) oi[slot] = pos0 + p;
        }
    }
    __syncthreads();  // (s_scan and s_wtot are free again)
    return tot;
}

template <typename S>
__device__ __forceinline__ void fill_tail(S *ok, uint32_t *oi, uint32_t m, uint32_t k, uint32_t threads) {
    for (size_t j = m + threadIdx.x; j < k; j += threads) {
        ok[j] = static_cast<S>(~static_cast<S>(0));
        if (oi) oi[j] = 0xFFFFFFFFu;
    }
}

__global__ __launch_bounds__(256) void topk_classify_kernel(TopkArgs a, TopkControl *__restrict__ ctl, uint32_t *__restrict__ list,
                                                            TopkSlot *__restrict__ slots, uint32_t slot_cap, uint32_t tile_cap) {
    __shared__ uint32_t s_stat[3];
    const uint32_t tid = threadIdx.x;
    if (tid < 3u) s_stat[tid] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + tid;
    if (i < a.num_segments) {
        uint32_t cb, ce;
        int tier = topk_tier_cap(a.offsets[i], a.offsets[i + 1u], a.n, a.lds_cap, a.grid_min_keys, &cb, &ce);
        atomicAdd(&s_stat[tier], 1u);
        const uint32_t len = ce - cb, m = min(a.k, len);
        if (tier == kTopkTierGrid) {
            const uint32_t tiles = static_cast<uint32_t>((static_cast<uint64_t>(len) + kTopkTile - 1u) / kTopkTile);  // (len + 16383 wraps near 2^32)
            const unsigned long long old = atomicAdd(&ctl->grid_packed, (static_cast<unsigned long long>(tiles) << 32) | 1ull);
            const uint32_t slot = static_cast<uint32_t>(old), base = static_cast<uint32_t>(old >> 32);
            bool valid = false;
            if (slot < slot_cap) {  // (beyond the caps: overlapping ranges; the BLOCK kernel takes them)
                valid = static_cast<uint64_t>(base) + tiles <= tile_cap;
                TopkSlot s{};
                s.seg = i;
                s.b = cb;
                s.len = len;
                s.m = m;
                s.tile_base = base;
                s.tiles = tiles;
                s.valid = valid ? 1u : 0u;
                s.sel = topk_sel_init<unsigned long long>(len, m);
                slots[slot] = s;
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
template <class T, int THREADS, int ITEMS, bool LDS>
__global__ __launch_bounds__(THREADS) void topk_workgroup_kernel(TopkArgs a, const TopkControl *__restrict__ ctl, const uint32_t *__restrict__ list) {
    using S = typename T::S;
    using R = typename T::R;
    constexpr int TILE = THREADS * ITEMS, E = ITEMS * (THREADS / 64);
    static_assert(!LDS || TILE * sizeof(R) == kTopkLdsBytes, "the LDS tier's segment is one tile");
    static_assert(ITEMS % T::PER == 0, "whole words per thread");
    __shared__ uint32_t s_hist[kTopkBins];
    __shared__ R s_r[LDS ? TILE : 1];
    __shared__ uint32_t s_scan[2 * E];
    __shared__ uint32_t s_wtot[16];
    __shared__ uint32_t s_res[3];
    const uint32_t count = LDS ? ctl->lds_count : ctl->block_count;
    const TopkRank<T> rank = rank_of<T>(a);
    for (size_t jw = blockIdx.x; jw < count; jw += gridDim.x) {
        const uint32_t j = static_cast<uint32_t>(jw);
        const uint32_t seg = LDS ? list[j] : list[a.num_segments - 1u - j];
        uint32_t b, e;
        (void)topk_tier(a.offsets[seg], a.offsets[seg + 1u], a.n, 0u, &b, &e);
        const uint32_t len = e - b, m = min(a.k, len);
        S *ok = static_cast<S *>(a.out_keys) + static_cast<size_t>(seg) * a.k;
        uint32_t *oi = a.positions ? a.positions + static_cast<size_t>(seg) * a.k : nullptr;
        fill_tail(ok, oi, m, a.k, THREADS);
        if (m == 0u) continue;
        const S *src = static_cast<const S *>(a.keys) + b;
        if constexpr (LDS) {
            if constexpr (T::PER > 1) {
                packed_walk<T, THREADS, ITEMS / T::PER>(src, len, 0u, packed_words<T>(src, len), [&](uint32_t p, S x) { s_r[p] = rank(x); });
            } else {
                for (uint32_t p = threadIdx.x; p < len; p += THREADS) s_r[p] = rank(src[p]);
            }
            __syncthreads();
        }
        TopkSel<R> sel = topk_sel_init<R>(len, m);
        for (int level = 0; level < T::LEVELS && !sel.done; ++level) {
            for (uint32_t c = threadIdx.x; c < kTopkBins; c += THREADS) s_hist[c] = 0u;
            __syncthreads();
            uint32_t shift, mask;
            select_level(T::B, level, &shift, &mask);
            if constexpr (!LDS && T::PER > 1) {  // (a count: the whole segment as words, no tiles)
                packed_walk<T, THREADS, ITEMS / T::PER>(src, len, 0u, packed_words<T>(src, len), [&](uint32_t, S x) {
                    const R r = rank(x);
                    if (sel_match(r, sel)) hist_add(s_hist, static_cast<uint32_t>(r >> shift) & mask);
                });
            } else {
                for (uint64_t tile0 = 0; tile0 < len; tile0 += TILE) {  // (64-bit: a 32-bit t0 + TILE wraps below len near 2^32)
                    const uint32_t t0 = static_cast<uint32_t>(tile0), cnt = min(static_cast<uint32_t>(TILE), len - t0);
                    if constexpr (LDS) hist_tile<THREADS, ITEMS>([&](uint32_t p) { return s_r[t0 + p]; }, cnt, sel, shift, mask, s_hist);
                    else hist_tile<THREADS, ITEMS>([&](uint32_t p) { return rank(src[t0 + p]); }, cnt, sel, shift, mask, s_hist);
                }
            }
            __syncthreads();
            select_digit<THREADS>(s_hist, sel.need, s_wtot, s_res);
            sel_apply(sel, T::B, level, s_res[0], s_res[1], s_res[2]);
            __syncthreads();
        }
        uint32_t lt_base = 0, eq_base = 0;
        for (uint64_t tile0 = 0; tile0 < len; tile0 += TILE) {
            const uint32_t t0 = static_cast<uint32_t>(tile0), cnt = min(static_cast<uint32_t>(TILE), len - t0);
            uint2 tot;
            if constexpr (LDS)
                tot = emit_tile<THREADS, ITEMS>([&](uint32_t p) { return s_r[t0 + p]; }, src + t0, cnt, t0, sel, m, lt_base, eq_base, ok, oi, s_scan, s_wtot);
            else
                tot = emit_tile<THREADS, ITEMS>([&](uint32_t p) { return rank(src[t0 + p]); }, src + t0, cnt, t0, sel, m, lt_base, eq_base, ok, oi, s_scan,
                                                s_wtot);
            lt_base += tot.x;
            eq_base += tot.y;
        }
    }
}

// ---- GRID tier: kernels that walk the virtual tiles [0, tiles taken) of every slot ----
constexpr int kGridThreads = 1024, kGridItems = 16;
static_assert(kGridThreads * kGridItems == static_cast<int>(kTopkTile), "a grid tile is one pass of a workgroup");

__global__ __launch_bounds__(256) void topk_grid_init_kernel(const TopkControl *__restrict__ ctl, uint32_t *__restrict__ hist, uint32_t slot_cap) {
    const uint32_t ns = grid_slots(ctl, slot_cap);
    for (size_t s = blockIdx.x; s < ns; s += gridDim.x)
        for (uint32_t c = threadIdx.x; c < kTopkBins; c += 256u) hist[s * kTopkBins + c] = 0u;
}

// PHASE 0: digit histograms of level `level`; 1: per-tile counts of the two classes; 2: the emission
template <class T, int PHASE>
__global__ __launch_bounds__(kGridThreads) void topk_grid_walk_kernel(TopkArgs a, const TopkControl *__restrict__ ctl, const TopkSlot *__restrict__ slots,
                                                                      uint32_t *__restrict__ hist, uint2 *__restrict__ tilecnt, uint32_t slot_cap,
                                                                      uint32_t tile_cap, int level) {
    using S = typename T::S;
    using R = typename T::R;
    constexpr int E = kGridItems * (kGridThreads / 64);
    __shared__ uint32_t s_hist[PHASE == 0 ? kTopkBins : 1];
    __shared__ uint32_t s_scan[PHASE == 2 ? 2 * E : 1];
    __shared__ uint32_t s_wtot[16];
    __shared__ uint32_t s_slot, s_cnt[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t ns = grid_slots(ctl, slot_cap), total = grid_tiles(ctl, slot_cap, tile_cap);
    const TopkRank<T> rank = rank_of<T>(a);
    if constexpr (PHASE == 0)
        for (uint32_t c = tid; c < kTopkBins; c += kGridThreads) s_hist[c] = 0u;
    uint32_t cur = 0xFFFFFFFFu;
    bool dirty = false;
    auto flush = [&]() {  // the workgroup's histogram of slot `cur` into the slot's: one atomic per non-zero bin
        __syncthreads();
        for (uint32_t c = tid; c < kTopkBins; c += kGridThreads) {
            const uint32_t v = s_hist[c];
            if (v != 0u) {
                atomicAdd(&hist[static_cast<size_t>(cur) * kTopkBins + c], v);
                s_hist[c] = 0u;
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
        if constexpr (PHASE == 0) {
            if (s != cur) {
                if (dirty) {
                    if constexpr (PHASE == 0) flush();
                    dirty = false;
                }
                cur = s;
            }
        }
        const TopkSlot &sl = slots[s];
        const TopkSel<R> sel = sel_of<R>(sl.sel);
        if (!sl.valid || t - sl.tile_base >= sl.tiles) continue;
        const uint32_t ti = t - sl.tile_base, off = ti * kTopkTile, cnt = min(kTopkTile, sl.len - off);
        const S *src = static_cast<const S *>(a.keys) + sl.b + off;
        auto load = [&](uint32_t p) { return rank(src[p]); };
        if constexpr (PHASE == 0) {
            if (sel.done) continue;
            uint32_t shift, mask;
            select_level(T::B, level, &shift, &mask);
            if constexpr (T::PER > 1) {  // (a count: tile ti takes the segment's words [ti, ti + 1) * 16384 / PER, the last one the rest)
                constexpr uint32_t WT = kTopkTile / T::PER;
                const S *seg_src = static_cast<const S *>(a.keys) + sl.b;
                const uint32_t w1 = ti + 1u == sl.tiles ? packed_words<T>(seg_src, sl.len) : (ti + 1u) * WT;
                packed_walk<T, kGridThreads, kGridItems / T::PER>(seg_src, sl.len, ti * WT, w1, [&](uint32_t, S x) {
                    const R r = rank(x);
                    if (sel_match(r, sel)) hist_add(s_hist, static_cast<uint32_t>(r >> shift) & mask);
                });
            } else {
                hist_tile<kGridThreads, kGridItems>(load, cnt, sel, shift, mask, s_hist);
            }
            dirty = true;
        } else if constexpr (PHASE == 1) {
            if (tid < 2u) s_cnt[tid] = 0u;
            __syncthreads();
            R r[kGridItems];
#pragma unroll
            for (int i = 0; i < kGridItems; ++i) {
                const uint32_t p = i * kGridThreads + tid;
                r[i] = p < cnt ? load(p) : static_cast<R>(0);
            }
            uint32_t nl = 0, ne = 0;
#pragma unroll
            for (int i = 0; i < kGridItems; ++i) {
                const uint32_t p = i * kGridThreads + tid;
                const bool lt = p < cnt && sel_less(r[i], sel), eq = p < cnt && !lt && sel_match(r[i], sel);
                nl += static_cast<uint32_t>(__popcll(__ballot(lt)));
                ne += static_cast<uint32_t>(__popcll(__ballot(eq)));
            }
            if ((tid & 63u) == 0u) {
                atomicAdd(&s_cnt[0], nl);
                atomicAdd(&s_cnt[1], ne);
            }
            __syncthreads();
            if (tid == 0u) tilecnt[t] = make_uint2(s_cnt[0], s_cnt[1]);
            __syncthreads();
        } else {
            const uint2 base = tilecnt[t];
            S *ok = static_cast<S *>(a.out_keys) + static_cast<size_t>(sl.seg) * a.k;
            uint32_t *oi = a.positions ? a.positions + static_cast<size_t>(sl.seg) * a.k : nullptr;
            (void)emit_tile<kGridThreads, kGridItems>(load, src, cnt, off, sel, sl.m, base.x, base.y, ok, oi, s_scan, s_wtot);
        }
    }
    if constexpr (PHASE == 0)
        if (dirty) flush();
}

// one workgroup per slot: the digit of level `level` from the slot's histogram (zeroed behind it for the next level)
__global__ __launch_bounds__(256) void topk_grid_select_kernel(const TopkControl *__restrict__ ctl, TopkSlot *__restrict__ slots, uint32_t *__restrict__ hist,
                                                               uint32_t slot_cap, int bits, int level) {
    __shared__ uint32_t s_hist[kTopkBins];
    __shared__ uint32_t s_wtot[4], s_res[3];
    const uint32_t ns = grid_slots(ctl, slot_cap);
    for (size_t sw = blockIdx.x; sw < ns; sw += gridDim.x) {
        const uint32_t s = static_cast<uint32_t>(sw);
        TopkSel<unsigned long long> sel = slots[s].sel;
        if (!slots[s].valid || sel.done) continue;
        uint32_t *h = hist + static_cast<size_t>(s) * kTopkBins;
        for (uint32_t c = threadIdx.x; c < kTopkBins; c += 256u) {
            s_hist[c] = h[c];
            h[c] = 0u;
        }
        __syncthreads();
        select_digit<256>(s_hist, sel.need, s_wtot, s_res);
        sel_apply(sel, bits, level, s_res[0], s_res[1], s_res[2]);
        if (threadIdx.x == 0u) slots[s].sel = sel;
        __syncthreads();
    }
}

// one workgroup per slot: the tiles' counts become their bases (exclusive scan in tile order); the slots past m get the filler
template <typename S>
__global__ __launch_bounds__(1024) void topk_grid_scan_kernel(TopkArgs a, const TopkControl *__restrict__ ctl, const TopkSlot *__restrict__ slots,
                                                              uint2 *__restrict__ tilecnt, uint32_t slot_cap) {
    __shared__ uint32_t s_wtot[2 * 16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t ns = grid_slots(ctl, slot_cap);
    for (size_t s = blockIdx.x; s < ns; s += gridDim.x) {
        const TopkSlot sl = slots[s];
        if (!sl.valid) continue;
        fill_tail(static_cast<S *>(a.out_keys) + static_cast<size_t>(sl.seg) * a.k, a.positions ? a.positions + static_cast<size_t>(sl.seg) * a.k : nullptr,
                  sl.m, a.k, 1024u);
        uint32_t carry_a = 0, carry_b = 0;
        for (uint32_t t0 = 0; t0 < sl.tiles; t0 += 1024u) {
            const uint32_t t = t0 + tid;
            const uint2 v = t < sl.tiles ? tilecnt[sl.tile_base + t] : make_uint2(0u, 0u);
            uint32_t ia = v.x, ib = v.y;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t ta = __shfl_up(ia, o), tb = __shfl_up(ib, o);
                if (lane >= static_cast<uint32_t>(o)) {
                    ia += ta;
                    ib += tb;
                }
            }
            if (lane == 63u) {
                s_wtot[wave] = ia;
                s_wtot[16 + wave] = ib;
            }
            __syncthreads();
            uint32_t add_a = carry_a, add_b = carry_b, all_a = carry_a, all_b = carry_b;
            for (uint32_t w = 0; w < 16u; ++w) {
                if (w < wave) {
                    add_a += s_wtot[w];
                    add_b += s_wtot[16 + w];
                }
                all_a += s_wtot[w];
                all_b += s_wtot[16 + w];
            }
            if (t < sl.tiles) tilecnt[sl.tile_base + t] = make_uint2(add_a + ia - v.x, add_b + ib - v.y);
            carry_a = all_a;
            carry_b = all_b;
            __syncthreads();
        }
    }
}

// VRS_TOPK_SORTED, k <= THREADS * ITEMS: one workgroup per segment sorts (rank, slot) of its m survivors by the rank, stably, over the
// bits that vary; then every slot takes the bits and the position of the slot that sorted into it -- all read before any is written
template <class T, int THREADS, int ITEMS>
__global__ __launch_bounds__(THREADS) void topk_sort_small_kernel(TopkArgs a) {
    using S = typename T::S;
    using R = typename T::R;
    constexpr int WAVES = THREADS / 64, CAP = THREADS * ITEMS;
    __shared__ R s_keys[CAP];
    __shared__ uint32_t s_vals[CAP];
    __shared__ uint32_t s_hist[WAVES * 256];
    __shared__ R s_tmp[WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t seg0 = wave * (ITEMS * 64) + lane;
    const TopkRank<T> rank = rank_of<T>(a);
    for (size_t sw = blockIdx.x; sw < a.num_segments; sw += gridDim.x) {
        const uint32_t seg = static_cast<uint32_t>(sw);
        uint32_t b, e;
        (void)topk_tier(a.offsets[seg], a.offsets[seg + 1u], a.n, 0u, &b, &e);
        const uint32_t m = min(a.k, e - b);
        if (m < 2u || m > static_cast<uint32_t>(CAP)) continue;
        S *ok = static_cast<S *>(a.out_keys) + static_cast<size_t>(seg) * a.k;
        uint32_t *oi = a.positions ? a.positions + static_cast<size_t>(seg) * a.k : nullptr;
        R key[ITEMS];
        uint32_t val[ITEMS];
        const R k0 = rank(ok[0]);
        R diff = 0;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t idx = seg0 + i * 64;
            key[i] = idx < m ? rank(ok[idx]) : k0;
            val[i] = idx < m ? idx : 0u;
            diff |= key[i] ^ k0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) diff |= __shfl_xor(diff, o);
        if constexpr (WAVES > 1) {
            if (lane == 0u) s_tmp[wave] = diff;
            __syncthreads();
#pragma unroll
            for (int v = 0; v < WAVES; ++v) diff |= s_tmp[v];
            __syncthreads();
        }
        if (diff == 0) continue;  // every survivor equal: already in index order
        const uint32_t width = 64u - static_cast<uint32_t>(__clzll(static_cast<unsigned long long>(diff)));
        for (uint32_t shift = 0; shift < width; shift += 8u)
            local_pass<THREADS, ITEMS, 8, true, true, R>(key, val, s_keys, s_vals, s_hist, reinterpret_cast<uint32_t *>(s_tmp), shift, m);
        S bits[ITEMS];
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t from = seg0 + i * 64 < m ? val[i] : 0u;  // (a position behind the survivors holds no slot)
            bits[i] = ok[from];
            val[i] = oi ? oi[from] : 0u;
        }
        __syncthreads();  // (every slot read before one is written)
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const uint32_t idx = seg0 + i * 64;
            if (idx < m) {
                ok[idx] = bits[i];
                if (oi) oi[idx] = val[i];
            }
        }
    }
}

__device__ __forceinline__ uint32_t segment_m(const TopkArgs &a, uint32_t seg, uint32_t *b) {
    uint32_t e;
    (void)topk_tier(a.offsets[seg], a.offsets[seg + 1u], a.n, 0u, b, &e);
    return min(a.k, e - *b);
}

// sk, sv: the sort area's ranks and values.  a.positions: where the emission put the positions (sv itself when TORCH and the call has no
// out_indices), null: none
template <class T>
__global__ __launch_bounds__(256) void topk_sort_prep_kernel(TopkArgs a, typename T::R *__restrict__ sk, uint32_t *sv) {
    using R = typename T::R;
    const uint32_t total = a.num_segments * a.k;
    const TopkRank<T> rank = rank_of<T>(a);
    const typename T::S *ok = static_cast<const typename T::S *>(a.out_keys);
    for (size_t sw = blockIdx.x * 256u + threadIdx.x; sw < total; sw += gridDim.x * 256u) {
        const uint32_t s = static_cast<uint32_t>(sw), seg = s / a.k, j = s - seg * a.k;
        uint32_t b;
        const bool in = j < segment_m(a, seg, &b);
        sk[s] = in ? rank(ok[s]) : static_cast<R>(~static_cast<R>(0));
        sv[s] = in && a.positions ? a.positions[s] : 0xFFFFFFFFu;
    }
}

__global__ __launch_bounds__(256) void topk_sort_offsets_kernel(TopkArgs a) {
    uint32_t *offs = static_cast<uint32_t *>(a.out_keys);
    for (size_t i = blockIdx.x * 256u + threadIdx.x; i <= a.num_segments; i += gridDim.x * 256u) offs[i] = static_cast<uint32_t>(i) * a.k;
}

// the sorted survivors back: TORCH -- the own bits at the sorted positions; else the key the sorted rank stands for
template <class T>
__global__ __launch_bounds__(256) void topk_sort_back_kernel(TopkArgs a, const typename T::R *__restrict__ sk, const uint32_t *__restrict__ sv) {
    using S = typename T::S;
    const uint32_t total = a.num_segments * a.k;
    const bool largest = (a.flags & kTopkLargest) != 0;
    S *ok = static_cast<S *>(a.out_keys);
    for (size_t sw = blockIdx.x * 256u + threadIdx.x; sw < total; sw += gridDim.x * 256u) {
        const uint32_t s = static_cast<uint32_t>(sw), seg = s / a.k, j = s - seg * a.k;
        uint32_t b;
        const bool in = j < segment_m(a, seg, &b);
        S x = static_cast<S>(~static_cast<S>(0));
        if (in) {
            if constexpr (T::TORCH) x = static_cast<const S *>(a.keys)[static_cast<size_t>(b) + sv[s]];
            else x = topk_unrank(sk[s], a.key_type, largest);
        }
        ok[s] = x;
        if (a.out_indices) a.out_indices[s] = in ? sv[s] : 0xFFFFFFFFu;
    }
}

uint32_t grid_of(uint64_t work, uint32_t cap) { return static_cast<uint32_t>(std::max<uint64_t>(1u, std::min<uint64_t>(work, cap))); }

template <class T>
hipError_t launch_topk_as(hipStream_t stream, const TopkArgs &a, const TopkLayout &L) {
    using S = typename T::S;
    auto *ctl = reinterpret_cast<TopkControl *>(a.scratch + L.control);
    auto *list = reinterpret_cast<uint32_t *>(a.scratch + L.list);
    auto *slots = reinterpret_cast<TopkSlot *>(a.scratch + L.slots);
    auto *hist = reinterpret_cast<uint32_t *>(a.scratch + L.hist);
    auto *tilecnt = reinterpret_cast<uint2 *>(a.scratch + L.tiles);
    hipError_t e = hipMemsetAsync(ctl, 0, sizeof(TopkControl), stream);
    if (e != hipSuccess) return e;
    const uint32_t S_ = a.num_segments;
    hipLaunchKernelGGL(topk_classify_kernel, dim3(grid_of((static_cast<uint64_t>(S_) + 255u) / 256u, 0xFFFFFFFFu)), dim3(256), 0, stream, a, ctl, list,
                       slots, L.slot_cap, L.tile_cap);
    hipLaunchKernelGGL((topk_workgroup_kernel<T, 256, T::LDS_ITEMS, true>), dim3(grid_of(S_, 8192u)), dim3(256), 0, stream, a, ctl, list);
    if (a.n > a.lds_cap)  // (else no segment is longer than the LDS tier's cap)
        hipLaunchKernelGGL((topk_workgroup_kernel<T, 1024, 16, false>), dim3(grid_of(S_, 1024u)), dim3(1024), 0, stream, a, ctl, list);
    if (L.slot_cap != 0u && a.grid_min_keys != 0u && a.n >= a.grid_min_keys) {
        const uint32_t walkers = grid_of(L.tile_cap, 1024u), per_slot = grid_of(L.slot_cap, 1024u);
        hipLaunchKernelGGL(topk_grid_init_kernel, dim3(per_slot), dim3(256), 0, stream, ctl, hist, L.slot_cap);
        for (int level = 0; level < T::LEVELS; ++level) {
            hipLaunchKernelGGL((topk_grid_walk_kernel<T, 0>), dim3(walkers), dim3(kGridThreads), 0, stream, a, ctl, slots, hist, tilecnt, L.slot_cap,
                               L.tile_cap, level);
            hipLaunchKernelGGL(topk_grid_select_kernel, dim3(per_slot), dim3(256), 0, stream, ctl, slots, hist, L.slot_cap, T::B, level);
        }
        hipLaunchKernelGGL((topk_grid_walk_kernel<T, 1>), dim3(walkers), dim3(kGridThreads), 0, stream, a, ctl, slots, hist, tilecnt, L.slot_cap, L.tile_cap, 0);
        hipLaunchKernelGGL(topk_grid_scan_kernel<S>, dim3(per_slot), dim3(1024), 0, stream, a, ctl, slots, tilecnt, L.slot_cap);
        hipLaunchKernelGGL((topk_grid_walk_kernel<T, 2>), dim3(walkers), dim3(kGridThreads), 0, stream, a, ctl, slots, hist, tilecnt, L.slot_cap, L.tile_cap, 0);
    }
    if ((a.flags & kTopkSorted) != 0 && !L.big_sort) {
        if (a.k <= 256u)
            hipLaunchKernelGGL((topk_sort_small_kernel<T, 64, 4>), dim3(grid_of(S_, 16384u)), dim3(64), 0, stream, a);
        else
            hipLaunchKernelGGL((topk_sort_small_kernel<T, 256, 16>), dim3(grid_of(S_, 8192u)), dim3(256), 0, stream, a);
    }
    return hipGetLastError();
}

template <class T>
hipError_t launch_sort_prep_as(hipStream_t stream, const TopkArgs &a, const TopkLayout &L) {
    auto *area = reinterpret_cast<typename T::R *>(a.scratch + L.sort);
    const size_t sk = static_cast<size_t>(a.num_segments) * a.k;
    const uint32_t blocks = grid_of((sk + 255u) / 256u, 8192u);
    hipLaunchKernelGGL(topk_sort_prep_kernel<T>, dim3(blocks), dim3(256), 0, stream, a, area, topk_sort_positions(a, L));
    hipLaunchKernelGGL(topk_sort_offsets_kernel, dim3(grid_of((static_cast<uint64_t>(a.num_segments) + 256u) / 256u, 8192u)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template <class T>
hipError_t launch_sort_back_as(hipStream_t stream, const TopkArgs &a, const TopkLayout &L) {
    auto *area = reinterpret_cast<typename T::R *>(a.scratch + L.sort);
    const size_t sk = static_cast<size_t>(a.num_segments) * a.k;
    hipLaunchKernelGGL(topk_sort_back_kernel<T>, dim3(grid_of((sk + 255u) / 256u, 8192u)), dim3(256), 0, stream, a, area, topk_sort_positions(a, L));
    return hipGetLastError();
}

// the instantiation of a call's key type: the three 32-bit key types share one, the nine dtypes of VRS_TOPK_DTYPE one per width
template <class F>
hipError_t with_traits(int key_type, F f) {
    if (!topk_key_type_torch(key_type)) return f(TopkTraits<uint32_t, uint32_t, false>{});
    switch (topk_elem_bytes(key_type)) {
        case 1: return f(TopkTraits<uint8_t, uint32_t, true>{});
        case 2: return f(TopkTraits<uint16_t, uint32_t, true>{});
        case 4: return f(TopkTraits<uint32_t, uint32_t, true>{});
        default: return f(TopkTraits<uint64_t, uint64_t, true>{});
    }
}

}  // namespace

hipError_t launch_topk(hipStream_t stream, const TopkArgs &a, const TopkLayout &L) {
    return with_traits(a.key_type, [&](auto t) { return launch_topk_as<decltype(t)>(stream, a, L); });
}

hipError_t launch_topk_sort_prep(hipStream_t stream, const TopkArgs &a, const TopkLayout &L) {
    return with_traits(a.key_type, [&](auto t) { return launch_sort_prep_as<decltype(t)>(stream, a, L); });
}

hipError_t launch_topk_sort_back(hipStream_t stream, const TopkArgs &a, const TopkLayout &L) {
    return with_traits(a.key_type, [&](auto t) { return launch_sort_back_as<decltype(t)>(stream, a, L); });
}

static_assert(64 * 4 >= 256 && 256 * 16 >= static_cast<int>(kTopkSortCap), "the sort kernels hold every k they are launched for");

}  // namespace vrs
