// vrs_select.hip -- one-rank selection (vrs_select_segments): entry j of every segment's stable order by radix select, its own bits and
// its index, one sequence of launches whose shapes do not depend on the segments.  Templates: S, the element as the unsigned integer of
// its width (1, 2, 4 or 8 bytes), and R, its rank's type (uint32_t, or uint64_t for 8 bytes).  An element is ranked in registers as it is
// read (select_rank: torch's order), element by element, so a segment may begin at any element offset.
//   classify: top-k's -- one thread per segment; its tier (select_tier, the function vrs_select_tier_for exports), a place on the LDS
//     tier's list (front of one array) or the BLOCK tier's (back of it), or a grid slot with a range of tiles; per-tier counters.
//   selection: digits of at most 11 bits of r from the top (select_level).  A level counts the digit of every key whose higher bits
//     match the prefix chosen so far and picks the digit that holds the need-th key; a segment is done once that bin holds one key, or
//     after the last level.  The first read also counts the keys of the NaN class, which the median modes' target needs (select_target).
//   the index: the answer is the need-th key in index order that matches the final prefix -- a walk that counts, not one that emits.
//   LDS tier (ranks of up to 32 KB): one 256-thread workgroup per segment, ranks read once into LDS.
//   BLOCK tier: one 1024-thread workgroup per segment streaming 16384-key tiles, one read per level; then the tiles in order with a
//     running count up to the tile that holds the need-th.
//   GRID tier: each phase one launch over a fixed grid that walks the tiles of every grid slot (top-k's bookkeeping).  After a level
//     whose chosen bin holds at most len / VRS_TUNE_SELECT_COMPACT_DIVISOR keys (and fits the slot's area), with two levels or more
//     still to come (the copy is itself one read of src, what one level costs), one walk copies the ranks of the matching keys into
//     the slot's area of the scratch buffer, unordered (a ballot and one cursor atomic per wave); the later levels read that area.
//     The index: a counting walk over src (one word per tile), then one workgroup per slot scans the words to the holding tile and
//     reads that one tile.
// Loops whose bound may come near 2^32 (grid strides, a segment's tiles) count in 64 bits: a 32-bit i + step would wrap below the bound.
#include "vrs_select.hpp"

#include "vrs_radix_select.hpp"

namespace vrs {
namespace {

template <typename R>
__device__ __forceinline__ bool sel_match(R r, const SelState<R> &s) {
    return s.shift == kSelNoShift || (r >> s.shift) == (s.prefix >> s.shift);
}

// the call's rank map: load(p) of every kernel is rank(src[p])
template <typename S, typename R>
struct RankOf {
    static constexpr int B = 8 * static_cast<int>(sizeof(S));
    int kind;
    R inf_bits, nan_rank;  // nan_rank: the rank of every NaN (meaningful for floats only)
    bool descending;
    __device__ __forceinline__ R operator()(S x) const { return select_rank<R, B>(static_cast<R>(x), kind, inf_bits, descending); }
};
template <typename S, typename R>
__device__ __forceinline__ RankOf<S, R> rank_of(const SelectArgs &a) {
    constexpr int B = RankOf<S, R>::B;
    constexpr R sign = static_cast<R>(1) << (B - 1), ones = sign | (sign - 1);
    RankOf<S, R> f;
    f.kind = select_kind(a.dtype);
    f.inf_bits = a.dtype == kSortF16    ? static_cast<R>(0x7C00u)
                 : a.dtype == kSortBF16 ? static_cast<R>(0x7F80u)
                 : a.dtype == kSortF32  ? static_cast<R>(0x7F800000u)
                                        : static_cast<R>(0x7FF0000000000000ull);
    f.descending = (a.flags & kSelDescending) != 0;
    f.nan_rank = f.descending ? static_cast<R>(0) : ones;
    return f;
}

// The digit histogram of the keys of one tile that match the selection so far; position p of the tile: load(p).  Returns the calling
// thread's keys of the NaN class when `nans` asks for them.
template <int THREADS, int ITEMS, typename R, class Load>
__device__ __forceinline__ uint32_t hist_tile(Load load, uint32_t cnt, const SelState<R> &sel, uint32_t shift, uint32_t mask, bool nans,
                                              R nan_rank, uint32_t *s_hist) {
    R r[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = i * THREADS + threadIdx.x;
        r[i] = p < cnt ? load(p) : static_cast<R>(0);
    }
    uint32_t nn = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = i * THREADS + threadIdx.x;
        if (p < cnt) {
            if (nans && r[i] == nan_rank) ++nn;
            if (sel_match(r[i], sel)) hist_add(s_hist, static_cast<uint32_t>(r[i] >> shift) & mask);
        }
    }
    return nn;
}

template <typename R>
__device__ __forceinline__ void sel_apply(SelState<R> &sel, int bits, int level, uint32_t d, uint32_t below, uint32_t at) {
    uint32_t shift, mask;
    select_level(bits, level, &shift, &mask);
    sel.need -= below;
    sel.shift = shift;
    sel.prefix |= static_cast<R>(d) << shift;
    sel.done = (at == 1u || level == select_levels(bits) - 1) ? 1u : 0u;
}

// One tile in index order (position p = i * THREADS + tid; match(p): the key at p matches the selection).  Returns the tile's matching
// keys; when it holds the want-th of them (1 <= want <= the return value), the thread that has it calls found(p).
template <int THREADS, int ITEMS, class Match, class Found>
__device__ __forceinline__ uint32_t locate_tile(Match match, uint32_t cnt, uint32_t want, uint32_t *s_cnt, uint32_t *s_wtot, uint32_t *s_hold,
                                                Found found) {
    constexpr int WAVES = THREADS / 64, E = ITEMS * WAVES;
    static_assert(E % 64 == 0 && E <= THREADS && E / 64 <= 16, "one scanning thread per (item, wave)");
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const uint32_t p = i * THREADS + tid;
        const uint64_t bal = __ballot(p < cnt && match(p));
        if (lane == 0u) s_cnt[i * WAVES + wave] = static_cast<uint32_t>(__popcll(bal));
    }
    __syncthreads();
    uint32_t c = 0, incl = 0;
    if (tid < static_cast<uint32_t>(E)) {
        c = s_cnt[tid];
        incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o);
            if (lane >= static_cast<uint32_t>(o)) incl += t;
        }
        if (lane == 63u) s_wtot[wave] = incl;
    }
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (int v = 0; v < E / 64; ++v) total += s_wtot[v];
    if (tid < static_cast<uint32_t>(E)) {
        uint32_t excl = incl - c;
        for (uint32_t v = 0; v < wave; ++v) excl += s_wtot[v];
        if (excl < want && want <= excl + c) {  // exactly one thread, when the tile holds the want-th
            s_hold[0] = tid;
            s_hold[1] = want - excl;
        }
    }
    __syncthreads();
    if (want <= total) {
        const uint32_t e = s_hold[0], within = s_hold[1];
        if (wave == e % WAVES) {
            const uint32_t p = (e / WAVES) * THREADS + tid;
            const bool m = p < cnt && match(p);
            const uint64_t bal = __ballot(m);
            if (m && count_below(bal) + 1u == within) found(p);
        }
    }
    __syncthreads();  // (s_cnt, s_wtot and s_hold are free again)
    return total;
}

template <typename S>
__device__ __forceinline__ void write_none(const SelectArgs &a, uint32_t seg) {
    static_cast<S *>(a.out_values)[seg] = static_cast<S>(0);
    if (a.out_indices) a.out_indices[seg] = 0xFFFFFFFFu;
}
template <typename S>
__device__ __forceinline__ void write_found(const SelectArgs &a, uint32_t seg, const S *src, uint32_t pos) {
    static_cast<S *>(a.out_values)[seg] = src[pos];
    if (a.out_indices) a.out_indices[seg] = pos;
}

__global__ __launch_bounds__(256) void select_classify_kernel(SelectArgs a, TopkControl *__restrict__ ctl, uint32_t *__restrict__ list,
                                                              SelSlot *__restrict__ slots, uint32_t slot_cap, uint32_t tile_cap) {
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
                SelSlot s{};
                s.seg = i;
                s.b = cb;
                s.len = len;
                s.tile_base = base;
                s.tiles = tiles;
                s.valid = valid ? 1u : 0u;
                s.ok = (a.mode != kSelKth || a.k <= len) ? 1u : 0u;  // (the median modes: a grid slot is never empty)
                s.shift = kSelNoShift;
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
template <typename S, typename R, int THREADS, int ITEMS, bool LDS>
__global__ __launch_bounds__(THREADS) void select_workgroup_kernel(SelectArgs a, const TopkControl *__restrict__ ctl, const uint32_t *__restrict__ list) {
    constexpr int B = 8 * static_cast<int>(sizeof(S)), LEVELS = (B + 10) / 11, TILE = THREADS * ITEMS, E = ITEMS * (THREADS / 64);
    static_assert(!LDS || TILE * sizeof(R) == kSelLdsBytes, "the LDS tier's segment is one tile");
    __shared__ uint32_t s_hist[kTopkBins];
    __shared__ R s_r[LDS ? TILE : 1];
    __shared__ uint32_t s_cnt[E];
    __shared__ uint32_t s_wtot[16];
    __shared__ uint32_t s_res[3], s_hold[2], s_nans;
    const uint32_t tid = threadIdx.x;
    const uint32_t count = LDS ? ctl->lds_count : ctl->block_count;
    const RankOf<S, R> rank = rank_of<S, R>(a);
    const bool count_nans = rank.kind == kSelFloat && a.mode != kSelKth;
    for (size_t jw = blockIdx.x; jw < count; jw += gridDim.x) {
        const uint32_t j = static_cast<uint32_t>(jw);
        const uint32_t seg = LDS ? list[j] : list[a.num_segments - 1u - j];
        uint32_t b, e;
        (void)topk_tier(a.offsets[seg], a.offsets[seg + 1u], a.n, 0u, &b, &e);
        const uint32_t len = e - b;
        const S *src = static_cast<const S *>(a.src) + b;
        if (len == 0u) {
            if (tid == 0u) write_none<S>(a, seg);
            continue;
        }
        if (tid == 0u) s_nans = 0u;
        __syncthreads();
        if constexpr (LDS) {
            uint32_t nn = 0;
            for (uint32_t p = tid; p < len; p += THREADS) {
                const R r = rank(src[p]);
                s_r[p] = r;
                if (count_nans && r == rank.nan_rank) ++nn;
            }
            if (nn != 0u) atomicAdd(&s_nans, nn);
            __syncthreads();
        }
        SelState<R> sel{static_cast<R>(0), kSelNoShift, 0u, 0u};
        bool ok = true;
        for (int level = 0; level < LEVELS && ok && !sel.done; ++level) {
            for (uint32_t c = tid; c < kTopkBins; c += THREADS) s_hist[c] = 0u;
            __syncthreads();
            uint32_t shift, mask, nn = 0;
            select_level(B, level, &shift, &mask);
            for (uint64_t tile0 = 0; tile0 < len; tile0 += TILE) {  // (64-bit: a 32-bit t0 + TILE wraps below len near 2^32)
                const uint32_t t0 = static_cast<uint32_t>(tile0), cnt = min(static_cast<uint32_t>(TILE), len - t0);
                if constexpr (LDS)
                    (void)hist_tile<THREADS, ITEMS>([&](uint32_t p) { return s_r[t0 + p]; }, cnt, sel, shift, mask, false, rank.nan_rank, s_hist);
                else
                    nn += hist_tile<THREADS, ITEMS>([&](uint32_t p) { return rank(src[t0 + p]); }, cnt, sel, shift, mask, count_nans && level == 0,
                                                    rank.nan_rank, s_hist);
            }
            if (nn != 0u) atomicAdd(&s_nans, nn);
            __syncthreads();
            if (level == 0) {  // the target: known once the first read has counted the NaN class
                const uint32_t nans = s_nans;
                uint32_t jt;
                ok = select_target(a.mode, a.k, len, nans, rank.descending, &jt);
                sel.need = jt + 1u;
                __syncthreads();  // (s_nans is read before the next segment clears it)
                if (!ok) break;
            }
            select_digit<THREADS>(s_hist, sel.need, s_wtot, s_res);
            sel_apply(sel, B, level, s_res[0], s_res[1], s_res[2]);
            __syncthreads();
        }
        if (!ok) {
            if (tid == 0u) write_none<S>(a, seg);
            continue;
        }
        uint32_t before = 0;  // matching keys in the tiles walked so far
        for (uint64_t tile0 = 0; tile0 < len; tile0 += TILE) {
            const uint32_t t0 = static_cast<uint32_t>(tile0), cnt = min(static_cast<uint32_t>(TILE), len - t0), want = sel.need - before;
            auto found = [&](uint32_t p) { write_found<S>(a, seg, src, t0 + p); };
            uint32_t total;
            if constexpr (LDS) total = locate_tile<THREADS, ITEMS>([&](uint32_t p) { return sel_match(s_r[t0 + p], sel); }, cnt, want, s_cnt, s_wtot, s_hold, found);
            else total = locate_tile<THREADS, ITEMS>([&](uint32_t p) { return sel_match(rank(src[t0 + p]), sel); }, cnt, want, s_cnt, s_wtot, s_hold, found);
            if (want <= total) break;
            before += total;
        }
    }
}

// ---- GRID tier: kernels that walk the virtual tiles [0, tiles taken) of every slot ----
constexpr int kGridThreads = 1024, kGridItems = 16;
static_assert(kGridThreads * kGridItems == static_cast<int>(kTopkTile), "a grid tile is one pass of a workgroup");

__global__ __launch_bounds__(256) void select_grid_init_kernel(const TopkControl *__restrict__ ctl, uint32_t *__restrict__ hist, uint32_t slot_cap) {
    const uint32_t ns = grid_slots(ctl, slot_cap);
    for (size_t s = blockIdx.x; s < ns; s += gridDim.x)
        for (uint32_t c = threadIdx.x; c < kTopkBins; c += 256u) hist[s * kTopkBins + c] = 0u;
}

constexpr int kWalkHist = 0, kWalkCompact = 1, kWalkCount = 2;

// PHASE kWalkHist: digit histograms of level `level` (of src, or of a compacted slot's area; level 0 also counts the NaN class);
// kWalkCompact: the ranks of the matching keys of every slot that has just qualified, into its area; kWalkCount: per-tile counts of the
// keys of src that match the final prefix
template <typename S, typename R, int PHASE>
__global__ __launch_bounds__(kGridThreads) void select_grid_walk_kernel(SelectArgs a, const TopkControl *__restrict__ ctl, SelSlot *slots,
                                                                        uint32_t *__restrict__ hist, uint32_t *__restrict__ tilecnt,
                                                                        R *__restrict__ area, uint32_t slot_cap, uint32_t tile_cap, int level) {
    constexpr int B = 8 * static_cast<int>(sizeof(S));
    __shared__ uint32_t s_hist[PHASE == kWalkHist ? kTopkBins : 1];
    __shared__ uint32_t s_slot, s_count, s_nans;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t ns = grid_slots(ctl, slot_cap), total = grid_tiles(ctl, slot_cap, tile_cap);
    const RankOf<S, R> rank = rank_of<S, R>(a);
    const bool count_nans = rank.kind == kSelFloat && a.mode != kSelKth && level == 0;
    if constexpr (PHASE == kWalkHist) {
        for (uint32_t c = tid; c < kTopkBins; c += kGridThreads) s_hist[c] = 0u;
        if (tid == 0u) s_nans = 0u;
    }
    uint32_t cur = 0xFFFFFFFFu;
    bool dirty = false;
    auto flush = [&]() {  // the workgroup's counts of slot `cur` into the slot's: one atomic per non-zero bin
        __syncthreads();
        for (uint32_t c = tid; c < kTopkBins; c += kGridThreads) {
            const uint32_t v = s_hist[c];
            if (v != 0u) {
                atomicAdd(&hist[static_cast<size_t>(cur) * kTopkBins + c], v);
                s_hist[c] = 0u;
            }
        }
        if (tid == 0u && s_nans != 0u) {
            atomicAdd(&slots[cur].nans, s_nans);
            s_nans = 0u;
        }
        __syncthreads();
    };
    for (size_t tw = blockIdx.x; tw < total; tw += gridDim.x) {
        const uint32_t t = static_cast<uint32_t>(tw);
        if (tid == 0u) s_slot = find_slot(slots, ns, t);
        __syncthreads();
        const uint32_t s = s_slot;
        __syncthreads();
        if constexpr (PHASE == kWalkHist) {
            if (s != cur) {
                if (dirty) {
                    flush();
                    dirty = false;
                }
                cur = s;
            }
        }
        const SelSlot *sl = &slots[s];
        const uint32_t ti = t - sl->tile_base, len = sl->len;
        if (!sl->valid || !sl->ok || ti >= sl->tiles) continue;
        const SelState<R> sel{static_cast<R>(sl->prefix), sl->shift, sl->need, sl->done};
        const uint32_t off = ti * kTopkTile;  // (below len)
        const S *src = static_cast<const S *>(a.src) + sl->b + off;
        auto load = [&](uint32_t p) { return rank(src[p]); };
        if constexpr (PHASE == kWalkHist) {
            if (sel.done) continue;
            uint32_t shift, mask;
            select_level(B, level, &shift, &mask);
            if (sl->state != 0u) {  // compacted: its first ccount / 16384 tiles stand for the area's
                const uint32_t have = sl->ccount;
                if (off >= have) continue;
                const R *ar = area + static_cast<size_t>(sl->tile_base) * kSelAreaPerTile + off;
                (void)hist_tile<kGridThreads, kGridItems>([&](uint32_t p) { return ar[p]; }, min(kTopkTile, have - off), sel, shift, mask, false,
                                                          rank.nan_rank, s_hist);
            } else {
                const uint32_t nn = hist_tile<kGridThreads, kGridItems>(load, min(kTopkTile, len - off), sel, shift, mask, count_nans, rank.nan_rank, s_hist);
                if (nn != 0u) atomicAdd(&s_nans, nn);
            }
            dirty = true;
        } else if constexpr (PHASE == kWalkCompact) {
            if (sl->state != 1u) continue;
            const uint32_t cnt = min(kTopkTile, len - off), room = sl->ccount;
            R *ar = area + static_cast<size_t>(sl->tile_base) * kSelAreaPerTile;
            R r[kGridItems];
#pragma unroll
            for (int i = 0; i < kGridItems; ++i) {
                const uint32_t p = i * kGridThreads + tid;
                r[i] = p < cnt ? load(p) : static_cast<R>(0);
            }
            uint32_t mine = 0, wave_total = 0;  // bit i of mine: this lane's item i matches
#pragma unroll
            for (int i = 0; i < kGridItems; ++i) {
                const uint32_t p = i * kGridThreads + tid;
                const bool m = p < cnt && sel_match(r[i], sel);
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
        } else {
            if (tid == 0u) s_count = 0u;
            __syncthreads();
            const uint32_t cnt = min(kTopkTile, len - off);
            R r[kGridItems];
#pragma unroll
            for (int i = 0; i < kGridItems; ++i) {
                const uint32_t p = i * kGridThreads + tid;
                r[i] = p < cnt ? load(p) : static_cast<R>(0);
            }
            uint32_t nm = 0;
#pragma unroll
            for (int i = 0; i < kGridItems; ++i) {
                const uint32_t p = i * kGridThreads + tid;
                nm += static_cast<uint32_t>(__popcll(__ballot(p < cnt && sel_match(r[i], sel))));
            }
            if (lane == 0u && nm != 0u) atomicAdd(&s_count, nm);
            __syncthreads();
            if (tid == 0u) tilecnt[t] = s_count;
            __syncthreads();
        }
    }
    if constexpr (PHASE == kWalkHist)
        if (dirty) flush();
}

// One workgroup per slot: the digit of level `level` from the slot's histogram (zeroed behind it for the next level); at level 0 the
// target from the NaN count first.  A slot whose chosen bin is small enough (and fits its area) compacts after this level.
__global__ __launch_bounds__(256) void select_grid_select_kernel(SelectArgs a, const TopkControl *__restrict__ ctl, SelSlot *__restrict__ slots,
                                                                 uint32_t *__restrict__ hist, uint32_t slot_cap, int bits, int level) {
    __shared__ uint32_t s_hist[kTopkBins];
    __shared__ uint32_t s_wtot[4], s_res[3];
    const uint32_t ns = grid_slots(ctl, slot_cap);
    for (size_t sw = blockIdx.x; sw < ns; sw += gridDim.x) {
        const uint32_t s = static_cast<uint32_t>(sw);
        SelSlot sl = slots[s];
        if (!sl.valid || !sl.ok || sl.done) continue;
        uint32_t *h = hist + static_cast<size_t>(s) * kTopkBins;
        for (uint32_t c = threadIdx.x; c < kTopkBins; c += 256u) {
            s_hist[c] = h[c];
            h[c] = 0u;
        }
        __syncthreads();
        if (level == 0) {
            uint32_t jt;
            (void)select_target(a.mode, a.k, sl.len, sl.nans, (a.flags & kSelDescending) != 0, &jt);  // (ok: the classification saw to it)
            sl.need = jt + 1u;
        }
        select_digit<256>(s_hist, sl.need, s_wtot, s_res);
        SelState<unsigned long long> sel{sl.prefix, sl.shift, sl.need, 0u};
        const uint32_t at = s_res[2];
        sel_apply(sel, bits, level, s_res[0], s_res[1], at);
        sl.prefix = sel.prefix;
        sl.shift = sel.shift;
        sl.need = sel.need;
        sl.done = sel.done;
        bool compacts = false;
        if (sl.state == 1u) {
            sl.state = 2u;
        } else if (sl.state == 0u && !sl.done && level + 2 < select_levels(bits) && a.compact_divisor != 0u && at <= sl.len / a.compact_divisor &&
                   at <= sl.tiles * kSelAreaPerTile) {  // (two levels left at least: the copy costs the read it saves when one is)
            compacts = true;
            sl.state = 1u;
            sl.ccount = at;
            sl.cursor = 0u;
        }
        if (threadIdx.x == 0u) {
            slots[s] = sl;
            if (compacts) atomicAdd(&a.stats[3], 1ull);
        }
        __syncthreads();
    }
}

// One workgroup per slot: the tiles' counts, in tile order, up to the tile that holds the need-th matching key; then that tile of src.
template <typename S, typename R>
__global__ __launch_bounds__(kGridThreads) void select_grid_locate_kernel(SelectArgs a, const TopkControl *__restrict__ ctl,
                                                                          const SelSlot *__restrict__ slots, const uint32_t *__restrict__ tilecnt,
                                                                          uint32_t slot_cap) {
    constexpr int E = kGridItems * (kGridThreads / 64);
    __shared__ uint32_t s_cnt[E];
    __shared__ uint32_t s_wtot[16];
    __shared__ uint32_t s_hold[2], s_tile[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t ns = grid_slots(ctl, slot_cap);
    const RankOf<S, R> rank = rank_of<S, R>(a);
    for (size_t sw = blockIdx.x; sw < ns; sw += gridDim.x) {
        const SelSlot sl = slots[sw];
        if (!sl.valid) continue;
        if (!sl.ok) {
            if (tid == 0u) write_none<S>(a, sl.seg);
            continue;
        }
        const SelState<R> sel{static_cast<R>(sl.prefix), sl.shift, sl.need, sl.done};
        uint32_t carry = 0;  // matching keys in the tiles scanned so far
        for (uint32_t t0 = 0; t0 < sl.tiles && carry < sel.need; t0 += kGridThreads) {
            const uint32_t t = t0 + tid;
            const uint32_t c = t < sl.tiles ? tilecnt[sl.tile_base + t] : 0u;
            uint32_t incl = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = __shfl_up(incl, o);
                if (lane >= static_cast<uint32_t>(o)) incl += v;
            }
            if (lane == 63u) s_wtot[wave] = incl;
            __syncthreads();
            uint32_t excl = carry + incl - c, all = carry;
            for (uint32_t w = 0; w < 16u; ++w) {
                if (w < wave) excl += s_wtot[w];
                all += s_wtot[w];
            }
            if (excl < sel.need && sel.need <= excl + c) {  // exactly one thread of one round
                s_tile[0] = t;
                s_tile[1] = sel.need - excl;
            }
            carry = all;
            __syncthreads();
        }
        if (carry < sel.need) continue;  // (src changed under the call: nothing is written)
        const uint32_t off = s_tile[0] * kTopkTile, want = s_tile[1];
        const S *seg_src = static_cast<const S *>(a.src) + sl.b;
        const S *src = seg_src + off;
        (void)locate_tile<kGridThreads, kGridItems>([&](uint32_t p) { return sel_match(rank(src[p]), sel); }, min(kTopkTile, sl.len - off), want, s_cnt,
                                                    s_wtot, s_hold, [&](uint32_t p) { write_found<S>(a, sl.seg, seg_src, off + p); });
    }
}

uint32_t grid_of(uint64_t work, uint32_t cap) { return static_cast<uint32_t>(std::max<uint64_t>(1u, std::min<uint64_t>(work, cap))); }

template <typename S, typename R>
hipError_t launch_select_as(hipStream_t stream, const SelectArgs &a, const SelLayout &L) {
    constexpr int B = 8 * static_cast<int>(sizeof(S)), LEVELS = (B + 10) / 11, LDS_ITEMS = static_cast<int>(kSelLdsBytes / sizeof(R)) / 256;
    auto *ctl = reinterpret_cast<TopkControl *>(a.scratch + L.control);
    auto *list = reinterpret_cast<uint32_t *>(a.scratch + L.list);
    auto *slots = reinterpret_cast<SelSlot *>(a.scratch + L.slots);
    auto *hist = reinterpret_cast<uint32_t *>(a.scratch + L.hist);
    auto *tilecnt = reinterpret_cast<uint32_t *>(a.scratch + L.tiles);
    auto *area = reinterpret_cast<R *>(a.scratch + L.area);
    hipError_t e = hipMemsetAsync(ctl, 0, sizeof(TopkControl), stream);
    if (e != hipSuccess) return e;
    const uint32_t S_ = a.num_segments;
    hipLaunchKernelGGL(select_classify_kernel, dim3(grid_of((static_cast<uint64_t>(S_) + 255u) / 256u, 0xFFFFFFFFu)), dim3(256), 0, stream, a, ctl, list,
                       slots, L.slot_cap, L.tile_cap);
    hipLaunchKernelGGL((select_workgroup_kernel<S, R, 256, LDS_ITEMS, true>), dim3(grid_of(S_, 8192u)), dim3(256), 0, stream, a, ctl, list);
    if (a.n > kSelLdsBytes / sizeof(R))  // (else no segment is longer than the LDS tier's cap)
        hipLaunchKernelGGL((select_workgroup_kernel<S, R, 1024, 16, false>), dim3(grid_of(S_, 1024u)), dim3(1024), 0, stream, a, ctl, list);
    if (L.slot_cap != 0u && a.grid_min_keys != 0u && a.n >= a.grid_min_keys) {
        const uint32_t walkers = grid_of(L.tile_cap, 1024u), per_slot = grid_of(L.slot_cap, 1024u);
        hipLaunchKernelGGL(select_grid_init_kernel, dim3(per_slot), dim3(256), 0, stream, ctl, hist, L.slot_cap);
        for (int level = 0; level < LEVELS; ++level) {
            hipLaunchKernelGGL((select_grid_walk_kernel<S, R, kWalkHist>), dim3(walkers), dim3(kGridThreads), 0, stream, a, ctl, slots, hist, tilecnt, area,
                               L.slot_cap, L.tile_cap, level);
            hipLaunchKernelGGL(select_grid_select_kernel, dim3(per_slot), dim3(256), 0, stream, a, ctl, slots, hist, L.slot_cap, B, level);
            if (level + 2 < LEVELS && a.compact_divisor != 0u)  // (the copy is one read of src: it pays when two levels or more are left)
                hipLaunchKernelGGL((select_grid_walk_kernel<S, R, kWalkCompact>), dim3(walkers), dim3(kGridThreads), 0, stream, a, ctl, slots, hist, tilecnt,
                                   area, L.slot_cap, L.tile_cap, level);
        }
        hipLaunchKernelGGL((select_grid_walk_kernel<S, R, kWalkCount>), dim3(walkers), dim3(kGridThreads), 0, stream, a, ctl, slots, hist, tilecnt, area,
                           L.slot_cap, L.tile_cap, 0);
        hipLaunchKernelGGL((select_grid_locate_kernel<S, R>), dim3(per_slot), dim3(kGridThreads), 0, stream, a, ctl, slots, tilecnt, L.slot_cap);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_select(hipStream_t stream, const SelectArgs &a, const SelLayout &L) {
    switch (sort_dtype_bytes(a.dtype)) {
        case 1: return launch_select_as<uint8_t, uint32_t>(stream, a, L);
        case 2: return launch_select_as<uint16_t, uint32_t>(stream, a, L);
        case 4: return launch_select_as<uint32_t, uint32_t>(stream, a, L);
        default: return launch_select_as<uint64_t, uint64_t>(stream, a, L);
    }
}

}  // namespace vrs
