// vrs_segreduce.hip -- the segmented reduction over rows (vrs_segment_reduce), gfx950, wave64: every segment of rows of C columns reduced
// in the fixed order of vrs_reduce_order.hpp, without a float atomic and without waiting for the host.
//
//   classify   one thread per segment: segments of at most LANE_ROWS rows with C < 64 go to the lane list; every other segment is cut
//              into chunk items of CH rows, level by level (a level's partial rows are reserved with one integer atomic per segment:
//              WHERE a partial row sits varies from run to run, what it holds does not), until one chunk is left: the final item.
//   lane       256 threads over consecutive (listed segment, column) pairs, the rows in order.
//   rows       C < 64: one wave per chunk item, the wave G = 64 / C' row groups of C' columns, combined with __shfl_xor.
//   columns    C >= 64: one wave per (chunk item, slab of 64 lanes x 16 bytes of columns), the rows in order.
// One launch of rows / columns per level; their grids are host-side upper bounds and every workgroup reads the real counts from the
// control block.  A work list's order may vary; each out element is written once, by the one thread that owns it.
#include "vrs_segreduce.hpp"

namespace vrs {

namespace {

constexpr uint32_t kThreads = 256u, kWaves = kThreads / 64u;
constexpr uint32_t kInlineItems = 8u;               // a classify thread writes up to this many items itself; longer runs are written by its workgroup
constexpr uint32_t kQueueCap = kThreads * 6u;       // runs of items left to the workgroup: fewer than one per thread and level
constexpr uint32_t kRowsInFlight = 4u;              // rows loaded before they are combined, in order

struct ReduceDev {
    ReduceControl *ctl;
    uint32_t *list;
    ReduceItem *items[kReduceMaxLevels];
    uint32_t item_cap[kReduceMaxLevels], part_cap[kReduceMaxLevels], levels;
};

struct ItemRun {
    uint32_t level_final, src, len, dst, at;  // level | final << 8; dst: the segment (final) or the first partial row; at: the first item
};

__device__ inline void write_items(const ReduceDev &d, const ItemRun &r, uint32_t CH, uint32_t first, uint32_t step) {
    const uint32_t level = r.level_final & 0xFFu;
    const bool final = (r.level_final >> 8) != 0u;
    const uint32_t count = final ? 1u : reduce_chunks(r.len, CH);
    for (uint32_t c = first; c < count; c += step) {
        const uint32_t begin = c * CH, len = std::min(CH, r.len - begin);
        ReduceItem it;
        it.src = r.src + begin;
        it.len_final = len | (final ? kReduceItemFinal : 0u);
        it.dst = final ? r.dst : r.dst + c;
        it.unused = 0u;
        d.items[level][r.at + c] = it;
    }
}

__global__ __launch_bounds__(kThreads) void reduce_classify_kernel(SegReduceArgs a, ReduceDev d) {
    __shared__ uint32_t s_stat[4];
    __shared__ uint32_t s_queued;
    __shared__ ItemRun s_queue[kQueueCap];
    const uint32_t tid = threadIdx.x, CH = a.chunk_rows;
    if (tid < 4u) s_stat[tid] = 0u;
    if (tid == 0u) s_queued = 0u;
    __syncthreads();
    const uint64_t i64 = static_cast<uint64_t>(blockIdx.x) * kThreads + tid;
    if (i64 < a.num_segments) {
        const uint32_t i = static_cast<uint32_t>(i64);
        const uint32_t b = a.offsets[i], e = a.offsets[i + 1u];
        const uint32_t cb = b < a.n ? b : a.n, hi = e > b ? e : b, ce = hi < a.n ? hi : a.n;  // (vrs_segment_tier_for's clamp)
        const uint32_t L = ce - cb;
        if (reduce_map(L, a.C, a.lane_rows) == kReduceMapLane) {
            d.list[atomicAdd(&d.ctl->lane_count, 1u)] = i;
            atomicAdd(&s_stat[kReduceMapLane], 1u);
            atomicMax(&s_stat[3], 1u);
        } else {
            uint32_t src = cb, len = L, level = 0u;
            bool ok = true;
            for (;;) {
                const uint32_t chunks = reduce_chunks(len, CH);
                const bool final = chunks == 1u;
                const uint32_t at = atomicAdd(&d.ctl->item_count[level], chunks);
                if (static_cast<uint64_t>(at) + chunks > d.item_cap[level]) ok = false;
                uint32_t part = 0u;
                if (ok && !final) {
                    if (level + 1u >= d.levels) {
                        ok = false;
                    } else {
                        part = atomicAdd(&d.ctl->part_rows[level + 1u], chunks);
                        if (static_cast<uint64_t>(part) + chunks > d.part_cap[level + 1u]) ok = false;
                    }
                }
                if (!ok) break;  // (only segments that overlap get here: the bounds hold for every other input)
                const ItemRun run{level | (final ? 0x100u : 0u), src, len, final ? i : part, at};
                if (chunks <= kInlineItems) write_items(d, run, CH, 0u, 1u);
                else s_queue[atomicAdd(&s_queued, 1u)] = run;
                // the chunks' maps: chunks - 1 of CH rows and the last one
                const uint32_t last = len - (chunks - 1u) * CH;
                if (chunks > 1u) atomicAdd(&s_stat[reduce_map(CH, a.C, a.lane_rows)], chunks - 1u);
                atomicAdd(&s_stat[reduce_map(last, a.C, a.lane_rows)], 1u);
                if (final) break;
                src = part;
                len = chunks;
                ++level;
            }
            if (ok) atomicMax(&s_stat[3], level + 1u);
            else d.list[a.num_segments - 1u - atomicAdd(&d.ctl->fail_count, 1u)] = i;
        }
    }
    __syncthreads();
    const uint32_t queued = s_queued;
    for (uint32_t q = 0; q < queued; ++q) write_items(d, s_queue[q], CH, tid, kThreads);
    if (tid < 3u && s_stat[tid] != 0u) atomicAdd(&a.stats[tid], static_cast<unsigned long long>(s_stat[tid]));
    if (tid == 3u && s_stat[3] != 0u) atomicMax(&a.stats[3], static_cast<unsigned long long>(s_stat[3]));
}

// element i of a buffer of T's storage, widened / an accumulator narrowed into it
template <typename T>
__device__ inline typename T::A load_as(const void *p, size_t i) { return reduce_widen<T>(static_cast<const typename T::S *>(p)[i]); }
template <typename T>
__device__ inline void store_as(void *p, size_t i, typename T::A v) { static_cast<typename T::S *>(p)[i] = reduce_narrow<T>(v); }

// reduce(rows) of (segment, column) becomes the out element: op(init, it), init's own bits for a segment without rows
template <typename T>
__device__ inline void finish(const SegReduceArgs &a, uint32_t seg, uint32_t col, typename T::A acc, bool empty) {
    const size_t at = static_cast<size_t>(seg) * a.C + col;
    using S = typename T::S;
    if (a.init && empty) {
        static_cast<S *>(a.out)[at] = static_cast<const S *>(a.init)[at];
        return;
    }
    if (a.init) acc = reduce_combine(a.op, load_as<T>(a.init, at), acc);
    store_as<T>(a.out, at, acc);
}

// the partials of a level are rows of accumulators
template <typename Acc>
struct ReducePartial { using S = Acc; using A = Acc; };

__device__ inline uint32_t row_number(const SegReduceArgs &a, uint32_t i) { return std::min(a.order[i], a.n - 1u); }

// lane map: thread <-> (listed segment, column), the rows in order.  The entries behind the lane list are the segments that found no
// room for their items (overlapping ranges only): they answer as segments without rows.
template <typename T>
__global__ __launch_bounds__(kThreads) void reduce_lane_kernel(SegReduceArgs a, ReduceDev d) {
    using A = typename T::A;
    const uint32_t lanes = std::min(d.ctl->lane_count, a.num_segments);
    const uint32_t fails = std::min(d.ctl->fail_count, a.num_segments - lanes);
    const uint64_t total = (static_cast<uint64_t>(lanes) + fails) * a.C;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; g < total; g += static_cast<uint64_t>(gridDim.x) * kThreads) {
        const uint32_t entry = static_cast<uint32_t>(g / a.C), col = static_cast<uint32_t>(g % a.C);
        const bool failed = entry >= lanes;
        const uint32_t seg = failed ? d.list[a.num_segments - 1u - (entry - lanes)] : d.list[entry];
        if (seg >= a.num_segments) continue;
        const uint32_t b = a.offsets[seg], e = a.offsets[seg + 1u];
        const uint32_t cb = b < a.n ? b : a.n, hi = e > b ? e : b, ce = hi < a.n ? hi : a.n;
        const uint32_t L = failed ? 0u : std::min(ce - cb, a.lane_rows);
        A acc = reduce_identity<A>(a.op);
        for (uint32_t t = 0; t < L; ++t) {
            const uint32_t row = a.order ? row_number(a, cb + t) : cb + t;
            acc = reduce_combine(a.op, acc, load_as<T>(a.values, static_cast<size_t>(row) * a.C + col));
        }
        finish<T>(a, seg, col, acc, L == 0u);
    }
}

// what a rows / columns launch reads and writes
struct LevelArgs {
    const void *src;      // values (level 0) or the level's partials
    void *next;           // the next level's partials (NULL at the last level)
    const ReduceItem *items;
    const uint32_t *item_count;
    uint32_t item_cap, src_rows, next_rows, level;
    int vec_ok;           // columns: every row of src starts on a 16-byte boundary
};

// an item as a kernel may use it: false for a slot that was never written (a reservation that did not fit) or does not fit its buffers
__device__ inline bool item_ok(const LevelArgs &v, const SegReduceArgs &a, const ReduceItem &it, uint32_t *len, bool *final) {
    *len = it.len_final & ~kReduceItemFinal;
    *final = (it.len_final & kReduceItemFinal) != 0u;
    if (*len > a.chunk_rows || static_cast<uint64_t>(it.src) + *len > v.src_rows) return false;
    return *final ? it.dst < a.num_segments : (v.next != nullptr && it.dst < v.next_rows);
}

// rows map: one wave per item.  X: how the level's source is stored, T: the dtype of the call.
template <typename X, typename T>
__global__ __launch_bounds__(kThreads) void reduce_rows_kernel(SegReduceArgs a, LevelArgs v, uint32_t padded) {
    using A = typename T::A;
    const uint32_t lane = threadIdx.x & 63u, C = a.C;
    const uint32_t G = 64u / padded, group = lane / padded, col = lane & (padded - 1u);
    const bool column = col < C;
    const bool gather = v.level == 0u && a.order != nullptr;
    const uint32_t count = std::min(*v.item_count, v.item_cap);
    const A identity = reduce_identity<A>(a.op);
    for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * kWaves + threadIdx.x / 64u; w < count; w += static_cast<uint64_t>(gridDim.x) * kWaves) {
        const ReduceItem it = v.items[w];
        uint32_t len;
        bool final;
        if (!item_ok(v, a, it, &len, &final)) continue;
        const bool one = reduce_map(len, C, a.lane_rows) == kReduceMapLane;  // a short chunk: one accumulator, the rows in order
        const uint32_t step = one ? 1u : G, first = one ? 0u : group;
        const bool adds = column && (!one || group == 0u);
        A acc = identity;
        for (uint32_t base = 0; base < len; base += 64u) {
            const uint32_t rows = std::min(64u, len - base);
            uint32_t mine = 0u;  // the chunk's row numbers, 64 at a time, one per lane
            if (gather && lane < rows) mine = row_number(a, it.src + base + lane);
            for (uint32_t t0 = 0; t0 < rows; t0 += step * kRowsInFlight) {
                A got[kRowsInFlight];
#pragma unroll
                for (uint32_t j = 0; j < kRowsInFlight; ++j) {
                    const uint32_t t = t0 + j * step + first;
                    uint32_t row = it.src + base + t;
                    if (gather) row = __shfl(mine, static_cast<int>(t & 63u));
                    got[j] = adds && t < rows ? load_as<X>(v.src, static_cast<size_t>(row) * C + col) : identity;
                }
#pragma unroll
                for (uint32_t j = 0; j < kRowsInFlight; ++j) acc = reduce_combine(a.op, acc, got[j]);
            }
        }
        if (!one)
            for (uint32_t s = G / 2u; s >= 1u; s >>= 1) acc = reduce_combine(a.op, acc, __shfl_xor(acc, static_cast<int>(s * padded)));
        if (group == 0u && column) {
            if (final) finish<T>(a, it.dst, col, acc, v.level == 0u && len == 0u);
            else static_cast<A *>(v.next)[static_cast<size_t>(it.dst) * C + col] = acc;
        }
    }
}

// columns map: one wave per (item, slab); a lane holds V = 16 bytes of columns -- V consecutive ones where every row starts on a 16-byte
// boundary (one load per row), else columns lane, lane + 64, ...
template <typename X, typename T>
__global__ __launch_bounds__(kThreads) void reduce_columns_kernel(SegReduceArgs a, LevelArgs v, uint32_t slabs) {
    using A = typename T::A;
    using S = typename X::S;
    constexpr uint32_t V = 16u / sizeof(S), W = 64u * V;
    const uint32_t lane = threadIdx.x & 63u, C = a.C;
    const bool gather = v.level == 0u && a.order != nullptr;
    const uint32_t count = std::min(*v.item_count, v.item_cap);
    const uint64_t work = static_cast<uint64_t>(count) * slabs;
    const A identity = reduce_identity<A>(a.op);
    for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * kWaves + threadIdx.x / 64u; w < work; w += static_cast<uint64_t>(gridDim.x) * kWaves) {
        const ReduceItem it = v.items[w / slabs];
        const uint32_t slab = static_cast<uint32_t>(w % slabs);
        uint32_t len;
        bool final;
        if (!item_ok(v, a, it, &len, &final)) continue;
        uint32_t cols[V];
#pragma unroll
        for (uint32_t k = 0; k < V; ++k) cols[k] = slab * W + (v.vec_ok ? lane * V + k : k * 64u + lane);
        A acc[V];
#pragma unroll
        for (uint32_t k = 0; k < V; ++k) acc[k] = identity;
        for (uint32_t base = 0; base < len; base += 64u) {
            const uint32_t rows = std::min(64u, len - base);
            uint32_t mine = 0u;
            if (gather && lane < rows) mine = row_number(a, it.src + base + lane);
            for (uint32_t t0 = 0; t0 < rows; t0 += kRowsInFlight) {
                A got[kRowsInFlight][V];
#pragma unroll
                for (uint32_t j = 0; j < kRowsInFlight; ++j) {
                    const uint32_t t = t0 + j;
                    uint32_t row = it.src + base + t;
                    if (gather) row = __shfl(mine, static_cast<int>(t & 63u));
                    const S *p = static_cast<const S *>(v.src) + static_cast<size_t>(row) * C;
                    if (t < rows && v.vec_ok && cols[0] < C) {
                        const uint4 bits = *reinterpret_cast<const uint4 *>(p + cols[0]);
                        S s[V];
                        __builtin_memcpy(s, &bits, 16);
#pragma unroll
                        for (uint32_t k = 0; k < V; ++k) got[j][k] = reduce_widen<X>(s[k]);
                    } else {
#pragma unroll
                        for (uint32_t k = 0; k < V; ++k) got[j][k] = t < rows && !v.vec_ok && cols[k] < C ? reduce_widen<X>(p[cols[k]]) : identity;
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < kRowsInFlight; ++j)
#pragma unroll
                    for (uint32_t k = 0; k < V; ++k) acc[k] = reduce_combine(a.op, acc[k], got[j][k]);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < V; ++k) {
            if (cols[k] >= C) continue;
            if (final) finish<T>(a, it.dst, cols[k], acc[k], v.level == 0u && len == 0u);
            else static_cast<A *>(v.next)[static_cast<size_t>(it.dst) * C + cols[k]] = acc[k];
        }
    }
}

inline uint32_t grid_of(uint64_t wanted, uint32_t cap) { return static_cast<uint32_t>(std::max<uint64_t>(std::min<uint64_t>(wanted, cap), 1u)); }

template <typename X, typename T>
void launch_level(hipStream_t stream, const SegReduceArgs &a, const LevelArgs &v, uint32_t blocks_cap) {
    if (a.C < kReduceWave) {
        hipLaunchKernelGGL((reduce_rows_kernel<X, T>), dim3(grid_of((static_cast<uint64_t>(v.item_cap) + kWaves - 1u) / kWaves, blocks_cap)), dim3(kThreads), 0,
                           stream, a, v, reduce_padded_width(a.C));
    } else {
        constexpr uint32_t W = 64u * 16u / sizeof(typename X::S);
        const uint32_t slabs = (a.C + W - 1u) / W;
        hipLaunchKernelGGL((reduce_columns_kernel<X, T>), dim3(grid_of((static_cast<uint64_t>(v.item_cap) * slabs + kWaves - 1u) / kWaves, blocks_cap)),
                           dim3(kThreads), 0, stream, a, v, slabs);
    }
}

template <typename T>
hipError_t launch_as(hipStream_t stream, const SegReduceArgs &a, const ReduceLayout &L, uint32_t compute_units) {
    using A = typename T::A;
    using P = ReducePartial<A>;
    ReduceDev d{};
    d.ctl = reinterpret_cast<ReduceControl *>(a.scratch + L.control);
    d.list = reinterpret_cast<uint32_t *>(a.scratch + L.list);
    d.levels = L.levels;
    for (uint32_t k = 0; k < L.levels; ++k) {
        d.items[k] = reinterpret_cast<ReduceItem *>(a.scratch + L.items[k]);
        d.item_cap[k] = L.item_cap[k];
        d.part_cap[k] = L.part_cap[k];
    }
    const uint32_t blocks_cap = std::max(compute_units, 64u) * 16u;  // the kernels stride over what is left
    hipLaunchKernelGGL(reduce_classify_kernel, dim3(grid_of((static_cast<uint64_t>(a.num_segments) + kThreads - 1u) / kThreads, 0x7FFFFFFFu)), dim3(kThreads), 0, stream, a, d);
    hipLaunchKernelGGL((reduce_lane_kernel<T>), dim3(grid_of((static_cast<uint64_t>(a.num_segments) * a.C + kThreads - 1u) / kThreads, blocks_cap)), dim3(kThreads), 0,
                       stream, a, d);
    for (uint32_t k = 0; k < L.levels; ++k) {
        LevelArgs v{};
        v.src = k == 0u ? a.values : static_cast<const void *>(a.scratch + L.parts[k]);
        v.next = k + 1u < L.levels ? a.scratch + L.parts[k + 1u] : nullptr;
        v.items = d.items[k];
        v.item_count = &d.ctl->item_count[k];
        v.item_cap = L.item_cap[k];
        v.src_rows = L.part_cap[k];
        v.next_rows = k + 1u < L.levels ? L.part_cap[k + 1u] : 0u;
        v.level = k;
        const size_t row_bytes = static_cast<size_t>(a.C) * (k == 0u ? sizeof(typename T::S) : sizeof(A));
        v.vec_ok = reinterpret_cast<uintptr_t>(v.src) % 16u == 0u && row_bytes % 16u == 0u;
        if (k == 0u) launch_level<T, T>(stream, a, v, blocks_cap);
        else launch_level<P, T>(stream, a, v, blocks_cap);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_segment_reduce(hipStream_t stream, const SegReduceArgs &a, const ReduceLayout &L, uint32_t compute_units) {
    switch (a.dtype) {
        case kSortI32: return launch_as<ReduceI32>(stream, a, L, compute_units);
        case kSortI64: return launch_as<ReduceI64>(stream, a, L, compute_units);
        case kSortF16: return launch_as<ReduceF16>(stream, a, L, compute_units);
        case kSortBF16: return launch_as<ReduceBF16>(stream, a, L, compute_units);
        case kSortF32: return launch_as<ReduceF32>(stream, a, L, compute_units);
        default: return launch_as<ReduceF64>(stream, a, L, compute_units);
    }
}

}  // namespace vrs
