// vrs_search.hip -- the kernels of the sorted-sequence search (vrs_search_sorted: torch.searchsorted / bucketize).
//   out = number of boundaries b of the query's row with r(b) < r(v) (left) or r(b) <= r(v) (right), r = sort_rank (torch's order).
// One query kernel in four modes; a workgroup of 1024 threads takes work items (query row, chunk of the row) from a grid-stride loop and
// every thread four consecutive queries at a time (one vector load, four interleaved searches, one vector store):
//   LDS      the boundary row's ranks, staged once per workgroup (per work item when every query row has its own boundaries), searched in LDS
//   TABLE    out = table[bit pattern of the query]; search_table_kernel searched each of the 2^8 / 2^16 patterns once
//   DIRECT   lower / upper bound in global memory, the rank map (and the sorter) applied to every probe
//   INDEXED  three levels: the index's top level in LDS, then `stride` index entries in global memory (the last five probes inside one
//            128-byte line), then the one 128-byte line of boundaries they point at.  search_index_kernel wrote the index (and, with a
//            sorter, the row's ranks gathered in order, which the last level then reads).
// Every search is the same branch-free loop over a fixed length (the row's, the stride, the line), so a wave never diverges; a probe
// past the end of a window's valid part counts as "not below", which also keeps unsorted input inside [0, m] and inside the buffers.
// Positions: base + half never exceeds the window's length, windows start at multiples of the line below m < 2^32.
// Identity queries (queries == NULL: 0, 1, 2, ... per row) take none of the four: search_identity_kernel merges, one chunk of
// kSearchChunk outputs per workgroup -- two ends by wave-wide probes, the boundaries between them counted into LDS, one prefix sum.
// Membership (VRS_SEARCH_MEMBER: torch.isin) is a template parameter of the query and table kernels: the left count by the same code,
// then one fetch of the boundary at the count -- guarded, count == m is one past the row -- search_member (vrs_search.hpp) and a byte
// per query, four of them as one word where the address allows it.
#include "vrs_search.hpp"

namespace vrs {
namespace {

template <typename S_, typename R_, bool FLOAT_, bool SIGNED_>
struct SearchTraits {
    using S = S_;
    using R = R_;
    static constexpr int B = 8 * static_cast<int>(sizeof(S_));
    __device__ static R rank(S u, R inf_bits) { return sort_rank<R, B, FLOAT_, SIGNED_>(static_cast<R>(u), inf_bits, false); }
    __device__ static bool is_nan(R r) { return search_rank_is_nan<R, B, FLOAT_>(r); }
};

template <typename E, int A>
struct alignas(A) Quad {
    E v[kSearchItems];
};
template <typename S> using QueryQuad = Quad<S, (sizeof(S) * kSearchItems < 16 ? sizeof(S) * kSearchItems : 16)>;

template <typename R>
__device__ inline bool below(R e, R v, int right) {
    return (e < v) | ((right != 0) & (e == v));
}

// count[k] = how many of the first `len` entries of the window are below v[k]; at(i, k) = entry i (i < len) for query k, or "not
// below" past the valid part.  Branch-free: log2(len) + 1 rounds whatever the data.
template <typename R, typename At>
__device__ inline void search_window(uint32_t len, const R (&v)[kSearchItems], int right, At at, uint32_t (&count)[kSearchItems]) {
#pragma unroll
    for (uint32_t k = 0; k < kSearchItems; ++k) count[k] = 0u;
    if (len == 0u) return;
    while (len > 1u) {
        const uint32_t half = len >> 1;
#pragma unroll
        for (uint32_t k = 0; k < kSearchItems; ++k) count[k] += at(count[k] + half - 1u, k, v[k]) ? half : 0u;
        len -= half;
    }
#pragma unroll
    for (uint32_t k = 0; k < kSearchItems; ++k) count[k] += at(count[k], k, v[k]) ? 1u : 0u;
}

// boundary j of a row as a rank: through the sorter (its entries clamped into the row) when there is one
template <typename T>
__device__ inline typename T::R boundary_rank(const typename T::S *row, const int64_t *sorter, uint32_t m, uint32_t j, typename T::R inf_bits) {
    const uint32_t at = sorter ? static_cast<uint32_t>(min(static_cast<unsigned long long>(sorter[j]), static_cast<unsigned long long>(m - 1u))) : j;
    return T::rank(row[at], inf_bits);
}

constexpr int kModeLds = 0, kModeTable = 1, kModeDirect = 2, kModeIndexed = 3;

// MEMBER (VRS_SEARCH_MEMBER): the left count as before, then one guarded fetch of the boundary at the count and a byte per query.
template <typename T, int MODE, bool MEMBER>
__global__ __launch_bounds__(kSearchThreads) void search_kernel(SearchArgs a) {
    using S = typename T::S;
    using R = typename T::R;
    const int right = MEMBER ? 0 : a.right;
    extern __shared__ __align__(16) unsigned char search_smem[];
    R *lds = reinterpret_cast<R *>(search_smem);
    const R inf_bits = static_cast<R>(a.inf_bits);
    const S *queries = static_cast<const S *>(a.queries);
    const uint64_t items = static_cast<uint64_t>(a.q_rows) * a.chunks_per_row;
    bool staged = false;
    for (uint64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const uint32_t q_row = static_cast<uint32_t>(w / a.chunks_per_row), chunk = static_cast<uint32_t>(w % a.chunks_per_row);
        const uint32_t b_row = a.b_rows == 1u ? 0u : q_row;
        const S *row = static_cast<const S *>(a.boundaries) + static_cast<size_t>(b_row) * a.m;
        const int64_t *sorter = a.sorter ? a.sorter + static_cast<size_t>(b_row) * a.m : nullptr;
        if ((MODE == kModeLds || MODE == kModeIndexed) && (!staged || a.b_rows != 1u)) {
            if (staged) __syncthreads();  // (the searches of the row before are done with the LDS)
            if (MODE == kModeLds) {
                for (uint32_t j = threadIdx.x; j < a.stage_len; j += kSearchThreads) lds[j] = boundary_rank<T>(row, sorter, a.m, j, inf_bits);
            } else {
                const R *top = static_cast<const R *>(a.top) + static_cast<size_t>(b_row) * a.shape.top;
                for (uint32_t j = threadIdx.x; j < a.stage_len; j += kSearchThreads) lds[j] = top[j];
            }
            __syncthreads();
            staged = true;
        }
        const uint64_t first = static_cast<uint64_t>(chunk) * a.chunk_len;  // within the query row
        const uint64_t len = min(static_cast<uint64_t>(a.q_len) - first, static_cast<uint64_t>(a.chunk_len));
        const uint64_t origin = static_cast<uint64_t>(q_row) * a.q_len + first;  // within the call
        for (uint64_t g = static_cast<uint64_t>(threadIdx.x) * kSearchItems; g < len; g += kSearchChunk) {
            const bool whole = a.vec_ok && g + kSearchItems <= len;
            S q[kSearchItems];
            if (whole) {
                const QueryQuad<S> in = *reinterpret_cast<const QueryQuad<S> *>(queries + origin + g);
#pragma unroll
                for (uint32_t k = 0; k < kSearchItems; ++k) q[k] = in.v[k];
            } else {
#pragma unroll
                for (uint32_t k = 0; k < kSearchItems; ++k) q[k] = g + k < len ? queries[origin + g + k] : S{};
            }
            uint32_t count[kSearchItems];
            if (MODE == kModeTable) {
#pragma unroll
                for (uint32_t k = 0; k < kSearchItems; ++k) count[k] = a.table[q[k]];
            } else {
                R v[kSearchItems];
#pragma unroll
                for (uint32_t k = 0; k < kSearchItems; ++k) v[k] = T::rank(q[k], inf_bits);
                const R *gathered = nullptr;
                if (MODE == kModeLds) {
                    search_window<R>(a.m, v, right, [&](uint32_t i, uint32_t, R x) { return below(lds[i], x, right); }, count);
                } else if (MODE == kModeDirect) {
                    search_window<R>(a.m, v, right,
                                     [&](uint32_t i, uint32_t, R x) { return below(boundary_rank<T>(row, sorter, a.m, i, inf_bits), x, right); }, count);
                } else {
                    const SearchIndexShape sh = a.shape;
                    const R *index = static_cast<const R *>(a.index) + static_cast<size_t>(b_row) * sh.full;
                    gathered = a.gathered ? static_cast<const R *>(a.gathered) + static_cast<size_t>(b_row) * a.m : nullptr;
                    uint32_t c0[kSearchItems], c1[kSearchItems];
                    search_window<R>(sh.top, v, right, [&](uint32_t i, uint32_t, R x) { return below(lds[i], x, right); }, c0);
                    search_window<R>(sh.stride, v, right,
                                     [&](uint32_t i, uint32_t k, R x) {
                                         const uint32_t at = c0[k] * sh.stride + i;  // (c0 * stride <= full <= 2^28 and i < stride <= max(full, 32))
                                         return at < sh.full && below(index[at], x, right);
                                     },
                                     c1);
                    uint32_t lines[kSearchItems];
#pragma unroll
                    for (uint32_t k = 0; k < kSearchItems; ++k) lines[k] = c0[k] * sh.stride + c1[k];  // <= full
                    search_window<R>(sh.line, v, right,
                                     [&](uint32_t i, uint32_t k, R x) {
                                         const uint64_t at = static_cast<uint64_t>(lines[k]) * sh.line + i;
                                         if (at >= a.m) return false;
                                         const uint32_t j = static_cast<uint32_t>(at);
                                         return below(gathered ? gathered[j] : T::rank(row[j], inf_bits), x, right);
                                     },
                                     count);
#pragma unroll
                    for (uint32_t k = 0; k < kSearchItems; ++k) count[k] += lines[k] * sh.line;  // <= m
                }
                if (MEMBER) {
                    // boundary count[k] decides, fetched only where it exists: a query above every boundary has count == m, one
                    // past the row (and past the staged ranks).  Lanes past the chunk's end hold S{} queries and are not stored.
#pragma unroll
                    for (uint32_t k = 0; k < kSearchItems; ++k) {
                        const uint32_t c = count[k];
                        R e = R{};
                        if (c < a.m) {
                            if (MODE == kModeLds) e = lds[c];
                            else if (MODE == kModeDirect) e = boundary_rank<T>(row, sorter, a.m, c, inf_bits);
                            else e = gathered ? gathered[c] : T::rank(row[c], inf_bits);
                        }
                        count[k] = search_member<R>(c, a.m, e, v[k], T::is_nan(v[k]));
                    }
                }
            }
            if (MEMBER) {
                // (the table tier's entries are the membership itself.)  Four answers as one word when the chunk is whole and the
                // address allows it (vec_ok: out 4-byte aligned, rows a multiple of four), else byte by byte.
                const uint32_t flip = a.invert ? 1u : 0u;
                unsigned char *out = static_cast<unsigned char *>(a.out) + origin + g;
                if (whole) {
                    uint32_t word = 0u;
#pragma unroll
                    for (uint32_t k = 0; k < kSearchItems; ++k) word |= (count[k] ^ flip) << (8u * k);
                    *reinterpret_cast<uint32_t *>(out) = word;
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < kSearchItems; ++k)
                        if (g + k < len) out[k] = static_cast<unsigned char>(count[k] ^ flip);
                }
            } else if (a.out64) {
                int64_t *out = static_cast<int64_t *>(a.out) + origin + g;
                if (whole) {
                    Quad<int64_t, 16> o;
#pragma unroll
                    for (uint32_t k = 0; k < kSearchItems; ++k) o.v[k] = static_cast<int64_t>(count[k]);
                    *reinterpret_cast<Quad<int64_t, 16> *>(out) = o;
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < kSearchItems; ++k)
                        if (g + k < len) out[k] = static_cast<int64_t>(count[k]);
                }
            } else {
                uint32_t *out = static_cast<uint32_t *>(a.out) + origin + g;
                if (whole) {
                    Quad<uint32_t, 16> o;
#pragma unroll
                    for (uint32_t k = 0; k < kSearchItems; ++k) o.v[k] = count[k];
                    *reinterpret_cast<Quad<uint32_t, 16> *>(out) = o;
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < kSearchItems; ++k)
                        if (g + k < len) out[k] = count[k];
                }
            }
        }
    }
}

// table[u] = the answer for a query of bit pattern u: one direct search per pattern (one shared boundary row).  MEMBER: the left count,
// then whether the pattern is a member (0 / 1 in the same 4-byte entries; the query kernel inverts).
template <typename T, bool MEMBER>
__global__ __launch_bounds__(256) void search_table_kernel(SearchArgs a, uint32_t *__restrict__ table) {
    using S = typename T::S;
    using R = typename T::R;
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;  // (the grid is exactly 2^B threads)
    const R inf_bits = static_cast<R>(a.inf_bits);
    const S *row = static_cast<const S *>(a.boundaries);
    const R v = T::rank(static_cast<S>(u), inf_bits);
    const int right = MEMBER ? 0 : a.right;
    uint32_t base = 0u, len = a.m;
    while (len > 1u) {
        const uint32_t half = len >> 1;
        base += below(boundary_rank<T>(row, a.sorter, a.m, base + half - 1u, inf_bits), v, right) ? half : 0u;
        len -= half;
    }
    if (a.m != 0u) base += below(boundary_rank<T>(row, a.sorter, a.m, base, inf_bits), v, right) ? 1u : 0u;
    if (MEMBER) {
        const R e = base < a.m ? boundary_rank<T>(row, a.sorter, a.m, base, inf_bits) : R{};  // (boundary m does not exist)
        base = search_member<R>(base, a.m, e, v, T::is_nan(v));
    }
    table[u] = base;
}

// The index of every boundary row: entry k = the rank of the last boundary of the row's k-th full line, and every stride-th of them
// again in the top level.  With a sorter the row's ranks are gathered in order on the way (one thread per boundary); without one a
// thread per index entry reads its one boundary.
template <typename T>
__global__ __launch_bounds__(256) void search_index_kernel(SearchArgs a, typename T::R *__restrict__ index, typename T::R *__restrict__ top,
                                                           typename T::R *__restrict__ gathered) {
    using S = typename T::S;
    using R = typename T::R;
    const R inf_bits = static_cast<R>(a.inf_bits);
    const SearchIndexShape sh = a.shape;
    const uint64_t per_row = gathered ? a.m : sh.full, total = per_row * a.b_rows;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; t < total; t += stride) {
        const uint32_t b_row = static_cast<uint32_t>(t / per_row), i = static_cast<uint32_t>(t % per_row);
        const S *row = static_cast<const S *>(a.boundaries) + static_cast<size_t>(b_row) * a.m;
        uint32_t k;  // the index entry this thread writes, if any
        R r;
        if (gathered) {
            r = boundary_rank<T>(row, a.sorter + static_cast<size_t>(b_row) * a.m, a.m, i, inf_bits);
            gathered[static_cast<size_t>(b_row) * a.m + i] = r;
            if (i % sh.line != sh.line - 1u) continue;
            k = i / sh.line;
        } else {
            k = i;
            r = T::rank(row[static_cast<size_t>(k) * sh.line + (sh.line - 1u)], inf_bits);
        }
        index[static_cast<size_t>(b_row) * sh.full + k] = r;
        if ((k + 1u) % sh.stride == 0u) top[static_cast<size_t>(b_row) * sh.top + (k + 1u) / sh.stride - 1u] = r;
    }
}

template <typename T, int MODE, bool MEMBER>
hipError_t launch_query(hipStream_t stream, const SearchArgs &a, uint32_t lds_entries) {
    using R = typename T::R;
    const bool uses_lds = MODE == kModeLds || MODE == kModeIndexed;
    const uint32_t lds = uses_lds ? std::max<uint32_t>((lds_entries * static_cast<uint32_t>(sizeof(R)) + 255u) & ~255u, 256u) : 0u;
    const uint64_t items = static_cast<uint64_t>(a.q_rows) * a.chunks_per_row;
    // as many workgroups as stay resident: two of 1024 threads per CU, one when its LDS is more than half a CU's
    const uint32_t resident = 256u * (uses_lds && lds > kSearchLdsMaxBytes / 2u ? 1u : 2u);
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>(items, uses_lds ? resident : 4u * resident));
    auto kernel = search_kernel<T, MODE, MEMBER>;
    if (lds > 64u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kSearchThreads), lds, stream, a);
    return hipGetLastError();
}

template <typename T, bool MEMBER>
hipError_t search_form(hipStream_t stream, SearchArgs a, int tier, const SearchLayout &L, char *scratch) {
    using R = typename T::R;
    switch (tier) {
        case kSearchTierLds:
            a.stage_len = a.m;
            return launch_query<T, kModeLds, MEMBER>(stream, a, a.m);
        case kSearchTierDirect: return launch_query<T, kModeDirect, MEMBER>(stream, a, 0u);
        case kSearchTierTable:
            if constexpr (sizeof(typename T::S) <= 2) {
                uint32_t *table = reinterpret_cast<uint32_t *>(scratch + L.table);
                hipLaunchKernelGGL((search_table_kernel<T, MEMBER>), dim3((1u << T::B) / 256u), dim3(256), 0, stream, a, table);
                if (const hipError_t e = hipGetLastError()) return e;
                a.table = table;
                return launch_query<T, kModeTable, MEMBER>(stream, a, 0u);
            } else {
                return hipErrorInvalidValue;
            }
        case kSearchTierIndexed: {
            R *index = reinterpret_cast<R *>(scratch + L.index), *top = reinterpret_cast<R *>(scratch + L.top);
            R *gathered = a.sorter ? reinterpret_cast<R *>(scratch + L.gathered) : nullptr;
            const uint64_t total = static_cast<uint64_t>(gathered ? a.m : a.shape.full) * a.b_rows;
            if (total != 0u) {
                const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>((total + 255u) / 256u, 8192u));
                hipLaunchKernelGGL(search_index_kernel<T>, dim3(blocks), dim3(256), 0, stream, a, index, top, gathered);
                if (const hipError_t e = hipGetLastError()) return e;
            }
            a.index = index;
            a.top = top;
            a.gathered = gathered;
            a.stage_len = a.shape.top;
            return launch_query<T, kModeIndexed, MEMBER>(stream, a, a.shape.top);
        }
        default: return hipErrorInvalidValue;
    }
}

// the form is a template parameter: the counting kernels are the instantiations they were
template <typename T>
hipError_t search_as(hipStream_t stream, const SearchArgs &a, int tier, const SearchLayout &L, char *scratch) {
    return a.member ? search_form<T, true>(stream, a, tier, L, scratch) : search_form<T, false>(stream, a, tier, L, scratch);
}

// ---- identity queries: the merge (vrs_search.hpp has the chunk's marking and scan)

constexpr uint32_t kSearchWaves = kSearchThreads / 64u;
static_assert(kSearchThreads * kSearchItems == kSearchChunk, "every lane of the identity kernel scans one group of a chunk");

// How many of the row's m ascending boundaries are below v (right: or equal), found by one wave: 64 evenly spaced probes and a ballot
// per round leave 1/65 of the window, so 2^32 boundaries take six dependent rounds instead of 32.  Wave-uniform result.  Every probe
// is inside the window, and the window inside the row, whatever the boundaries hold: a result in [0, m].
template <typename S>
__device__ inline uint32_t wave_count_below(const S *row, uint32_t m, int64_t v, int right) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t lo = 0u, len = m;  // the result is in [lo, lo + len]
    while (len != 0u) {
        const uint32_t step = len / 65u + 1u;          // (64 * step > len - step: what the probes leave is shorter than step)
        const uint32_t idx = (lane + 1u) * step - 1u;  // (< 2^32: step <= 2^32 / 65 + 1)
        const bool hit = idx < len && below<int64_t>(static_cast<int64_t>(row[lo + idx]), v, right);
        const uint32_t c = static_cast<uint32_t>(__popcll(__ballot(hit)));  // (c probes are inside the window: c * step <= len)
        lo += c * step;
        len = min(step - 1u, len - c * step);
    }
    return lo;
}

// the workgroup as a team of search_identity_chunk
struct SearchIdentityTeam {
    uint32_t *wave_sums;  // kSearchWaves words of LDS
    __device__ void barrier() { __syncthreads(); }
    __device__ void add(uint32_t *slot) { atomicAdd(slot, 1u); }
    __device__ uint32_t exclusive(uint32_t x) {
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        uint32_t incl = x;
#pragma unroll
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63u) wave_sums[wave] = incl;
        __syncthreads();
        uint32_t before = incl - x;
        for (uint32_t w = 0; w < wave; ++w) before += wave_sums[w];
        return before;
    }
};

template <typename S, typename O>
__global__ __launch_bounds__(kSearchThreads) void search_identity_kernel(SearchIdentityArgs a) {
    __shared__ __align__(16) uint32_t marks[kSearchChunk];
    __shared__ uint32_t wave_sums[kSearchWaves];
    __shared__ uint32_t ends[2];
    const uint64_t j0 = static_cast<uint64_t>(blockIdx.x) * kSearchChunk;
    const uint32_t n = static_cast<uint32_t>(min(a.q_len - j0, static_cast<uint64_t>(kSearchChunk)));
    SearchIdentityTeam team{wave_sums};
    for (uint64_t q_row = blockIdx.y; q_row < a.q_rows; q_row += gridDim.y) {  // (64-bit: q_row + gridDim.y may pass 2^32)
        const S *row = static_cast<const S *>(a.boundaries) + (a.b_rows == 1u ? 0u : static_cast<size_t>(q_row) * a.m);
        // waves 0 and 1 find the two ends: the answers of the chunk's first and last output
        if (threadIdx.x < 128u) {
            const uint32_t which = threadIdx.x >> 6;
            const uint32_t e = wave_count_below<S>(row, a.m, static_cast<int64_t>(j0 + (which ? n - 1u : 0u)), a.right);
            if ((threadIdx.x & 63u) == 0u) ends[which] = e;
        }
        O *out = static_cast<O *>(a.out) + static_cast<size_t>(q_row) * a.q_len + j0;
        const int vec_ok = a.vec_ok;
        __syncthreads();
        const uint32_t a0 = ends[0], a1 = ends[1];
        search_identity_chunk<S>(row, a0, a1, j0, n, a.right, marks, threadIdx.x, kSearchThreads, team,
                                 [&](uint32_t g, const uint32_t (&v)[kSearchItems], uint32_t k) {
                                     if (vec_ok && k == kSearchItems) {
                                         Quad<O, 16> o;
#pragma unroll
                                         for (uint32_t i = 0; i < kSearchItems; ++i) o.v[i] = static_cast<O>(v[i]);
                                         *reinterpret_cast<Quad<O, 16> *>(out + g) = o;
                                     } else {
                                         for (uint32_t i = 0; i < k; ++i) out[g + i] = static_cast<O>(v[i]);
                                     }
                                 });
        __syncthreads();  // (the next row's searches write `ends`, its chunk clears the marks)
    }
}

template <typename S>
hipError_t identity_as(hipStream_t stream, const SearchIdentityArgs &a) {
    const uint64_t chunks = (a.q_len + kSearchChunk - 1u) / kSearchChunk;  // (2^20 at most)
    const dim3 grid(static_cast<uint32_t>(chunks), std::min<uint32_t>(a.q_rows, 65535u));
    if (a.out64)
        hipLaunchKernelGGL((search_identity_kernel<S, int64_t>), grid, dim3(kSearchThreads), 0, stream, a);
    else
        hipLaunchKernelGGL((search_identity_kernel<S, uint32_t>), grid, dim3(kSearchThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_search_identity(hipStream_t stream, const SearchIdentityArgs &a, int dtype) {
    switch (dtype) {
        case kSortI32: return identity_as<int32_t>(stream, a);
        case kSortI64: return identity_as<int64_t>(stream, a);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_search(hipStream_t stream, SearchArgs a, int dtype, int tier, uint32_t lds_bytes, const SearchLayout &L, char *scratch) {
    a.shape = search_index_shape(a.m, dtype, lds_bytes);
    switch (dtype) {
        case kSortI8: return search_as<SearchTraits<uint8_t, uint32_t, false, true>>(stream, a, tier, L, scratch);
        case kSortU8: return search_as<SearchTraits<uint8_t, uint32_t, false, false>>(stream, a, tier, L, scratch);
        case kSortI16: return search_as<SearchTraits<uint16_t, uint32_t, false, true>>(stream, a, tier, L, scratch);
        case kSortI32: return search_as<SearchTraits<uint32_t, uint32_t, false, true>>(stream, a, tier, L, scratch);
        case kSortI64: return search_as<SearchTraits<uint64_t, uint64_t, false, true>>(stream, a, tier, L, scratch);
        case kSortF16: a.inf_bits = 0x7C00ull; return search_as<SearchTraits<uint16_t, uint32_t, true, false>>(stream, a, tier, L, scratch);
        case kSortBF16: a.inf_bits = 0x7F80ull; return search_as<SearchTraits<uint16_t, uint32_t, true, false>>(stream, a, tier, L, scratch);
        case kSortF32: a.inf_bits = 0x7F800000ull; return search_as<SearchTraits<uint32_t, uint32_t, true, false>>(stream, a, tier, L, scratch);
        case kSortF64:
            a.inf_bits = 0x7FF0000000000000ull;
            return search_as<SearchTraits<uint64_t, uint64_t, true, false>>(stream, a, tier, L, scratch);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace vrs
