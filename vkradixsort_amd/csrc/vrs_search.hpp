// vrs_search.hpp -- what the sorted-sequence search's kernels (vrs_search.hip) and their host side (vrs_capi_search.hip) share: the tiers
// and the function that picks one (exported as vrs_search_tier_for), the shape of the sampled index, the scratch layout and the launch
// wrapper; the identity form's chunk function (search_identity_chunk), which the merge kernel and a host program both run; and the
// membership form's decision (search_member), which every query mode, the table kernel and a host program run.  Internal.
#pragma once
#include <algorithm>

#include "vrs_sort_rank.hpp"

namespace vrs {

constexpr int kSearchTierLds = 0, kSearchTierTable = 1, kSearchTierDirect = 2, kSearchTierIndexed = 3, kSearchTiers = 4;
constexpr int kSearchRight = 1, kSearchOutInt64 = 2;  // VRS_SEARCH_RIGHT, VRS_SEARCH_OUT_INT64
constexpr int kSearchMember = 16, kSearchMemberInvert = 32;  // VRS_SEARCH_MEMBER, VRS_SEARCH_MEMBER_INVERT (bits 4 and 8: unknown, refused)
constexpr uint32_t kSearchThreads = 1024u, kSearchItems = 4u, kSearchChunk = kSearchThreads * kSearchItems;  // queries per workgroup pass
constexpr uint32_t kSearchLine = 128u;  // bytes of boundaries one index entry stands for: what a query's last global fetch brings in
// The measured settings (DESIGN "K10", profiles/labs/k10_searchsorted.txt):
constexpr uint32_t kSearchLdsMaxBytes = 160u * 1024u;          // what a workgroup can claim at all
constexpr uint32_t kSearchDefaultLdsBytes = 64u * 1024u;       // VRS_TUNE_SEARCH_LDS_BYTES: a row's ranks up to this many bytes are searched in LDS
constexpr uint32_t kSearchDefaultTableMinQueries = 1u << 16;   // VRS_TUNE_SEARCH_TABLE_MIN_QUERIES (2-byte dtypes; 1-byte dtypes: 1/256 of it)
constexpr uint32_t kSearchDefaultIndexMinQueries = 1u << 16;   // VRS_TUNE_SEARCH_INDEX_MIN_QUERIES (queries per boundary row)

__host__ __device__ inline uint32_t search_line_elems(int dtype) { return kSearchLine / static_cast<uint32_t>(sort_dtype_bytes(dtype)); }

// The queries from which a narrow dtype takes the table tier (0: never).
__host__ __device__ inline uint32_t search_table_min(int dtype, uint32_t table_min_queries) {
    if (table_min_queries == 0u || sort_dtype_bytes(dtype) > 2) return 0u;
    return sort_dtype_bytes(dtype) == 2 ? table_min_queries : std::max(table_min_queries >> 8, 1u);
}

// The tier of a call: m boundaries per row in b_rows rows (1: shared by every query), q_per_row queries per boundary row.
//   table   -- 1- and 2-byte dtypes, one shared row, enough queries to pay for searching every bit pattern once
//   LDS     -- the row's ranks fit lds_bytes (empty rows included)
//   indexed -- longer rows with index_min_queries or more queries each (0: never)
//   direct  -- everything else
__host__ __device__ inline int search_tier(uint32_t m, uint32_t b_rows, uint32_t q_per_row, int dtype, uint32_t lds_bytes,
                                           uint32_t table_min_queries, uint32_t index_min_queries) {
    const uint32_t tmin = search_table_min(dtype, table_min_queries);
    if (tmin != 0u && b_rows == 1u && m != 0u && q_per_row >= tmin) return kSearchTierTable;
    if (static_cast<uint64_t>(m) * static_cast<uint32_t>(sort_rank_bytes(dtype)) <= std::min(lds_bytes, kSearchLdsMaxBytes)) return kSearchTierLds;
    if (index_min_queries != 0u && q_per_row >= index_min_queries) return kSearchTierIndexed;
    return kSearchTierDirect;
}

// The sampled index of one boundary row of m elements: entry k = the rank of boundary (k + 1) * line - 1 (the last of the k-th full
// 128-byte line), `full` entries; its top level, staged in LDS, = every stride-th entry of those (top entry j = entry (j + 1) * stride - 1),
// stride a power of two of at least 32 (one 128-byte line of 4-byte index entries) chosen so that the top level fits lds_bytes.
struct SearchIndexShape {
    uint32_t line, full, stride, top;
};
__host__ __device__ inline SearchIndexShape search_index_shape(uint32_t m, int dtype, uint32_t lds_bytes) {
    SearchIndexShape s{};
    s.line = search_line_elems(dtype);
    s.full = m / s.line;
    const uint32_t cap = std::max(std::min(lds_bytes, kSearchLdsMaxBytes) / static_cast<uint32_t>(sort_rank_bytes(dtype)), 1u);
    s.stride = 32u;
    while (s.full / s.stride > cap) s.stride <<= 1;  // (full < 2^32: ends at 2^31 at the latest, where full / stride <= 1)
    s.top = s.full / s.stride;
    return s;
}

// the scratch buffer's layout: the same function sizes it (vrs_search_scratch_bytes) and cuts it (the call).  Independent of the LDS
// capacity in force: the top level is sized for its smallest stride.
struct SearchLayout {
    size_t table, index, top, gathered, bytes;  // byte offsets
};
inline SearchLayout search_layout(uint32_t m, uint32_t b_rows, int dtype, bool sorter, int tier) {
    auto up = [](size_t x) { return (x + 255u) & ~static_cast<size_t>(255u); };
    const size_t rb = static_cast<size_t>(sort_rank_bytes(dtype));
    SearchLayout L{};
    size_t at = 0;
    L.table = at;
    if (tier == kSearchTierTable) at += up(sizeof(uint32_t) << (8 * sort_dtype_bytes(dtype)));
    L.index = at;
    if (tier == kSearchTierIndexed) {
        const size_t full = m / search_line_elems(dtype);
        at += up(static_cast<size_t>(b_rows) * full * rb);
        L.top = at;
        at += up(static_cast<size_t>(b_rows) * (full / 32u) * rb);
        L.gathered = at;
        if (sorter) at += up(static_cast<size_t>(b_rows) * m * rb);
    }
    L.bytes = at;
    return L;
}

// ---- Membership (VRS_SEARCH_MEMBER: torch.isin / numpy.isin).  The decision, written once for the four query modes, the table kernel
// and a host program: with c = the left count of a query of rank v among the m boundaries of its row (c <= m, boundaries ascending),
// the query is a member exactly when boundary c exists and has the query's rank -- unless the query is of the NaN class, which IEEE ==
// makes a member of nothing, a row of NaNs included (every NaN has one rank, so the ranks alone would say "member").  -0.0 and +0.0
// share a rank: each is a member of a row that holds the other.  rank_at_c: the rank of boundary c when c < m, ANY value otherwise --
// the caller must not fetch boundary m (a query above every boundary has c == m), and this function does not look at it then.
template <typename R>
__host__ __device__ inline uint32_t search_member(uint32_t c, uint32_t m, R rank_at_c, R v, bool v_is_nan) {
    return (c < m && rank_at_c == v && !v_is_nan) ? 1u : 0u;
}
// whether rank r (sort_rank, ascending) is the NaN class of a B-bit float: its largest rank (an integer's largest rank is its largest value)
template <typename R, int B, bool FLOAT>
__host__ __device__ inline bool search_rank_is_nan(R r) {
    constexpr R sign = static_cast<R>(1) << (B - 1);
    return FLOAT && r == (sign | (sign - 1));
}

struct SearchArgs {
    const void *boundaries;   // b_rows rows of m elements of the dtype
    const int64_t *sorter;    // NULL, or b_rows rows of m positions within the row
    const void *queries;      // q_rows rows of q_len elements
    void *out;                // as many int32 / int64; membership form: as many bytes
    uint32_t m, b_rows, q_rows, q_len;
    int right, out64, vec_ok;  // vec_ok: every group of four queries and outputs may move as one aligned vector
    int member, invert;        // the membership form (right == 0, out64 == 0): out bytes are membership ^ invert
    unsigned long long inf_bits;
    uint32_t chunks_per_row;  // work items per query row
    unsigned long long chunk_len;  // queries of a work item (a multiple of kSearchChunk)
    uint32_t stage_len;       // entries a workgroup stages per boundary row: m (LDS tier) or the index's top level
    const void *index, *top, *gathered;  // the indexed tier's scratch areas (gathered: with a sorter)
    SearchIndexShape shape;
    const uint32_t *table;
};

// the launches of one call in `tier` (the table / index build included)
hipError_t launch_search(hipStream_t stream, SearchArgs a, int dtype, int tier, uint32_t lds_bytes, const SearchLayout &L, char *scratch);

// ---- Identity queries (vrs_search_sorted with queries == NULL: query row i holds 0, 1, ..., q_len - 1): a merge, not a search.
// One work item is a chunk of kSearchChunk consecutive outputs [j0, j0 + n) of a row.  With a0 = the answer for j0 and a1 = the answer
// for the chunk's last output, the boundaries [a0, a1) of the row are exactly those that change the answer inside the chunk: boundary b
// raises it by one from output b on (right: b <= j) or from output b + 1 on (left: b < j).  So every such boundary adds one to a counter
// at its output's place in the chunk, and the answers are a0 + the inclusive prefix sums of those counters.

// The place in the chunk [j0, j0 + n) from which boundary b counts, or n when it is outside (ascending boundaries within [a0, a1) never
// are; ones that are not ascending may be anywhere).  lo = j0 - 1 >= -1 and b >= lo, so the difference is exact in uint64.
__host__ __device__ inline uint32_t search_identity_place(int64_t b, uint64_t j0, uint32_t n, int right) {
    const int64_t lo = static_cast<int64_t>(j0) - (right ? 0 : 1);
    if (b < lo) return n;
    const uint64_t p = static_cast<uint64_t>(b) - static_cast<uint64_t>(lo);
    return p < n ? static_cast<uint32_t>(p) : n;
}

// The marking and the scan of one chunk over plain arrays, written for a team of `threads` lanes of which this is lane `tid`.  The
// kernel runs it with kSearchThreads lanes, marks in LDS and a Team whose add() is an LDS atomic, whose barrier() is the workgroup's and
// whose exclusive() is a workgroup scan; a host program runs the same code with one lane (SearchIdentitySerial).
//   row    the boundary row (S = int32_t or int64_t); entries [a0, a1) are read, in pieces of kSearchChunk however many there are
//   marks  kSearchChunk words, contents on entry unspecified
//   store  store(g, v, k): outputs g .. g + k - 1 of the chunk (g a multiple of kSearchItems, k <= kSearchItems) are v[0 .. k - 1]
// Team::exclusive(x) returns the sum of the x of every earlier call in lane order (lane 0's first call, lane 1's first call, ...);
// every lane of a workgroup team calls it exactly once, which static_asserts in the kernel hold to kSearchThreads * kSearchItems ==
// kSearchChunk.  Every answer lies in [a0, max(a0, a1)] whatever the boundaries hold.
template <typename S, typename Team, typename Store>
__host__ __device__ inline void search_identity_chunk(const S *row, uint32_t a0, uint32_t a1, uint64_t j0, uint32_t n, int right,
                                                      uint32_t *marks, uint32_t tid, uint32_t threads, Team &team, Store store) {
    for (uint32_t g = tid; g < kSearchChunk; g += threads) marks[g] = 0u;
    team.barrier();
    for (uint64_t base = a0; base < a1; base += kSearchChunk) {  // (64-bit: base + kSearchChunk may pass 2^32)
        const uint64_t end = base + kSearchChunk < a1 ? base + kSearchChunk : a1;
        for (uint64_t i = base + tid; i < end; i += threads) {
            const uint32_t p = search_identity_place(static_cast<int64_t>(row[i]), j0, n, right);
            if (p < n) team.add(marks + p);
        }
    }
    team.barrier();
    for (uint32_t g = tid * kSearchItems; g < kSearchChunk; g += threads * kSearchItems) {
        uint32_t v[kSearchItems];
        uint32_t sum = 0u;
        for (uint32_t k = 0; k < kSearchItems; ++k) v[k] = sum += marks[g + k];
        const uint32_t before = a0 + team.exclusive(sum);
        for (uint32_t k = 0; k < kSearchItems; ++k) v[k] += before;
        if (g < n) store(g, v, n - g < kSearchItems ? n - g : kSearchItems);
    }
}

// the team of one: what a host program (or a single device lane) passes
struct SearchIdentitySerial {
    uint32_t running = 0u;
    __host__ __device__ void barrier() {}
    __host__ __device__ void add(uint32_t *slot) { *slot += 1u; }
    __host__ __device__ uint32_t exclusive(uint32_t x) {
        const uint32_t r = running;
        running += x;
        return r;
    }
};

struct SearchIdentityArgs {
    const void *boundaries;  // b_rows rows of m elements of int32 / int64
    void *out;               // q_rows x q_len uint32 / int64
    uint32_t m, b_rows, q_rows;
    uint64_t q_len;          // outputs per row (below 2^32)
    int right, out64, vec_ok;  // vec_ok: every group of four outputs may move as aligned 16-byte vectors
};

// the one launch of an identity call (dtype: kSortI32 or kSortI64; m, q_rows and q_len all nonzero)
hipError_t launch_search_identity(hipStream_t stream, const SearchIdentityArgs &a, int dtype);

}  // namespace vrs
