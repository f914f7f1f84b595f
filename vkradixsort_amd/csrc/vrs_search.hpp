// vrs_search.hpp -- what the sorted-sequence search's kernels (vrs_search.hip) and their host side (vrs_capi_search.hip) share: the tiers
// and the function that picks one (exported as vrs_search_tier_for), the shape of the sampled index, the scratch layout and the launch
// wrapper.  Internal.
#pragma once
#include <algorithm>

#include "vrs_sort_rank.hpp"

namespace vrs {

constexpr int kSearchTierLds = 0, kSearchTierTable = 1, kSearchTierDirect = 2, kSearchTierIndexed = 3, kSearchTiers = 4;
constexpr int kSearchRight = 1, kSearchOutInt64 = 2;  // VRS_SEARCH_RIGHT, VRS_SEARCH_OUT_INT64
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

struct SearchArgs {
    const void *boundaries;   // b_rows rows of m elements of the dtype
    const int64_t *sorter;    // NULL, or b_rows rows of m positions within the row
    const void *queries;      // q_rows rows of q_len elements
    void *out;                // as many int32 / int64
    uint32_t m, b_rows, q_rows, q_len;
    int right, out64, vec_ok;  // vec_ok: every group of four queries and outputs may move as one aligned vector
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

}  // namespace vrs
