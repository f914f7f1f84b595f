// vrs_capi_search.hip -- the C ABI of the sorted-sequence search (vrs_search_*): argument checks, the tier decision, the scratch layout
// and the launches of vrs_search.hip, in the counting form and the membership form (VRS_SEARCH_MEMBER: a byte per query).
#include "vrs_host.hpp"
#include "vrs_search.hpp"

using namespace vrsh;

namespace {

constexpr int kKnownFlags = vrs::kSearchRight | vrs::kSearchOutInt64 | vrs::kSearchMember | vrs::kSearchMemberInvert;  // (not bits 4 and 8)

struct Shape {
    uint32_t m, b_rows, q_rows, q_len, q_per_row;  // q_rows x q_len as the kernels walk them; q_per_row: queries per boundary row
};

// the checks every entry point shares: a known dtype, whole rows, one boundary row or one per query row
int check_shape(vrs_context ctx, uint32_t num_boundaries, uint32_t boundary_row_len, uint32_t num_queries, uint32_t query_row_len, int dtype,
                Shape *s) {
    if (!vrs::sort_dtype_known(dtype)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "search: unknown dtype");
    if (num_boundaries != 0u && (boundary_row_len == 0u || num_boundaries % boundary_row_len != 0u))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "search: num_boundaries is not a whole number of rows of boundary_row_len");
    if (num_queries != 0u && (query_row_len == 0u || num_queries % query_row_len != 0u))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "search: num_queries is not a whole number of rows of query_row_len");
    const uint32_t b_rows = num_boundaries ? num_boundaries / boundary_row_len : 1u;
    const uint32_t q_rows = num_queries ? num_queries / query_row_len : b_rows;
    if (b_rows != 1u && b_rows != q_rows)
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "search: the boundaries must be one row or as many rows as the queries");
    s->m = num_boundaries ? boundary_row_len : 0u;
    s->b_rows = b_rows;
    s->q_rows = b_rows == 1u ? 1u : q_rows;
    s->q_len = b_rows == 1u ? num_queries : query_row_len;
    s->q_per_row = s->q_len;
    return VRS_OK;
}

// queries == NULL: query row i holds 0, 1, ..., query_row_len - 1 (the merge of vrs_search.hip).  Rows as the caller gave them: with
// one boundary row too, every query row starts again at 0.  No tier, no scratch, no counter of vrs_search_stats.
int search_identity(vrs_context ctx, vrs_buffer boundaries, uint32_t num_boundaries, const Shape &s, uint32_t num_queries,
                    uint32_t query_row_len, int dtype, int flags, vrs_buffer sorter, vrs_buffer out) {
    int rc;
    if (dtype != vrs::kSortI32 && dtype != vrs::kSortI64)
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "search: queries == NULL (the identity queries) takes VRS_SORT_INT32 or VRS_SORT_INT64");
    if (dtype == vrs::kSortI32 && query_row_len > (1u << 31))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "search: identity queries of VRS_SORT_INT32 end at 2^31 - 1 (query_row_len above 2^31)");
    if (sorter) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "search: queries == NULL (the identity queries) takes no sorter");
    if (!out || (num_boundaries != 0u && !boundaries)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "a buffer handle is NULL");
    const size_t eb = static_cast<size_t>(vrs::sort_dtype_bytes(dtype)), ob = (flags & vrs::kSearchOutInt64) ? 8u : 4u;
    if ((rc = check_buffer(ctx, out, num_queries * ob, "out")) ||
        (num_boundaries != 0u && (rc = check_buffer(ctx, boundaries, num_boundaries * eb, "boundaries"))))
        return rc;
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    if (s.m == 0u) {  // no boundary is below anything
        VRS_HIP(ctx, hipMemsetAsync(out->ptr, 0, num_queries * ob, ctx->stream));
        return VRS_OK;
    }
    vrs::SearchIdentityArgs a{};
    a.boundaries = boundaries->ptr;
    a.out = out->ptr;
    a.m = s.m;
    a.b_rows = s.b_rows;
    a.q_rows = num_queries / query_row_len;
    a.q_len = query_row_len;
    a.right = (flags & vrs::kSearchRight) ? 1 : 0;
    a.out64 = (flags & vrs::kSearchOutInt64) ? 1 : 0;
    a.vec_ok = reinterpret_cast<uintptr_t>(a.out) % 16u == 0u && (a.q_rows == 1u || query_row_len % vrs::kSearchItems == 0u);
    VRS_HIP(ctx, vrs::launch_search_identity(ctx->stream, a, dtype));
    return VRS_OK;
}

}  // namespace

extern "C" {

int vrs_search_tier_for(uint32_t num_boundaries, uint32_t boundary_row_len, uint32_t num_queries, uint32_t query_row_len, int dtype,
                        uint32_t lds_bytes, uint32_t table_min_queries, uint32_t index_min_queries, int *tier) {
    if (!tier) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "tier is NULL");
    Shape s;
    if (const int rc = check_shape(nullptr, num_boundaries, boundary_row_len, num_queries, query_row_len, dtype, &s)) return rc;
    *tier = vrs::search_tier(s.m, s.b_rows, s.q_per_row, dtype, lds_bytes, table_min_queries, index_min_queries);
    return VRS_OK;
}

int vrs_search_scratch_bytes(uint32_t num_boundaries, uint32_t boundary_row_len, int dtype, int has_sorter, int tier, uint64_t *bytes) {
    if (!bytes) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "bytes is NULL");
    if (tier < 0 || tier >= vrs::kSearchTiers) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "search: unknown tier");
    Shape s;
    if (const int rc = check_shape(nullptr, num_boundaries, boundary_row_len, 0u, 0u, dtype, &s)) return rc;
    if (tier == vrs::kSearchTierTable && vrs::sort_dtype_bytes(dtype) > 2)
        return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "search: the table tier takes 1- and 2-byte dtypes");
    *bytes = vrs::search_layout(s.m, s.b_rows, dtype, has_sorter != 0, tier).bytes;
    return VRS_OK;
}

int vrs_search_plan(vrs_context ctx, uint32_t num_boundaries, uint32_t boundary_row_len, uint32_t num_queries, uint32_t query_row_len,
                    int dtype, int has_sorter, int *tier, uint64_t *scratch_bytes) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if (!tier || !scratch_bytes) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "an output pointer is NULL");
    Shape s;
    if (const int rc = check_shape(ctx, num_boundaries, boundary_row_len, num_queries, query_row_len, dtype, &s)) return rc;
    *tier = vrs::search_tier(s.m, s.b_rows, s.q_per_row, dtype, ctx->tune.search_lds_bytes, ctx->tune.search_table_min_queries,
                             ctx->tune.search_index_min_queries);
    *scratch_bytes = vrs::search_layout(s.m, s.b_rows, dtype, has_sorter != 0, *tier).bytes;
    return VRS_OK;
}

int vrs_search_stats(vrs_context ctx, uint64_t *lds_calls, uint64_t *table_calls, uint64_t *direct_calls, uint64_t *indexed_calls) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if (lds_calls) *lds_calls = ctx->search_calls[vrs::kSearchTierLds];
    if (table_calls) *table_calls = ctx->search_calls[vrs::kSearchTierTable];
    if (direct_calls) *direct_calls = ctx->search_calls[vrs::kSearchTierDirect];
    if (indexed_calls) *indexed_calls = ctx->search_calls[vrs::kSearchTierIndexed];
    return VRS_OK;
}

int vrs_search_sorted(vrs_context ctx, vrs_buffer boundaries, uint32_t num_boundaries, uint32_t boundary_row_len, vrs_buffer queries,
                      uint32_t num_queries, uint32_t query_row_len, int dtype, int flags, vrs_buffer sorter, vrs_buffer out,
                      vrs_buffer scratch) {
    Shape s;
    int rc;
    if ((rc = check_shape(ctx, num_boundaries, boundary_row_len, num_queries, query_row_len, dtype, &s))) return rc;
    if (flags & ~kKnownFlags) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "search: unknown flag bits");
    const bool member = (flags & vrs::kSearchMember) != 0;
    if ((flags & vrs::kSearchMemberInvert) && !member)
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "search: VRS_SEARCH_MEMBER_INVERT is valid only together with VRS_SEARCH_MEMBER");
    if (member && (flags & (vrs::kSearchRight | vrs::kSearchOutInt64)))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "search: VRS_SEARCH_MEMBER takes neither VRS_SEARCH_RIGHT nor VRS_SEARCH_OUT_INT64 (out is one byte per query)");
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if (num_queries == 0u) return VRS_OK;
    if (!queries && member)
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "search: VRS_SEARCH_MEMBER needs queries (queries == NULL, the identity queries, has no membership form)");
    if (!queries) return search_identity(ctx, boundaries, num_boundaries, s, num_queries, query_row_len, dtype, flags, sorter, out);
    if (!out || (num_boundaries != 0u && !boundaries)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "a buffer handle is NULL");
    const int invert = (flags & vrs::kSearchMemberInvert) ? 1 : 0;
    const size_t eb = static_cast<size_t>(vrs::sort_dtype_bytes(dtype)), ob = member ? 1u : (flags & vrs::kSearchOutInt64) ? 8u : 4u;
    const int tier = vrs::search_tier(s.m, s.b_rows, s.q_per_row, dtype, ctx->tune.search_lds_bytes, ctx->tune.search_table_min_queries,
                                      ctx->tune.search_index_min_queries);
    const vrs::SearchLayout L = vrs::search_layout(s.m, s.b_rows, dtype, sorter != nullptr, tier);
    if ((rc = check_buffer(ctx, queries, num_queries * eb, "queries")) || (rc = check_buffer(ctx, out, num_queries * ob, "out")) ||
        (num_boundaries != 0u && (rc = check_buffer(ctx, boundaries, num_boundaries * eb, "boundaries"))) ||
        (num_boundaries != 0u && sorter && (rc = check_buffer(ctx, sorter, num_boundaries * sizeof(int64_t), "sorter"))))
        return rc;
    if (L.bytes != 0u) {
        if (!scratch) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "search: this call needs a scratch buffer (vrs_search_plan)");
        if ((rc = check_buffer(ctx, scratch, L.bytes, "scratch"))) return rc;
    }
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    if (s.m == 0u) {  // no boundary is below anything, nothing is a member (inverted: every byte 1)
        VRS_HIP(ctx, hipMemsetAsync(out->ptr, invert, num_queries * ob, ctx->stream));
        return VRS_OK;
    }
    vrs::SearchArgs a{};
    a.boundaries = boundaries->ptr;
    a.sorter = sorter ? static_cast<const int64_t *>(sorter->ptr) : nullptr;
    a.queries = queries->ptr;
    a.out = out->ptr;
    a.m = s.m;
    a.b_rows = s.b_rows;
    a.q_rows = s.q_rows;
    a.q_len = s.q_len;
    a.right = (flags & vrs::kSearchRight) ? 1 : 0;
    a.out64 = (flags & vrs::kSearchOutInt64) ? 1 : 0;
    a.member = member ? 1 : 0;
    a.invert = invert;
    // four answers move as one vector: 16 bytes of uint32, 32 of int64 (16-byte aligned halves), one 4-byte word of membership bytes
    const size_t q_align = std::min<size_t>(eb * vrs::kSearchItems, 16u), o_align = member ? 4u : 16u;
    a.vec_ok = reinterpret_cast<uintptr_t>(a.queries) % q_align == 0u && reinterpret_cast<uintptr_t>(a.out) % o_align == 0u &&
               (s.q_rows == 1u || s.q_len % vrs::kSearchItems == 0u);
    // work items: every chunk of a query row; with a boundary row per query row a workgroup stages that row for each of its items,
    // so a long row is cut into fewer, longer chunks (about 2048 items per call)
    const bool restages = s.b_rows != 1u && (tier == vrs::kSearchTierLds || tier == vrs::kSearchTierIndexed);
    uint64_t chunks = (static_cast<uint64_t>(s.q_len) + vrs::kSearchChunk - 1u) / vrs::kSearchChunk;
    if (restages) chunks = std::min<uint64_t>(chunks, std::max<uint32_t>(2048u / s.q_rows, 1u));
    const uint64_t per_chunk = (static_cast<uint64_t>(s.q_len) + chunks - 1u) / chunks;
    a.chunk_len = (per_chunk + vrs::kSearchChunk - 1u) / vrs::kSearchChunk * vrs::kSearchChunk;
    a.chunks_per_row = static_cast<uint32_t>((static_cast<uint64_t>(s.q_len) + a.chunk_len - 1u) / a.chunk_len);
    VRS_HIP(ctx, vrs::launch_search(ctx->stream, a, dtype, tier, ctx->tune.search_lds_bytes, L, scratch ? static_cast<char *>(scratch->ptr) : nullptr));
    ctx->search_calls[tier] += 1u;
    return VRS_OK;
}

}  // extern "C"
