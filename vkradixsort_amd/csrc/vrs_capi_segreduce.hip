// vrs_capi_segreduce.hip -- the C ABI of the segmented reduction (vrs_segment_reduce*): argument checks, the pure companions (map, levels,
// scratch size), the statistics, the order restated on the host (vrs_segment_reduce_host) and the launches of vrs_segreduce.hip.
#include "vrs_host.hpp"
#include "vrs_segreduce.hpp"

using namespace vrsh;

// device memory of a context's reductions
struct vrs_reduce_state {
    unsigned long long *stats = nullptr;  // [4] cumulative chunks per map and the deepest level count, zeroed when it is made
};

namespace vrsh {

void reduce_release(vrs_context ctx) {
    vrs_reduce_state *s = ctx->reduce;
    if (!s) return;
    if (s->stats) (void)hipFree(s->stats);
    delete s;
    ctx->reduce = nullptr;
}

}  // namespace vrsh

namespace {

int check_kind(vrs_context ctx, int dtype, int op, uint32_t row_width) {
    if (!vrs::reduce_dtype_known(dtype))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "segment_reduce: the dtype must be int32, int64, float16, bfloat16, float32 or float64");
    if (!vrs::reduce_op_known(op)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "segment_reduce: unknown op");
    if (row_width == 0u) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "segment_reduce: row_width must be 1 or more");
    return VRS_OK;
}

int check_knobs(vrs_context ctx, uint32_t chunk_rows, uint32_t lane_rows) {
    if (chunk_rows < vrs::kReduceChunkMin || chunk_rows > vrs::kReduceChunkMax)
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "segment_reduce: chunk_rows must be 64 .. 4096");
    if (lane_rows > vrs::kReduceLaneRowsMax) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "segment_reduce: lane_rows must be 0 .. 64");
    return VRS_OK;
}

bool overlap(const void *p, size_t pb, const void *q, size_t qb) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return pb != 0u && qb != 0u && a < b + qb && b < a + pb;
}

// reduce(rows) of every segment and column, by the functions the kernels compile: level by level, the partials in the accumulator type
template <typename T>
void reduce_on_host(const void *values, uint64_t n, uint32_t C, const uint32_t *order, const uint32_t *offsets, uint32_t num_segments, int op,
                    const void *init, uint32_t CH, uint32_t lane_rows, void *out) {
    using A = typename T::A;
    using S = typename T::S;
    const S *val = static_cast<const S *>(values), *ini = static_cast<const S *>(init);
    S *res = static_cast<S *>(out);
    const uint32_t n32 = static_cast<uint32_t>(std::min<uint64_t>(n, 0xFFFFFFFFull));
    std::vector<A> cur, next;
    for (uint32_t s = 0; s < num_segments; ++s) {
        const uint32_t b = offsets[s], e = offsets[s + 1u];
        const uint32_t cb = b < n32 ? b : n32, hi = e > b ? e : b, ce = hi < n32 ? hi : n32;
        const uint32_t L = ce - cb;
        for (uint32_t col = 0; col < C; ++col) {
            const size_t at = static_cast<size_t>(s) * C + col;
            if (L == 0u) {
                res[at] = ini ? ini[at] : vrs::reduce_narrow<T>(vrs::reduce_identity<A>(op));
                continue;
            }
            cur.resize(L);
            for (uint32_t t = 0; t < L; ++t) {
                const uint32_t row = order ? std::min(order[cb + t], n32 - 1u) : cb + t;
                cur[t] = vrs::reduce_widen<T>(val[static_cast<size_t>(row) * C + col]);
            }
            for (;;) {
                const uint32_t len = static_cast<uint32_t>(cur.size()), chunks = vrs::reduce_chunks(len, CH);
                next.resize(chunks);
                for (uint32_t c = 0; c < chunks; ++c) {
                    const A *rows = cur.data() + static_cast<size_t>(c) * CH;
                    next[c] = vrs::reduce_chunk<A>(op, std::min(CH, len - c * CH), C, lane_rows, [rows](uint32_t t) { return rows[t]; });
                }
                cur.swap(next);
                if (chunks == 1u) break;
            }
            A acc = cur[0];
            if (ini) acc = vrs::reduce_combine(op, vrs::reduce_widen<T>(ini[at]), acc);
            res[at] = vrs::reduce_narrow<T>(acc);
        }
    }
}

}  // namespace

extern "C" {

int vrs_segment_reduce_map_for(uint32_t chunk_len, uint32_t row_width, uint32_t lane_rows, int *map) {
    if (!map) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "map is NULL");
    if (row_width == 0u) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "segment_reduce: row_width must be 1 or more");
    if (lane_rows > vrs::kReduceLaneRowsMax) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "segment_reduce: lane_rows must be 0 .. 64");
    *map = vrs::reduce_map(chunk_len, row_width, lane_rows);
    return VRS_OK;
}

int vrs_segment_reduce_levels_for(uint32_t len, uint32_t chunk_rows, uint32_t *levels) {
    if (!levels) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "levels is NULL");
    if (const int rc = check_knobs(nullptr, chunk_rows, 0u)) return rc;
    *levels = vrs::reduce_levels(len, chunk_rows);
    return VRS_OK;
}

int vrs_segment_reduce_scratch_bytes(uint32_t num_rows, uint32_t row_width, uint32_t num_segments, int dtype, uint32_t chunk_rows, uint64_t *bytes) {
    if (!bytes) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "bytes is NULL");
    int rc;
    if ((rc = check_kind(nullptr, dtype, vrs::kReduceSum, row_width)) || (rc = check_knobs(nullptr, chunk_rows, 0u))) return rc;
    *bytes = vrs::reduce_layout(num_rows, row_width, num_segments, dtype, chunk_rows).bytes;
    return VRS_OK;
}

int vrs_segment_reduce_stats(vrs_context ctx, uint64_t *lane_chunks, uint64_t *row_chunks, uint64_t *column_chunks, uint64_t *max_levels) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    unsigned long long st[4];
    if (const int rc = read_counters(ctx, ctx->reduce ? ctx->reduce->stats : nullptr, st, 4)) return rc;
    if (lane_chunks) *lane_chunks = st[vrs::kReduceMapLane];
    if (row_chunks) *row_chunks = st[vrs::kReduceMapRows];
    if (column_chunks) *column_chunks = st[vrs::kReduceMapColumns];
    if (max_levels) *max_levels = st[3];
    return VRS_OK;
}

int vrs_segment_reduce_host(const void *values, uint64_t num_rows, uint32_t row_width, int dtype, const uint32_t *order, const uint32_t *offsets,
                            uint32_t num_segments, int op, const void *init, uint32_t chunk_rows, uint32_t lane_rows, void *out) {
    int rc;
    if ((rc = check_kind(nullptr, dtype, op, row_width)) || (rc = check_knobs(nullptr, chunk_rows, lane_rows))) return rc;
    if (num_rows >= (1ull << 32)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "segment_reduce: fewer than 2^32 rows");
    if (num_segments == 0u) return VRS_OK;
    if (!offsets || !out || (num_rows != 0u && !values)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "values, offsets or out is NULL");
    switch (dtype) {
        case vrs::kSortI32: reduce_on_host<vrs::ReduceI32>(values, num_rows, row_width, order, offsets, num_segments, op, init, chunk_rows, lane_rows, out); break;
        case vrs::kSortI64: reduce_on_host<vrs::ReduceI64>(values, num_rows, row_width, order, offsets, num_segments, op, init, chunk_rows, lane_rows, out); break;
        case vrs::kSortF16: reduce_on_host<vrs::ReduceF16>(values, num_rows, row_width, order, offsets, num_segments, op, init, chunk_rows, lane_rows, out); break;
        case vrs::kSortBF16: reduce_on_host<vrs::ReduceBF16>(values, num_rows, row_width, order, offsets, num_segments, op, init, chunk_rows, lane_rows, out); break;
        case vrs::kSortF32: reduce_on_host<vrs::ReduceF32>(values, num_rows, row_width, order, offsets, num_segments, op, init, chunk_rows, lane_rows, out); break;
        default: reduce_on_host<vrs::ReduceF64>(values, num_rows, row_width, order, offsets, num_segments, op, init, chunk_rows, lane_rows, out); break;
    }
    return VRS_OK;
}

int vrs_segment_reduce(vrs_context ctx, vrs_buffer values, uint32_t num_rows, uint32_t row_width, int dtype, vrs_buffer order, vrs_buffer offsets,
                       uint32_t num_segments, int op, vrs_buffer init, vrs_buffer out, vrs_buffer scratch) {
    int rc;
    if ((rc = check_kind(ctx, dtype, op, row_width))) return rc;
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if (!offsets || !out || !scratch || (num_rows != 0u && !values))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "a buffer handle is NULL (values, offsets, out, scratch)");
    if (num_segments == 0u) return VRS_OK;
    const size_t eb = static_cast<size_t>(vrs::sort_dtype_bytes(dtype));
    const size_t value_bytes = static_cast<size_t>(num_rows) * row_width * eb, out_bytes = static_cast<size_t>(num_segments) * row_width * eb;
    const size_t order_bytes = order ? static_cast<size_t>(num_rows) * sizeof(uint32_t) : 0u, offset_bytes = (static_cast<size_t>(num_segments) + 1u) * sizeof(uint32_t);
    const vrs::ReduceLayout L = vrs::reduce_layout(num_rows, row_width, num_segments, dtype, ctx->tune.reduce_chunk_rows);
    if ((num_rows != 0u && (rc = check_buffer(ctx, values, value_bytes, "values"))) ||
        (order && num_rows != 0u && (rc = check_buffer(ctx, order, order_bytes, "order"))) ||
        (rc = check_buffer(ctx, offsets, offset_bytes, "offsets")) || (init && (rc = check_buffer(ctx, init, out_bytes, "init"))) ||
        (rc = check_buffer(ctx, out, out_bytes, "out")) || (rc = check_buffer(ctx, scratch, L.bytes, "scratch")))
        return rc;
    const void *vp = num_rows != 0u ? values->ptr : nullptr, *op_ = order && num_rows != 0u ? order->ptr : nullptr, *ip = init ? init->ptr : nullptr;
    if (eb == 8u && ((reinterpret_cast<uintptr_t>(vp) | reinterpret_cast<uintptr_t>(ip) | reinterpret_cast<uintptr_t>(out->ptr) |
                      reinterpret_cast<uintptr_t>(scratch->ptr)) & 7u))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "segment_reduce: 8-byte elements need values, init, out and scratch on 8-byte boundaries");
    if (overlap(out->ptr, out_bytes, vp, value_bytes) || overlap(out->ptr, out_bytes, op_, order_bytes) ||
        overlap(out->ptr, out_bytes, offsets->ptr, offset_bytes) || (ip && ip != out->ptr && overlap(out->ptr, out_bytes, ip, out_bytes)))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "segment_reduce: out may not alias values, order, offsets or init (out == init is allowed)");
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    if (!ctx->reduce) ctx->reduce = new (std::nothrow) vrs_reduce_state;
    vrs_reduce_state *s = ctx->reduce;
    if (!s) return fail(ctx, VRS_ERROR_OUT_OF_MEMORY, "reduce state");
    if ((rc = make_counters(ctx, &s->stats, 4))) return rc;
    vrs::SegReduceArgs a{};
    a.values = vp;
    a.order = static_cast<const uint32_t *>(op_);
    a.offsets = static_cast<const uint32_t *>(offsets->ptr);
    a.init = ip;
    a.out = out->ptr;
    a.scratch = static_cast<char *>(scratch->ptr);
    a.n = num_rows;
    a.C = row_width;
    a.num_segments = num_segments;
    a.chunk_rows = ctx->tune.reduce_chunk_rows;
    a.lane_rows = ctx->tune.reduce_lane_rows;
    a.dtype = dtype;
    a.op = op;
    a.stats = s->stats;
    VRS_HIP(ctx, hipMemsetAsync(a.scratch + L.control, 0, sizeof(vrs::ReduceControl), ctx->stream));
    VRS_HIP(ctx, vrs::launch_segment_reduce(ctx->stream, a, L, ctx->scatter.compute_units));
    return VRS_OK;
}

}  // extern "C"
