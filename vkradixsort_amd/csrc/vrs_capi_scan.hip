// vrs_capi_scan.hip -- the C ABI of the prefix scan over rows (vrs_scan_rows*): argument checks, the pure companions (tier, levels, depth,
// scratch size), the statistics, the order restated on the host (vrs_scan_rows_host) and the launches of vrs_scan.hip.
#include "vrs_host.hpp"
#include "vrs_scan.hpp"

using namespace vrsh;

namespace vrsh {

void scan_release(vrs_context ctx) {
    if (ctx->scan_takeovers) (void)hipFree(ctx->scan_takeovers);
    ctx->scan_takeovers = nullptr;
}

}  // namespace vrsh

namespace {

int check_kind(vrs_context ctx, int dtype, int out_dtype, int op) {
    if (!vrs::scan_op_known(op)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "scan_rows: unknown op");
    if (!vrs::scan_kind_known(dtype, out_dtype, op))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT,
                    "scan_rows: sum and prod take int32, int64, float16, bfloat16, float32 or float64 into the same dtype, or int8, uint8, int16 or int32 "
                    "into int64; max and min take the nine dtypes of vrs_sort_dtype into the same dtype");
    return VRS_OK;
}

int check_shape(vrs_context ctx, uint32_t S, uint32_t L, uint32_t C, uint32_t T) {
    if (!vrs::scan_tile_rows_known(T)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "scan_rows: tile_rows must be a multiple of 256 in 256 .. 8192");
    if (C == 0u) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "scan_rows: row_width must be 1 or more");
    if (static_cast<uint64_t>(S) * L >= (1ull << 32)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "scan_rows: fewer than 2^32 rows in all");
    return VRS_OK;
}

template <class F>
void with_algebra(int dtype, int out_dtype, int op, F f) {
    using namespace vrs;
    if (op >= kScanMax) {
        switch (dtype) {
            case kSortI8: return f(ScanPairs<int8_t, 0>{});
            case kSortU8: return f(ScanPairs<uint8_t, 0>{});
            case kSortI16: return f(ScanPairs<int16_t, 0>{});
            case kSortI32: return f(ScanPairs<int32_t, 0>{});
            case kSortI64: return f(ScanPairs<int64_t, 0>{});
            case kSortF16: return f(ScanPairs<uint16_t, 1>{});
            case kSortBF16: return f(ScanPairs<uint16_t, 2>{});
            case kSortF32: return f(ScanPairs<float, 0>{});
            default: return f(ScanPairs<double, 0>{});
        }
    }
    if (out_dtype == kSortI64) {
        switch (dtype) {
            case kSortI8: return f(ScanArith<ReduceI64, int8_t>{});
            case kSortU8: return f(ScanArith<ReduceI64, uint8_t>{});
            case kSortI16: return f(ScanArith<ReduceI64, int16_t>{});
            case kSortI32: return f(ScanArith<ReduceI64, int32_t>{});
            default: return f(ScanArith<ReduceI64, int64_t>{});
        }
    }
    switch (out_dtype) {
        case kSortI32: return f(ScanArith<ReduceI32, int32_t>{});
        case kSortF16: return f(ScanArith<ReduceF16, uint16_t>{});
        case kSortBF16: return f(ScanArith<ReduceBF16, uint16_t>{});
        case kSortF32: return f(ScanArith<ReduceF32, float>{});
        default: return f(ScanArith<ReduceF64, double>{});
    }
}

bool overlap(const void *p, size_t pb, const void *q, size_t qb) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return pb != 0u && qb != 0u && a < b + qb && b < a + pb;
}

}  // namespace

extern "C" {

int vrs_scan_tier_for(uint32_t num_segments, uint32_t num_rows, uint32_t row_width, int dtype, int out_dtype, int op, uint32_t tile_rows,
                      uint32_t single_pass_min_rows, int *tier) {
    if (!tier) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "tier is NULL");
    int rc;
    if ((rc = check_kind(nullptr, dtype, out_dtype, op)) || (rc = check_shape(nullptr, num_segments, num_rows, row_width, tile_rows))) return rc;
    *tier = vrs::scan_tier(num_segments, num_rows, row_width, out_dtype, op, tile_rows, single_pass_min_rows);
    return VRS_OK;
}

int vrs_scan_levels_for(uint32_t num_rows, uint32_t tile_rows, uint32_t *levels) {
    if (!levels) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "levels is NULL");
    if (const int rc = check_shape(nullptr, 1u, num_rows, 1u, tile_rows)) return rc;
    *levels = vrs::scan_levels(num_rows, tile_rows);
    return VRS_OK;
}

int vrs_scan_depth_for(uint32_t num_rows, uint32_t row_width, uint32_t tile_rows, uint32_t *depth) {
    if (!depth) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "depth is NULL");
    if (const int rc = check_shape(nullptr, 1u, num_rows, row_width, tile_rows)) return rc;
    *depth = vrs::scan_depth(num_rows, row_width, tile_rows);
    return VRS_OK;
}

int vrs_scan_scratch_bytes(uint32_t num_segments, uint32_t num_rows, uint32_t row_width, int dtype, int out_dtype, int op, uint32_t tile_rows,
                           uint32_t single_pass_min_rows, uint64_t *bytes) {
    if (!bytes) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "bytes is NULL");
    int rc;
    if ((rc = check_kind(nullptr, dtype, out_dtype, op)) || (rc = check_shape(nullptr, num_segments, num_rows, row_width, tile_rows))) return rc;
    const int tier = vrs::scan_tier(num_segments, num_rows, row_width, out_dtype, op, tile_rows, single_pass_min_rows);
    *bytes = vrs::scan_layout(num_segments, num_rows, row_width, out_dtype, op, tile_rows, tier).bytes;
    return VRS_OK;
}

int vrs_scan_stats(vrs_context ctx, uint64_t *tile_calls, uint64_t *three_launch_calls, uint64_t *single_pass_calls, uint64_t *takeovers) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    unsigned long long taken[1];
    if (const int rc = read_counters(ctx, ctx->scan_takeovers, taken, 1)) return rc;
    if (tile_calls) *tile_calls = ctx->scan_calls[vrs::kScanTierTile];
    if (three_launch_calls) *three_launch_calls = ctx->scan_calls[vrs::kScanTierThreeLaunch];
    if (single_pass_calls) *single_pass_calls = ctx->scan_calls[vrs::kScanTierSinglePass];
    if (takeovers) *takeovers = taken[0];
    return VRS_OK;
}

int vrs_scan_rows_host(const void *values, uint32_t num_segments, uint32_t num_rows, uint32_t row_width, int dtype, int out_dtype, int op,
                       uint32_t tile_rows, void *out, int64_t *out_indices) {
    int rc;
    if ((rc = check_kind(nullptr, dtype, out_dtype, op)) || (rc = check_shape(nullptr, num_segments, num_rows, row_width, tile_rows))) return rc;
    if (num_segments == 0u || num_rows == 0u) return VRS_OK;
    if (!values || !out || (op >= vrs::kScanMax && !out_indices)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "values, out or out_indices is NULL");
    with_algebra(dtype, out_dtype, op, [&](auto x) {
        vrs::scan_rows_on_host<decltype(x)>(values, num_segments, num_rows, row_width, op, tile_rows, out, out_indices);
    });
    return VRS_OK;
}

int vrs_scan_rows(vrs_context ctx, vrs_buffer values, uint32_t num_segments, uint32_t num_rows, uint32_t row_width, int dtype, int out_dtype, int op,
                  vrs_buffer out, vrs_buffer out_indices, vrs_buffer scratch) {
    int rc;
    if ((rc = check_kind(ctx, dtype, out_dtype, op))) return rc;
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if ((rc = check_shape(ctx, num_segments, num_rows, row_width, ctx->tune.scan_tile_rows))) return rc;
    if (num_segments == 0u || num_rows == 0u) return VRS_OK;
    const bool pairs = op >= vrs::kScanMax;
    const int tier = vrs::scan_tier(num_segments, num_rows, row_width, out_dtype, op, ctx->tune.scan_tile_rows, ctx->tune.scan_single_pass_min_rows);
    const vrs::ScanLayout l = vrs::scan_layout(num_segments, num_rows, row_width, out_dtype, op, ctx->tune.scan_tile_rows, tier);
    if (!values || !out || (pairs && !out_indices) || (l.bytes != 0u && !scratch))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "a buffer handle is NULL (values, out, out_indices for max and min, scratch)");
    const size_t count = static_cast<size_t>(num_segments) * num_rows * row_width;
    const size_t in_bytes = count * static_cast<size_t>(vrs::sort_dtype_bytes(dtype)), out_bytes = count * static_cast<size_t>(vrs::sort_dtype_bytes(out_dtype));
    const size_t index_bytes = pairs ? count * sizeof(int64_t) : 0u;
    if ((rc = check_buffer(ctx, values, in_bytes, "values")) || (rc = check_buffer(ctx, out, out_bytes, "out")) ||
        (pairs && (rc = check_buffer(ctx, out_indices, index_bytes, "out_indices"))) || (l.bytes != 0u && (rc = check_buffer(ctx, scratch, l.bytes, "scratch"))))
        return rc;
    const void *ip = pairs ? out_indices->ptr : nullptr, *sp = l.bytes != 0u ? scratch->ptr : nullptr;
    if ((reinterpret_cast<uintptr_t>(values->ptr) % static_cast<uintptr_t>(vrs::sort_dtype_bytes(dtype))) ||
        (reinterpret_cast<uintptr_t>(out->ptr) % static_cast<uintptr_t>(vrs::sort_dtype_bytes(out_dtype))) || (reinterpret_cast<uintptr_t>(ip) & 7u) ||
        (reinterpret_cast<uintptr_t>(sp) & 15u))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "scan_rows: values and out on their element's boundary, out_indices on 8 bytes, scratch on 16");
    if (overlap(out->ptr, out_bytes, values->ptr, in_bytes) || overlap(ip, index_bytes, values->ptr, in_bytes) || overlap(ip, index_bytes, out->ptr, out_bytes) ||
        overlap(sp, l.bytes, values->ptr, in_bytes) || overlap(sp, l.bytes, out->ptr, out_bytes) || overlap(sp, l.bytes, ip, index_bytes))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "scan_rows: values, out, out_indices and scratch may not overlap");
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    if ((rc = make_counters(ctx, &ctx->scan_takeovers, 1))) return rc;
    vrs::ScanArgs a{};
    a.values = values->ptr;
    a.out = out->ptr;
    a.indices = pairs ? static_cast<int64_t *>(out_indices->ptr) : nullptr;
    a.scratch = l.bytes != 0u ? static_cast<char *>(scratch->ptr) : nullptr;
    a.S = num_segments;
    a.L = num_rows;
    a.C = row_width;
    a.T = ctx->tune.scan_tile_rows;
    a.dtype = dtype;
    a.out_dtype = out_dtype;
    a.op = op;
    a.tier = tier;
    a.spin_budget = ctx->tune.scan_spin_budget;
    a.takeovers = ctx->scan_takeovers;
    VRS_HIP(ctx, vrs::launch_scan_rows(ctx->stream, a, l, ctx->scatter.compute_units));
    ++ctx->scan_calls[tier];
    return VRS_OK;
}

}  // extern "C"
