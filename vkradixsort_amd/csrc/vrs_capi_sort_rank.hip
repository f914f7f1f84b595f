// vrs_capi_sort_rank.hip -- the C ABI of the torch.sort drop-in's two streaming kernels (vrs_sort_rank_keys, vrs_sort_restore): argument
// checks and the launches of vrs_sort_rank.hip.  The sort between them is a segmented (or one-call) sort of the ranks.
#include "vrs_host.hpp"
#include "vrs_sort_rank.hpp"

using namespace vrsh;

namespace {

constexpr int kKnownSortFlags = vrs::kSortDescending;

// the checks both entry points share: a known dtype and flags, uniform rows
int check_shape(vrs_context ctx, uint32_t n, uint32_t row_len, int dtype, int flags) {
    if (!vrs::sort_dtype_known(dtype)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "sort: unknown dtype");
    if (flags & ~kKnownSortFlags) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "sort: unknown flag bits");
    if (n != 0u && (row_len == 0u || n % row_len != 0u))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "sort: num_elements is not a whole number of rows of row_len");
    return VRS_OK;
}

}  // namespace

extern "C" {

int vrs_sort_rank_bytes(int dtype, int *rank_bytes) {
    if (!rank_bytes) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "rank_bytes is NULL");
    if (!vrs::sort_dtype_known(dtype)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "sort: unknown dtype");
    *rank_bytes = vrs::sort_rank_bytes(dtype);
    return VRS_OK;
}

int vrs_sort_rank_keys(vrs_context ctx, vrs_buffer src, uint32_t num_elements, uint32_t row_len, int dtype, int flags, vrs_buffer out_ranks,
                       vrs_buffer out_positions) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    int rc;
    if ((rc = check_shape(ctx, num_elements, row_len, dtype, flags))) return rc;
    if (!src || !out_ranks) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "a buffer handle is NULL");
    const uint32_t n = num_elements;
    if (n == 0u) return VRS_OK;
    const size_t en = static_cast<size_t>(n);
    if ((rc = check_buffer(ctx, src, en * vrs::sort_dtype_bytes(dtype), "src")) ||
        (rc = check_buffer(ctx, out_ranks, en * vrs::sort_rank_bytes(dtype), "out_ranks")) ||
        (out_positions && (rc = check_buffer(ctx, out_positions, en * sizeof(uint32_t), "out_positions"))))
        return rc;
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    VRS_HIP(ctx, vrs::launch_sort_rank(ctx->stream, src->ptr, n, row_len, dtype, (flags & vrs::kSortDescending) != 0, out_ranks->ptr,
                                       out_positions ? static_cast<uint32_t *>(out_positions->ptr) : nullptr));
    return VRS_OK;
}

int vrs_sort_restore(vrs_context ctx, vrs_buffer src, vrs_buffer ranks, vrs_buffer positions, uint32_t num_elements, uint32_t row_len,
                     int dtype, int flags, vrs_buffer out_values, vrs_buffer out_indices_i64) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    int rc;
    if ((rc = check_shape(ctx, num_elements, row_len, dtype, flags))) return rc;
    if (!ranks) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "ranks is NULL");
    if (out_indices_i64 && !positions) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "sort: indices need positions");
    const bool exact_bits = out_values && vrs::sort_dtype_float(dtype);  // the ±0.0 and NaN classes read the input
    if (exact_bits && (!positions || !src))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "sort: the values of a float sort need src and positions");
    const uint32_t n = num_elements;
    if (n == 0u) return VRS_OK;
    const size_t en = static_cast<size_t>(n), vb = en * vrs::sort_dtype_bytes(dtype);
    if ((rc = check_buffer(ctx, ranks, en * vrs::sort_rank_bytes(dtype), "ranks")) ||
        (positions && (rc = check_buffer(ctx, positions, en * sizeof(uint32_t), "positions"))) ||
        (exact_bits && (rc = check_buffer(ctx, src, vb, "src"))) || (out_values && (rc = check_buffer(ctx, out_values, vb, "out_values"))) ||
        (out_indices_i64 && (rc = check_buffer(ctx, out_indices_i64, en * sizeof(int64_t), "out_indices_i64"))))
        return rc;
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    VRS_HIP(ctx, vrs::launch_sort_restore(ctx->stream, exact_bits ? src->ptr : nullptr, ranks->ptr,
                                          positions ? static_cast<const uint32_t *>(positions->ptr) : nullptr, n, row_len, dtype,
                                          (flags & vrs::kSortDescending) != 0, out_values ? out_values->ptr : nullptr,
                                          out_indices_i64 ? static_cast<int64_t *>(out_indices_i64->ptr) : nullptr));
    return VRS_OK;
}

}  // extern "C"
