// vrs_capi_sort_rank.hip -- the C ABI of the torch.sort drop-in's two streaming kernels (vrs_sort_rank_keys, vrs_sort_restore): argument
// checks and the launches of vrs_sort_rank.hip.  The sort between them is a segmented (or one-call) sort of the ranks.  vrs_sort_restore
// with VRS_SORT_MODE is the torch.mode drop-in's reduction instead (vrs_sort_mode.hip): the longest run of every sorted row.
#include "vrs_host.hpp"
#include "vrs_sort_mode_order.hpp"
#include "vrs_sort_rank.hpp"

using namespace vrsh;

namespace {

// The flags are looked at before the context (which may be NULL here): a call that is wrong in both is refused for its flags.
int check_flags(vrs_context ctx, int flags, int known) {
    if (flags & ~known) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "sort: unknown flag bits");
    if ((flags & vrs::kSortMode) && (flags & vrs::kSortDescending))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "sort: VRS_SORT_MODE takes no VRS_SORT_DESCENDING");
    return VRS_OK;
}

// the checks both entry points share: a known dtype, uniform rows
int check_shape(vrs_context ctx, uint32_t n, uint32_t row_len, int dtype) {
    if (!vrs::sort_dtype_known(dtype)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "sort: unknown dtype");
    if (n != 0u && (row_len == 0u || n % row_len != 0u))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "sort: num_elements is not a whole number of rows of row_len");
    return VRS_OK;
}

// vrs_sort_restore with VRS_SORT_MODE: `positions` is the call's scratch, one 8-byte word per row
int sort_mode(vrs_context ctx, vrs_buffer src, vrs_buffer ranks, vrs_buffer scratch, uint32_t n, uint32_t row_len, int dtype,
              vrs_buffer out_values, vrs_buffer out_indices_i64) {
    if (!src || !ranks || !scratch || !out_values || !out_indices_i64)
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "mode: src, ranks, positions (the scratch), out_values or out_indices_i64 is NULL");
    if (n == 0u) return VRS_OK;
    const size_t en = static_cast<size_t>(n), rows = en / row_len;
    int rc;
    if ((rc = check_buffer(ctx, src, en * vrs::sort_dtype_bytes(dtype), "src")) ||
        (rc = check_buffer(ctx, ranks, en * vrs::sort_rank_bytes(dtype), "ranks")) ||
        (rc = check_buffer(ctx, scratch, rows * sizeof(uint64_t), "positions (the mode form's scratch)")) ||
        (rc = check_buffer(ctx, out_values, rows * vrs::sort_dtype_bytes(dtype), "out_values")) ||
        (rc = check_buffer(ctx, out_indices_i64, rows * sizeof(int64_t), "out_indices_i64")))
        return rc;
    if (reinterpret_cast<uintptr_t>(scratch->ptr) % sizeof(uint64_t) != 0u)
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "mode: positions (the scratch) is off an 8-byte boundary");
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    VRS_HIP(ctx, vrs::launch_sort_mode(ctx->stream, src->ptr, ranks->ptr, static_cast<uint64_t *>(scratch->ptr), n, row_len, dtype,
                                       out_values->ptr, static_cast<int64_t *>(out_indices_i64->ptr)));
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
    int rc;
    if ((rc = check_flags(ctx, flags, vrs::kSortDescending))) return rc;
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if ((rc = check_shape(ctx, num_elements, row_len, dtype))) return rc;
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
    int rc;
    if ((rc = check_flags(ctx, flags, vrs::kSortDescending | vrs::kSortMode))) return rc;
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if ((rc = check_shape(ctx, num_elements, row_len, dtype))) return rc;
    if (flags & vrs::kSortMode) return sort_mode(ctx, src, ranks, positions, num_elements, row_len, dtype, out_values, out_indices_i64);
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
