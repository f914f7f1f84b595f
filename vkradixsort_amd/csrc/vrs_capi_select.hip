// vrs_capi_select.hip -- the C ABI of the one-rank selection (vrs_select_*): argument checks, the pure companions (tier, target, scratch
// size), the statistics and the launches of vrs_select.hip.
#include "vrs_host.hpp"
#include "vrs_select.hpp"

using namespace vrsh;

// device memory of a context's selections
struct vrs_select_state {
    unsigned long long *stats = nullptr;  // [4] cumulative segments per tier and grid slots that compacted, zeroed when it is made
};

namespace vrsh {

void select_release(vrs_context ctx) {
    vrs_select_state *s = ctx->select;
    if (!s) return;
    if (s->stats) (void)hipFree(s->stats);
    delete s;
    ctx->select = nullptr;
}

}  // namespace vrsh

namespace {

bool mode_known(int mode) { return mode == vrs::kSelKth || mode == vrs::kSelMedian || mode == vrs::kSelNanMedian; }

}  // namespace

extern "C" {

int vrs_select_scratch_bytes(uint32_t num_elements, uint32_t num_segments, int dtype, uint64_t *bytes) {
    if (!bytes) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "bytes is NULL");
    if (!vrs::sort_dtype_known(dtype)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "select: unknown dtype");
    *bytes = num_segments == 0u ? 0u : vrs::select_layout(num_elements, num_segments, dtype).bytes;
    return VRS_OK;
}

int vrs_select_tier_for(uint32_t begin, uint32_t end, uint32_t num_elements, int dtype, uint32_t grid_min_keys, uint32_t *clamped_begin,
                        uint32_t *clamped_end, int *tier) {
    if (!tier || !clamped_begin || !clamped_end) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "an output pointer is NULL");
    if (!vrs::sort_dtype_known(dtype)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "select: unknown dtype");
    *tier = vrs::select_tier(begin, end, num_elements, dtype, grid_min_keys, clamped_begin, clamped_end);
    return VRS_OK;
}

int vrs_select_target_for(int mode, uint32_t k, uint32_t len, uint32_t nans, int descending, uint32_t *j, int *valid) {
    if (!j || !valid) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "an output pointer is NULL");
    if (!mode_known(mode)) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "select: unknown mode");
    if (nans > len) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "select: more NaNs than keys");
    *valid = vrs::select_target(mode, k, len, nans, descending != 0, j) ? 1 : 0;
    return VRS_OK;
}

int vrs_select_stats(vrs_context ctx, uint64_t *lds_segments, uint64_t *block_segments, uint64_t *grid_segments, uint64_t *compacted_segments) {
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    unsigned long long st[4];
    if (const int rc = read_counters(ctx, ctx->select ? ctx->select->stats : nullptr, st, 4)) return rc;
    if (lds_segments) *lds_segments = st[vrs::kTopkTierLds];
    if (block_segments) *block_segments = st[vrs::kTopkTierBlock];
    if (grid_segments) *grid_segments = st[vrs::kTopkTierGrid];
    if (compacted_segments) *compacted_segments = st[3];
    return VRS_OK;
}

int vrs_select_segments(vrs_context ctx, vrs_buffer src, uint32_t num_elements, vrs_buffer offsets, uint32_t num_segments, int dtype, int mode,
                        uint32_t k, int flags, vrs_buffer out_values, vrs_buffer out_indices, vrs_buffer scratch) {
    if (!vrs::sort_dtype_known(dtype)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "select: unknown dtype");
    if (!mode_known(mode)) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "select: unknown mode");
    if (flags & ~vrs::kSelDescending) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "select: unknown flag bits");
    if (mode == vrs::kSelKth && k == 0u) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "select: k starts at 1");
    if (!ctx) return fail(nullptr, VRS_ERROR_INVALID_ARGUMENT, "context is NULL");
    if (!src || !offsets || !out_values || !scratch) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "a buffer handle is NULL");
    if (num_segments == 0u) return VRS_OK;
    const size_t eb = static_cast<size_t>(vrs::sort_dtype_bytes(dtype));
    const vrs::SelLayout L = vrs::select_layout(num_elements, num_segments, dtype);
    int rc;
    if ((rc = check_buffer(ctx, src, static_cast<size_t>(num_elements) * eb, "src")) ||
        (rc = check_buffer(ctx, offsets, (static_cast<size_t>(num_segments) + 1u) * sizeof(uint32_t), "offsets")) ||
        (rc = check_buffer(ctx, out_values, static_cast<size_t>(num_segments) * eb, "out_values")) ||
        (out_indices && (rc = check_buffer(ctx, out_indices, static_cast<size_t>(num_segments) * sizeof(uint32_t), "out_indices"))) ||
        (rc = check_buffer(ctx, scratch, L.bytes, "scratch")))
        return rc;
    if (eb == 8u && ((reinterpret_cast<uintptr_t>(src->ptr) | reinterpret_cast<uintptr_t>(out_values->ptr) | reinterpret_cast<uintptr_t>(scratch->ptr)) & 7u))
        return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "select: 8-byte elements need src, out_values and scratch on 8-byte boundaries");
    // whatever the dtype: the control block at the scratch's head holds a 64-bit word the classification adds to atomically
    if (reinterpret_cast<uintptr_t>(scratch->ptr) & 7u) return fail(ctx, VRS_ERROR_INVALID_ARGUMENT, "select: scratch must be on an 8-byte boundary");
    VRS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = settle_pending(ctx))) return rc;
    if (!ctx->select) ctx->select = new (std::nothrow) vrs_select_state;
    vrs_select_state *s = ctx->select;
    if (!s) return fail(ctx, VRS_ERROR_OUT_OF_MEMORY, "select state");
    if ((rc = make_counters(ctx, &s->stats, 4))) return rc;
    vrs::SelectArgs a{};
    a.src = src->ptr;
    a.offsets = static_cast<const uint32_t *>(offsets->ptr);
    a.n = num_elements;
    a.num_segments = num_segments;
    a.k = k;
    a.grid_min_keys = ctx->tune.select_grid_min_keys;
    a.compact_divisor = ctx->tune.select_compact_divisor;
    a.dtype = dtype;
    a.mode = mode;
    a.flags = flags;
    a.out_values = out_values->ptr;
    a.out_indices = out_indices ? static_cast<uint32_t *>(out_indices->ptr) : nullptr;
    a.scratch = static_cast<char *>(scratch->ptr);
    a.stats = s->stats;
    VRS_HIP(ctx, vrs::launch_select(ctx->stream, a, L));
    return VRS_OK;
}

}  // extern "C"
